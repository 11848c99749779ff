"""The model of smx_recon_decimate_mesh (include/smx.h): vertex clustering in numpy, vectorised with lexsort and unique.

Every quantity of the contract is an integer or a float32 expression written out below operation by operation (numpy
rounds each float32 operation once and never contracts a * b + c), so results are compared with the library's for
equality.  Deliberately another route than the kernels': cells and duplicates are found by sorting, where
smx_decimate.hip uses two hash tables with 64-bit atomics."""
import numpy as np

INVALID = np.uint32(0xFFFFFFFF)
CELL_LIMIT = 1 << 20


class CellRangeError(ValueError):
    """A cell coordinate of a used vertex lies outside [-2^20, 2^20): the cell is too small for the extent of the map."""


def live_mask(pos32, r2):
    return ~(np.asarray(r2) < 0) & np.all(np.isfinite(pos32), axis=1)


def canonical(tri):
    """Each row rotated so that its smallest index comes first (the winding is kept)."""
    tri = np.asarray(tri).reshape(-1, 3)
    k = np.argmin(tri, axis=1)
    rows = np.arange(tri.shape[0])
    return np.stack([tri[rows, k], tri[rows, (k + 1) % 3], tri[rows, (k + 2) % 3]], axis=1)


def decimate(pos, r2, triangles, cell_size):
    """pos [n, 3] smooth positions, r2 [n] RadiusSquared, triangles [T, 3] slot indices, cell_size > 0.
    Returns (triangles_out [T_out, 3] uint32, vertex_map [n] uint32, stats dict)."""
    pos32 = np.ascontiguousarray(np.asarray(pos), dtype=np.float32)
    n = pos32.shape[0]
    tri = np.asarray(triangles, dtype=np.uint32).reshape(-1, 3)
    cell = np.float32(cell_size)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError("cell_size must be finite and > 0")
    if tri.size and int(tri.max()) >= n:
        raise ValueError("an index is >= the slot count")
    stats = dict(n_in=tri.shape[0], n_not_live=0, n_used_vertices=0, n_cells=0, n_collapsed=0, n_duplicates=0, n_triangles=0)
    vmap = np.full(n, INVALID, np.uint32)
    live = live_mask(pos32, r2)
    t = tri.astype(np.int64)
    keep = np.all(live[t], axis=1) if t.size else np.zeros(0, bool)
    stats["n_not_live"] = int(t.shape[0] - keep.sum())
    t = t[keep]
    used = np.unique(t)
    stats["n_used_vertices"] = int(used.size)
    if used.size == 0:
        return np.zeros((0, 3), np.uint32), vmap, stats
    # ---- cells (float32, one operation at a time)
    inv = np.float32(1.0) / cell
    x = pos32[used]
    c = np.floor(x * inv)
    if not np.all((c >= -CELL_LIMIT) & (c < CELL_LIMIT)):
        raise CellRangeError("cell_size %g is too small for the extent of the map" % float(cell))
    ci = c.astype(np.int64)
    key = ((ci[:, 0] + CELL_LIMIT) << 42) | ((ci[:, 1] + CELL_LIMIT) << 21) | (ci[:, 2] + CELL_LIMIT)
    centre = (ci.astype(np.float32) + np.float32(0.5)) * cell
    d = x - centre
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == np.float32
    word = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | used.astype(np.uint64)
    order = np.lexsort((word, key))
    first = np.ones(order.size, bool)
    first[1:] = key[order][1:] != key[order][:-1]
    stats["n_cells"] = int(first.sum())
    rep_sorted = used[order][np.maximum.accumulate(np.where(first, np.arange(order.size), 0))]
    vmap[used[order]] = rep_sorted.astype(np.uint32)
    # ---- triangles
    m = vmap[t].astype(np.int64)
    collapsed = (m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2]) | (m[:, 0] == m[:, 2])
    stats["n_collapsed"] = int(collapsed.sum())
    m = m[~collapsed]
    if m.shape[0]:
        _, first_at = np.unique(np.sort(m, axis=1), axis=0, return_index=True)   # (the first occurrence of each corner set)
    else:
        first_at = np.zeros(0, np.int64)
    stats["n_duplicates"] = int(m.shape[0] - first_at.size)
    out = canonical(m[np.sort(first_at)])
    out = out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))].astype(np.uint32)
    stats["n_triangles"] = int(out.shape[0])
    return out, vmap, stats


def check_properties(out, vmap, stats):
    out = np.asarray(out).reshape(-1, 3).astype(np.int64)
    assert stats["n_in"] == stats["n_not_live"] + stats["n_collapsed"] + stats["n_duplicates"] + stats["n_triangles"]
    assert stats["n_triangles"] == out.shape[0]
    reps = np.unique(vmap[vmap != INVALID])
    assert reps.size == stats["n_cells"]
    assert np.array_equal(vmap[reps], reps), "vertex_map is not idempotent on representatives"
    assert int(np.sum(vmap != INVALID)) == stats["n_used_vertices"]
    if out.shape[0] == 0:
        return
    assert np.all(out[:, 0] < out[:, 1]) and np.all(out[:, 0] < out[:, 2]), "the smallest index is not first"
    a, b = out[:-1], out[1:]
    ordered = (a[:, 0] < b[:, 0]) | ((a[:, 0] == b[:, 0]) & ((a[:, 1] < b[:, 1]) | ((a[:, 1] == b[:, 1]) & (a[:, 2] < b[:, 2]))))
    assert np.all(ordered), "not in format order"
    assert np.unique(np.sort(out, axis=1), axis=0).shape[0] == out.shape[0], "a set of three corners occurs twice"
    assert np.all(np.isin(out, reps)), "an index is not a representative"
