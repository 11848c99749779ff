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


# One decision of the contract changed each (decimate(..., mutant=name)): what tests/test_decimate_cases.py has to notice.
MUTANTS = {
    "trunc": "the cell coordinate truncated towards zero instead of floor",
    "div": "x / cell_size instead of x * inv",
    "centre_distributed": "the centre as c * cell_size + 0.5 * cell_size",
    "d2_fma_z": "d2 = fmaf(dz, dz, dx * dx + dy * dy)",
    "d2_fma_y": "d2 = fmaf(dy, dy, dx * dx) + dz * dz",
    "d2_fma_both": "d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)): what a compiler that contracts makes of the expression",
    "d2_assoc": "d2 = dx * dx + (dy * dy + dz * dz)",
    "ftz": "x * inv flushed to zero when subnormal",
    "tie_high": "equal d2 bits go to the higher slot",
    "key_shift20": "the fields of the cell key shifted by 20 and 40 instead of 21 and 42",
    "range_hi_far": "c = 2^20 accepted",
    "range_hi_early": "c = 2^20 - 1 refused",
    "range_lo_far": "c = -2^20 - 1 accepted",
    "range_lo_early": "c = -2^20 refused",
    "same_winding_only": "a duplicate is recognised in the same winding only",
    "latest_duplicate": "the latest triangle of a corner set survives",
    "sorted_triple": "the output triple sorted instead of rotated",
    "no_r0r2": "the collapse test without r0 == r2",
    "u_all_live": "U holds the live corners of all triangles, dropped ones included",
    "bits_minus_1": "the sort key of the order built as (a << (bits - 1)) | b",
}


def fmaf(a, b, c):
    """float32 a * b + c rounded once.  The product of two float32 is exact in float64; the sum is rounded to odd in float64
    (two-sum gives the sign of what the addition lost), which the final rounding to float32 cannot tell from the exact sum."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
        fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        towards = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, towards), s)
        return s.astype(np.float32)


def d2_of(dx, dy, dz, form=None):
    """(dx dx + dy dy) + dz dz in float32, one rounding per operation; form: one of the d2_* mutants instead."""
    if form == "d2_fma_z":
        return fmaf(dz, dz, dx * dx + dy * dy)
    if form == "d2_fma_y":
        return fmaf(dy, dy, dx * dx) + dz * dz
    if form == "d2_fma_both":
        return fmaf(dz, dz, fmaf(dy, dy, dx * dx))
    if form == "d2_assoc":
        return dx * dx + (dy * dy + dz * dz)
    return (dx * dx + dy * dy) + dz * dz


def sort_bits(n):
    """Bits of the largest slot index, at least 1: the width of one field of the order's sort key."""
    return max(1, int(n - 1).bit_length())


def decimate(pos, r2, triangles, cell_size, mutant=None):
    """pos [n, 3] smooth positions, r2 [n] RadiusSquared, triangles [T, 3] slot indices, cell_size > 0.
    Returns (triangles_out [T_out, 3] uint32, vertex_map [n] uint32, stats dict).  mutant: a name of MUTANTS, for tests."""
    assert mutant is None or mutant in MUTANTS, mutant
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
    if mutant == "u_all_live":
        every = tri.astype(np.int64).reshape(-1)
        used = np.unique(every[live[every]])
    stats["n_used_vertices"] = int(used.size)
    if used.size == 0:
        return np.zeros((0, 3), np.uint32), vmap, stats
    # ---- cells (float32, one operation at a time)
    inv = np.float32(1.0) / cell
    x = pos32[used]
    with np.errstate(all="ignore"):
        scaled = x / cell if mutant == "div" else x * inv
    if mutant == "ftz":
        scaled = np.where(np.abs(scaled) < np.finfo(np.float32).tiny, np.copysign(np.float32(0), scaled), scaled)
    c = np.trunc(scaled) if mutant == "trunc" else np.floor(scaled)
    lo = -CELL_LIMIT + {"range_lo_far": -1, "range_lo_early": 1}.get(mutant, 0)
    hi = CELL_LIMIT + {"range_hi_far": 1, "range_hi_early": -1}.get(mutant, 0)
    if not np.all((c >= lo) & (c < hi)):
        raise CellRangeError("cell_size %g is too small for the extent of the map" % float(cell))
    ci = c.astype(np.int64)
    s1, s2 = (20, 40) if mutant == "key_shift20" else (21, 42)
    key = ((ci[:, 0] + CELL_LIMIT) << s2) | ((ci[:, 1] + CELL_LIMIT) << s1) | (ci[:, 2] + CELL_LIMIT)
    with np.errstate(over="ignore", invalid="ignore"):
        if mutant == "centre_distributed":
            centre = ci.astype(np.float32) * cell + np.float32(0.5) * cell
        else:
            centre = (ci.astype(np.float32) + np.float32(0.5)) * cell
        d = x - centre
        d2 = d2_of(d[:, 0], d[:, 1], d[:, 2], mutant)
    assert d2.dtype == np.float32
    low = ~used.astype(np.uint32) if mutant == "tie_high" else used.astype(np.uint32)
    word = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)
    order = np.lexsort((word, key))
    first = np.ones(order.size, bool)
    first[1:] = key[order][1:] != key[order][:-1]
    stats["n_cells"] = int(first.sum())
    rep_sorted = used[order][np.maximum.accumulate(np.where(first, np.arange(order.size), 0))]
    vmap[used[order]] = rep_sorted.astype(np.uint32)
    # ---- triangles
    m = vmap[t].astype(np.int64)
    collapsed = (m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2])
    if mutant != "no_r0r2":
        collapsed |= m[:, 0] == m[:, 2]
    stats["n_collapsed"] = int(collapsed.sum())
    m = m[~collapsed]
    if m.shape[0]:
        sets = canonical(m) if mutant == "same_winding_only" else np.sort(m, axis=1)
        if mutant == "latest_duplicate":
            _, last_at = np.unique(sets[::-1], axis=0, return_index=True)
            first_at = m.shape[0] - 1 - last_at
        else:
            _, first_at = np.unique(sets, axis=0, return_index=True)             # (the first occurrence of each corner set)
    else:
        first_at = np.zeros(0, np.int64)
    stats["n_duplicates"] = int(m.shape[0] - first_at.size)
    out = canonical(m[np.sort(first_at)])
    if mutant == "sorted_triple":
        out = np.sort(out, axis=1)
    if mutant == "bits_minus_1":
        ab = (out[:, 1].astype(np.uint64) << np.uint64(sort_bits(n) - 1)) | out[:, 2].astype(np.uint64)
        out = out[np.lexsort((ab, out[:, 0]))].astype(np.uint32)
    else:
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
