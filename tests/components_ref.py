"""The model of smx_recon_mesh_components (include/smx.h): connected components of a triangle array in numpy.

Every quantity of the contract is an integer or a float32 expression written out below operation by operation (numpy
rounds each float32 operation once and never contracts a * b + c), so results are compared with the library's for
equality.  Deliberately another route than the kernels': labels spread by rounds of "take the smallest label across every
edge, then jump to the label's label" over whole arrays, where smx_components.hip runs a lock-free union-find."""
import numpy as np

INVALID = np.uint32(0xFFFFFFFF)
COMPONENT_DTYPE = np.dtype([("label", "<u4"), ("n_vertices", "<u4"), ("n_triangles", "<u4"), ("kept", "<u4"),
                            ("lo", "<f4", (3,)), ("hi", "<f4", (3,))])
STAT_NAMES = ("n_in", "n_not_live", "n_used_vertices", "n_components", "n_kept_components", "n_largest_triangles", "n_triangles")


def live_mask(pos32, r2):
    return ~(np.asarray(r2) < 0) & np.all(np.isfinite(pos32), axis=1)


def order_key(f):
    """k(f) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000): uint32 keys that order as the floats do, -0 below +0."""
    bits = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return bits ^ np.where((bits >> np.uint32(31)) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def order_unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    bits = np.where((k >> np.uint32(31)) != 0, k ^ np.uint32(0x80000000), ~k)
    return bits.astype(np.uint32).view(np.float32)


def diag2_of(lo, hi):
    d = hi.astype(np.float32) - lo.astype(np.float32)
    out = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert out.dtype == np.float32
    return out


def labels_of(n, t):
    """label[i] = the smallest slot of i's component for the slots in t ([T,3] int64), INVALID elsewhere."""
    lab = np.arange(n, dtype=np.int64)
    u = np.concatenate([t[:, 0], t[:, 0]])
    v = np.concatenate([t[:, 1], t[:, 2]])
    while True:
        m = np.minimum(lab[u], lab[v])
        new = lab.copy()
        np.minimum.at(new, u, m)
        np.minimum.at(new, v, m)
        while True:                      # (a label is a slot of the same component with a label no larger)
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            break
        lab = new
    out = np.full(n, INVALID, np.uint32)
    used = np.unique(t)
    out[used] = lab[used].astype(np.uint32)
    return out, used


def components(pos, r2, triangles, min_triangles=0, min_diagonal=0.0, keep_largest=0):
    """pos [n, 3] smooth positions, r2 [n] RadiusSquared, triangles [T, 3] slot indices in any order.
    Returns (triangles_out [T_out, 3] uint32, vertex_labels [n] uint32, table [n_components] COMPONENT_DTYPE, stats dict)."""
    pos32 = np.ascontiguousarray(np.asarray(pos), dtype=np.float32)
    n = pos32.shape[0]
    tri = np.asarray(triangles, dtype=np.uint32).reshape(-1, 3)
    mind = np.float32(min_diagonal)
    if not (np.isfinite(mind) and mind >= 0):
        raise ValueError("min_diagonal must be finite and >= 0")
    if tri.size and int(tri.max()) >= n:
        raise ValueError("an index is >= the slot count")
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats["n_in"] = tri.shape[0]
    live = live_mask(pos32, r2)
    t_all = tri.astype(np.int64)
    remaining = np.all(live[t_all], axis=1) if t_all.size else np.zeros(0, bool)
    stats["n_not_live"] = int(t_all.shape[0] - remaining.sum())
    t = t_all[remaining]
    labels, used = labels_of(n, t)
    stats["n_used_vertices"] = int(used.size)
    roots = np.unique(labels[used])                      # ascending: the table's order
    C = roots.size
    stats["n_components"] = int(C)
    table = np.zeros(C, COMPONENT_DTYPE)
    if C == 0:
        return np.zeros((0, 3), np.uint32), labels, table, stats
    comp_of_vertex = np.searchsorted(roots, labels[used])
    comp_of_tri = np.searchsorted(roots, labels[t[:, 0]])
    table["label"] = roots
    table["n_vertices"] = np.bincount(comp_of_vertex, minlength=C)
    table["n_triangles"] = np.bincount(comp_of_tri, minlength=C)
    keys = order_key(pos32[used])                        # [|U|, 3]
    lo = np.full((C, 3), 0xFFFFFFFF, np.uint32)
    hi = np.zeros((C, 3), np.uint32)
    for k in range(3):
        np.minimum.at(lo[:, k], comp_of_vertex, keys[:, k])
        np.maximum.at(hi[:, k], comp_of_vertex, keys[:, k])
    table["lo"], table["hi"] = order_unkey(lo), order_unkey(hi)
    d2 = diag2_of(table["lo"], table["hi"])
    passes = (table["n_triangles"] >= np.uint32(min_triangles)) & (d2 >= mind * mind)
    kept = passes.copy()
    if keep_largest > 0:
        rank = np.lexsort((table["label"], -table["n_triangles"].astype(np.int64)))   # (n_triangles descending, label ascending)
        rank = rank[passes[rank]]
        kept[:] = False
        kept[rank[:keep_largest]] = True
    table["kept"] = kept
    stats["n_kept_components"] = int(kept.sum())
    stats["n_largest_triangles"] = int(table["n_triangles"].max())
    keep_tri = np.zeros(tri.shape[0], bool)
    keep_tri[np.flatnonzero(remaining)] = kept[comp_of_tri]
    out = tri[keep_tri]
    stats["n_triangles"] = int(out.shape[0])
    return out, labels, table, stats


def check_properties(tri_in, out, labels, table, stats):
    tri_in = np.asarray(tri_in, np.uint32).reshape(-1, 3)
    out = np.asarray(out, np.uint32).reshape(-1, 3)
    assert stats["n_triangles"] == out.shape[0] and stats["n_components"] == table.shape[0]
    # the output is a subsequence of the input: greedy matching of whole rows, in order
    j = 0
    for row in tri_in:
        if j < out.shape[0] and np.array_equal(row, out[j]):
            j += 1
    assert j == out.shape[0], "the output is not a subsequence of the input"
    # every kept label is a table row with kept == 1, and the table is ascending by label
    assert np.all(np.diff(table["label"].astype(np.int64)) > 0), "the table is not ascending by label"
    if out.shape[0]:
        lab = labels[out.astype(np.int64)]
        assert np.all(lab[:, 0] == lab[:, 1]) and np.all(lab[:, 0] == lab[:, 2]) and np.all(lab[:, 0] != INVALID)
        rows = np.searchsorted(table["label"], lab[:, 0])
        assert np.all(table["label"][rows] == lab[:, 0]) and np.all(table["kept"][rows] == 1)
    assert int(table["kept"].sum()) == stats["n_kept_components"] and set(np.unique(table["kept"])) <= {0, 1}
    assert int(table["n_triangles"][table["kept"] == 1].sum()) == out.shape[0]
    # the counts add up
    assert int(table["n_triangles"].sum()) == stats["n_in"] - stats["n_not_live"]
    assert int(table["n_vertices"].sum()) == stats["n_used_vertices"] == int(np.sum(labels != INVALID))
    assert stats["n_largest_triangles"] == (int(table["n_triangles"].max()) if table.shape[0] else 0)
    # the labels are minima: every label labels itself, is no larger than its slot, and is a table row
    used = np.flatnonzero(labels != INVALID)
    lab = labels[used]
    assert np.all(lab <= used) and np.array_equal(labels[lab.astype(np.int64)], lab)
    assert np.array_equal(np.unique(lab), table["label"])
