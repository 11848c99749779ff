"""What the tests of smx_distscene add to tests/distance_ref.py (a plain module, no fixtures): the first-record rule of the
contract (include/smx.h) in numpy, and the case lists.  The model of a query is distance_ref's brute force as it stands: a scene
answers what smx_recon_mesh_distance answers."""
import numpy as np

import distance_ref as dr

WIDE_BIT = 0x80000000
NO_REC = 0xFFFFFFFF
# (max_distance of the build, the explicit cell_size): at these the winners come from the wide list for nearly every point,
# from both, and from cell records only (distance_ref.structure: n_wide 9553 / 361 / 0 of the world's triangles)
BUILDS = ((0.002, 0.00225), (0.02, 0.0225), (0.5, 0.5625))
# a build also runs once with the library's choice and once with everything in 8 cells
OTHER_CELLS = (0.0, 100.0)
# the first points of "vertices 0 / 1 / 5 mm": the edges of the 256-point workgroup
TILE_SET = "vertices 0 / 1 / 5 mm"
TILE_PREFIXES = (1, 255, 256, 257, 512)


def queries(bound):
    """Every max_distance of distance_ref.MAX_DISTANCES a scene built for `bound` answers."""
    return tuple(q for q in dr.MAX_DISTANCES if dr.F(q) <= dr.F(bound))


def first_records(pos, r2, tri, cell):
    """first_rec of the contract for the cell size c = `cell` (as used, float32): per input triangle the smallest position among
    its records in the cell records -- the entries ordered by (cell key, t), which is what a stable sort by cell key of the
    entries written triangle after triangle gives --, WIDE_BIT for a triangle on the wide list (its position there is the order
    of arrival: any), NO_REC outside R.  Returns (first [n_in] uint32, wide [n_in] bool)."""
    pos32 = np.asarray(pos).astype(dr.F)
    R, t_of, _ = dr.classify(pos, r2, tri)
    n_in = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3).shape[0]
    c = dr.F(cell)
    p = pos32[R.astype(np.int64)]
    lo = np.floor(p.min(axis=1) / c).astype(np.int64)
    hi = np.floor(p.max(axis=1) / c).astype(np.int64)
    dims = hi - lo + 1
    cells = dims[:, 0] * dims[:, 1] * dims[:, 2]
    wide = cells > dr.WIDE_CELLS
    keys, ts = [], []
    for j in range(dr.WIDE_CELLS):
        m = ~wide & (cells > j)
        if not np.any(m):
            break
        nx, ny = dims[m, 0], dims[m, 1]
        cx, cy, cz = lo[m, 0] + j % nx, lo[m, 1] + (j // nx) % ny, lo[m, 2] + j // (nx * ny)
        keys.append(((cx + (1 << 20)) << 42) | ((cy + (1 << 20)) << 21) | (cz + (1 << 20)))
        ts.append(t_of[m].astype(np.int64))
    first = np.full(n_in, NO_REC, np.uint32)
    is_wide = np.zeros(n_in, bool)
    is_wide[t_of[wide]] = True
    first[t_of[wide]] = WIDE_BIT
    if keys:
        key, t = np.concatenate(keys), np.concatenate(ts)
        order = np.lexsort((t, key))
        smallest = np.full(n_in, NO_REC, np.int64)
        np.minimum.at(smallest, t[order], np.arange(order.size, dtype=np.int64))
        got = smallest != NO_REC
        first[got] = smallest[got].astype(np.uint32)
    return first, is_wide
