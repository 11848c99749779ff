"""The occupancy bit grid of smx_rayscene in numpy, for the tests: the occupied cell box and the cells with entries of the world
of tests/distance_ref.py at a given cell size (from raycast_ref.boxes), which block sizes fit the cap, and the set bits."""
import numpy as np

import raycast_ref as rr

MAX_BITS = 1 << 31
MAX_LOG2 = 6
SETTINGS = (-1, 0, 1, 4)      # occupancy: none, the library chooses, k = 0, k = 3
_GRIDS = {}


def grid(pos, r2, tri, c):
    """dict(lo, hi: [3] int64 occupied box (None without entries), cells: [n, 3] int64 the distinct cells with entries)."""
    key = (id(pos), id(tri), float(c))
    if key not in _GRIDS:
        lo, hi, wide, _ = rr.boxes(pos, r2, tri, c)
        lo, hi = lo[~wide], hi[~wide]
        dims = hi - lo + 1
        count = dims[:, 0] * dims[:, 1] * dims[:, 2]
        cells = []
        for j in range(rr.WIDE_CELLS):
            m = count > j
            if not np.any(m):
                break
            nx, ny = dims[m, 0], dims[m, 1]
            cells.append(np.stack([lo[m, 0] + j % nx, lo[m, 1] + (j // nx) % ny, lo[m, 2] + j // (nx * ny)], axis=1))
        cells = np.unique(np.concatenate(cells), axis=0) if cells else np.zeros((0, 3), np.int64)
        _GRIDS[key] = dict(lo=lo.min(axis=0) if lo.size else None, hi=hi.max(axis=0) if hi.size else None, cells=cells)
    return _GRIDS[key]


def bits(g, k):
    if g["lo"] is None:
        return 0
    nb = ((g["hi"] - g["lo"]) >> k) + 1
    return int(nb[0]) * int(nb[1]) * int(nb[2])


def fits(g, k):
    return bits(g, k) <= MAX_BITS


def smallest(g):
    for k in range(MAX_LOG2 + 1):
        if fits(g, k):
            return k
    return -1


def blocks_set(g, k):
    """The number of distinct blocks of 2^k cells per axis that hold a cell with entries."""
    if g["lo"] is None:
        return 0
    b = (g["cells"] - g["lo"]) >> k
    nb = ((g["hi"] - g["lo"]) >> k) + 1
    return int(np.unique((b[:, 2] * nb[1] + b[:, 1]) * nb[0] + b[:, 0]).size)
