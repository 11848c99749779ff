"""The cases of the shared triangle-grid build: one small map, 64 points, 64 rays and the triangle arrays at
whose sizes the build can go wrong.  Every case is run through smx_recon_mesh_distance, smx_recon_raycast_mesh and a scene by
tests/test_gpu_trigrid.py and compared with the brute-force models of distance_ref.py and raycast_ref.py; test_trigrid_model.py
checks on the CPU that the models express every case."""
import functools

import numpy as np

import distance_ref as dr
import raycast_ref as rr

F = np.float32
SIDE = 20                    # the map: SIDE x SIDE slots 2 cm apart on a wavy sheet, then one dead slot and one at 65 m
DEAD, FAR = SIDE * SIDE, SIDE * SIDE + 1
EXPLICIT = 0.03              # above both services' lower bounds at MAX_DISTANCE
MAX_DISTANCE = 0.02
T_RANGE = (0.0, 8.0)


@functools.lru_cache(maxsize=None)
def world():
    """(pos, nrm, r2, sheet): 402 slots and the 722 triangles of the sheet in a fixed shuffled order.  Read-only."""
    rng = np.random.default_rng(41)
    i, j = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    x, y = 0.02 * i.ravel() - 0.19, 0.02 * j.ravel() - 0.19
    z = 0.004 * np.sin(9.0 * x) * np.cos(7.0 * y) + rng.uniform(-0.0005, 0.0005, x.size)
    pos = np.concatenate([np.stack([x, y, z], axis=1), [[0.0, 0.0, 0.05], [65.0, 0.0, 0.0]]]).astype(F).astype(np.float64)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (pos.shape[0], 1))
    r2 = np.full(pos.shape[0], 1e-4)
    r2[DEAD] = -1.0
    a = (i[:-1, :-1] * SIDE + j[:-1, :-1]).ravel()
    quads = np.concatenate([np.stack([a, a + SIDE, a + 1], axis=1), np.stack([a + SIDE, a + SIDE + 1, a + 1], axis=1)])
    sheet = np.ascontiguousarray(quads[rng.permutation(quads.shape[0])], np.uint32)
    for arr in (pos, nrm, r2, sheet):
        arr.setflags(write=False)
    return pos, nrm, r2, sheet


@functools.lru_cache(maxsize=None)
def queries():
    """(points [64, 3], rays [64, 6]) float32, read-only: on and a little off the sheet, with one BAD entry and one far away."""
    pos, _, _, sheet = world()
    rng = np.random.default_rng(43)
    T = sheet[:62].astype(np.int64)
    cen = (pos[T[:, 0]] + pos[T[:, 1]] + pos[T[:, 2]]) / 3.0
    lift = np.tile([0.0, 0.0005, 0.004, -0.002, 0.015, 0.03], 11)[:62]
    pts = np.concatenate([cen + np.stack([np.zeros(62), np.zeros(62), lift], axis=1), [[np.nan, 0.0, 0.0], [3.0, 3.0, 3.0]]])
    d = np.stack([rng.uniform(-0.2, 0.2, 62), rng.uniform(-0.2, 0.2, 62), np.where(np.arange(62) % 5 == 4, 1.0, -1.0)], axis=1)
    o = cen - 2.0 * d
    rays = np.concatenate([np.concatenate([o, d], axis=1), [[0.0, 0.0, 1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 0.0, 0.0, 1.0]]])
    pts, rays = np.ascontiguousarray(pts, F), np.ascontiguousarray(rays, F)
    pts.setflags(write=False)
    rays.setflags(write=False)
    return pts, rays


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(tri [n, 3] uint32 read-only, cells: the cell_size settings, max_distance)."""
    _, _, _, sheet = world()
    corner = lambda a, b: a * SIDE + b                                               # noqa: E731
    long_one = [corner(0, 0), corner(SIDE - 1, 0), corner(0, SIDE - 1)]               # spans the sheet: wide at every cell size used
    out = {}
    for n in (0, 1, 255, 256, 257):
        out["n_in = %d" % n] = dict(tri=sheet[:n])
    # 2 cm boxes in 2 mm cells: at least 10 x 10 cells each, above the 64 of the wide list (the distance's c >= 1.125 mm)
    out["every triangle wide"] = dict(tri=sheet[:130], cells=(2.0 ** -9,), max_distance=0.001)
    none = np.array([[DEAD, 0, 1], [2, 2, 3], [FAR, 4, 5], [6, DEAD, 6]] * 18, np.uint32)[:70]
    out["no triangle in R"] = dict(tri=none)
    mix = sheet[:200].copy()
    mix[10] = long_one
    mix[63] = [5, DEAD, 6]
    mix[64] = [7, 8, 7]
    mix[127] = [FAR, 9, 10]
    mix[128] = long_one[::-1]
    out["wide list, entries and drops at lanes 63 and 64"] = dict(tri=mix)
    for c in out.values():
        c.setdefault("cells", (EXPLICIT, 0.0))
        c.setdefault("max_distance", MAX_DISTANCE)
        c["tri"] = np.ascontiguousarray(c["tri"], np.uint32).reshape(-1, 3)
        c["tri"].setflags(write=False)
    return out


def auto_cell(pos, r2, tri):
    """What cell_size 0 asks for: the mean over R of the largest box extent, summed in 2^-20 m as the build sums it."""
    R, _, _ = dr.classify(pos, r2, tri)
    if R.shape[0] == 0:
        return F(0.0)
    p = np.asarray(pos).astype(F)[R.astype(np.int64)]
    ext = (p.max(axis=1) - p.min(axis=1)).astype(F).max(axis=1)
    total = int((ext * F(1048576.0)).astype(np.uint64).sum())
    return F(float(total) / float(R.shape[0]) * (1.0 / 1048576.0))


def distance_cell(pos, r2, tri, cell_size, max_distance):
    return float(dr.cell_used(cell_size if cell_size > 0 else auto_cell(pos, r2, tri), max_distance))


def raycast_cell(pos, r2, tri, cell_size):
    return float(rr.cell_used(cell_size if cell_size > 0 else auto_cell(pos, r2, tri)))
