"""The exact model of smx_distscene_register (include/smx.h), shared by the host, API and GPU tests.  Test
infrastructure; numpy, no GPU.

What it is made of, none of it the code under test:
  * the move and the row in numpy float32, each operation of the contract one numpy operation (one rounding each);
  * the association by distance_ref.brute -- every moved sample against every triangle of R, no grid -- with the gate applied
    afterwards, as distance_ref.answer does;
  * the sums in the order of the launch by track_exact.launch_sum (workgroups of 256, a lane's samples one after the other,
    the cross-lane tree, the wavefronts in index order, the slabs in index order);
  * the solve by track_ref.solve and the pose chain by track_exact.next_pose.
An iteration's sums are evaluated at the 12 floats the implementation RECORDED for it where a record is given (exact_call's
`recorded`), so that equality never depends on the last bit of a double sin or cos.

`mutant` turns one decision of the model the other way (MUTANTS); tests/test_register_kernel_host.py shows that each of them
changes the sums of a named case.  The fixtures: the world of tests/distance_ref.py, and corner(), three mutually
perpendicular, slightly jittered vertex grids on which all six degrees of freedom can be observed."""
import functools
import math

import numpy as np

import distance_ref as dr
import track_exact as te
import track_ref as tr

F, f64 = np.float32, np.float64
INVALID = dr.INVALID
N_SUMS = 31
BUILDS = ((0.02, 0.0225), (0.5, 0.5625))          # (bound, cell_size) of the two scene builds every case runs against
WHERE = ("BAD", "not matched", "collinear winner", "normal gate failed", "inlier")
BAD, UNMATCHED, COLLINEAR, NORMAL_GATE, INLIER = range(5)

MUTANTS = {
    "gate_lt": "d^2 < q^2 ('<' for '<=')",
    "angle_gt": "m . N > cos(max angle) ('>' for '>=')",
    "collinear_inlier": "a winner without an area is not skipped",
    "tie_last": "of the triangles at the winner's distance the LAST wins",
    "winding_reversed": "g = e2 x e1",
    "right_twist": "J = (N x p', N)",
    "bad_counted": "a BAD moved point counts in [29]",
    "move_order": "p' = (R00 x + (R01 y + R02 z)) + t0",
    "stride_floor": "a level has floor(n / stride) samples",
    "waves_reversed": te.MUTANTS["waves_reversed"],
    "lanes_strided": te.MUTANTS["lanes_strided"],
    "slabs_reversed": te.MUTANTS["slabs_reversed"],
    "clamp255": te.MUTANTS["clamp255"],
}


class Params:
    """Mirror of smx_register_params with the defaults of smx_register_params_default(); levels: (stride, iterations,
    max_distance) with 0 = the scene's bound."""

    def __init__(self, levels=((4, 4, 0.0), (2, 5, 0.0), (1, 10, 0.0)), max_normal_angle_deg=30.0, convergence_rotation=1e-5,
                 convergence_translation=1e-5, min_inliers=50, min_inlier_fraction=0.1, min_pivot_ratio=1e-6):
        self.levels = tuple((int(lv[0]), int(lv[1]), float(F(lv[2] if len(lv) > 2 else 0.0))) for lv in levels)
        self.max_normal_angle_deg = float(F(max_normal_angle_deg))
        self.convergence_rotation = float(F(convergence_rotation))
        self.convergence_translation = float(F(convergence_translation))
        self.min_inliers = int(min_inliers)
        self.min_inlier_fraction = float(F(min_inlier_fraction))
        self.min_pivot_ratio = float(F(min_pivot_ratio))

    def cos_max(self):
        return F(np.cos(np.deg2rad(f64(self.max_normal_angle_deg))))

    def fields(self):
        """The keyword arguments of meshing.register_params / RegisterParams.defaults for these parameters."""
        return dict(levels=self.levels, max_normal_angle_deg=self.max_normal_angle_deg, convergence_rotation=self.convergence_rotation,
                    convergence_translation=self.convergence_translation, min_inliers=self.min_inliers,
                    min_inlier_fraction=self.min_inlier_fraction, min_pivot_ratio=self.min_pivot_ratio)


class Mesh:
    """A map (pos, r2) and a triangle array over it, as the scene was built from them."""

    def __init__(self, pos, nrm, r2, tri):
        self.pos, self.nrm, self.r2, self.tri = pos, nrm, r2, np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
        self.pos32 = np.asarray(pos).astype(F)
        self._seen = {}

    def nearest(self, moved, mutant=None):
        """distance_ref.brute of the DISTINCT rows of `moved`, handed back per row (a tiled point set costs one tile)."""
        moved = np.ascontiguousarray(moved, F).reshape(-1, 3)
        if moved.shape[0] == 0:
            return dict(d2=np.zeros(0, F), t=np.zeros(0, np.uint32), Q=np.zeros((0, 3), F), bad=np.zeros(0, bool))
        key = (moved.tobytes(), mutant == "tie_last")
        if key in self._seen:             # (the same moved points again: another mutant of the sum order, the other build)
            return self._seen[key]
        rows, inverse = np.unique(moved.view(np.dtype((np.void, 12))).reshape(-1), return_inverse=True)
        uniq = rows.view(F).reshape(-1, 3)
        m = dr.brute(self.pos, self.r2, self.tri, uniq)
        out = {k: m[k] for k in ("d2", "t", "Q", "bad")}
        if mutant == "tie_last" and uniq.shape[0]:
            out = dict(out, t=self._last_of_ties(uniq, m))
        out = {k: v[inverse.reshape(-1)] for k, v in out.items()}
        if len(self._seen) < 64 and moved.shape[0] <= 8192:
            self._seen[key] = out
        return out

    def _last_of_ties(self, pts, m):
        R, t_of, _ = dr.classify(self.pos, self.r2, self.tri)
        t = m["t"].copy()
        corners = [tuple(self.pos32[R[:, c].astype(np.int64), k][None, :] for k in range(3)) for c in range(3)]
        for i in np.flatnonzero(m["ties"] > 1):
            P = tuple(pts[i:i + 1, k][:, None] for k in range(3))
            d2 = dr._dist2(P, dr._closest(P, *corners)[0])[0]
            t[i] = t_of[np.flatnonzero(d2 == m["d2"][i])].max()
        return t


def move(Tf, pts, rotate_only=False, mutant=None):
    """p' = ((R00 x + R01 y) + R02 z) + t0 and its two siblings in float32; rotate_only: m = R n, summed in the same order."""
    T = np.asarray(Tf, F).reshape(3, 4)
    p = np.ascontiguousarray(pts, F).reshape(-1, 3)
    out = np.zeros_like(p)
    with np.errstate(all="ignore"):
        for k in range(3):
            if mutant == "move_order" and not rotate_only:
                v = T[k, 0] * p[:, 0] + (T[k, 1] * p[:, 1] + T[k, 2] * p[:, 2])
            else:
                v = (T[k, 0] * p[:, 0] + T[k, 1] * p[:, 1]) + T[k, 2] * p[:, 2]
            out[:, k] = v if rotate_only else v + T[k, 3]
    return out


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def n_samples(n, stride, mutant=None):
    return n // stride if mutant == "stride_floor" else -(-n // stride)


def iteration(mesh, pts, nrm, Tf, stride, q, cos_max, mutant=None):
    """(sums float64 [31], detail) of one iteration at the pose Tf (12 float32 values) with gate q.  detail: where [m] of WHERE,
    t [m], moved [m, 3], wide-list membership is the caller's to work out."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    m = n_samples(pts.shape[0], stride, mutant)
    S = pts[::stride][:m]
    moved = move(Tf, S, mutant=mutant)
    near = mesh.nearest(moved, mutant)
    q2 = F(q) * F(q)
    with np.errstate(all="ignore"):
        matched = ~near["bad"] & ((near["d2"] < q2) if mutant == "gate_lt" else (near["d2"] <= q2))
        where = np.where(near["bad"], BAD, np.where(matched, INLIER, UNMATCHED))
        idx = np.flatnonzero(matched)
        t = near["t"][idx].astype(np.int64)
        A, B, C = (mesh.pos32[mesh.tri[t, k].astype(np.int64)] for k in range(3))
        e1, e2 = B - A, C - A
        g = _cross(e2, e1) if mutant == "winding_reversed" else _cross(e1, e2)
        len2 = _dot(g, g)
        area = len2 > 0
        if mutant == "collinear_inlier":
            area = np.ones_like(area)
        N = g / np.sqrt(len2)[:, None]
        gate = np.ones(idx.size, bool)
        if nrm is not None:
            mm = move(Tf, np.ascontiguousarray(nrm, F).reshape(-1, 3)[::stride][:m][idx], rotate_only=True)
            dots = _dot(mm, N)
            gate = (dots > cos_max) if mutant == "angle_gt" else (dots >= cos_max)
        where[idx] = np.where(~area, COLLINEAR, np.where(~gate, NORMAL_GATE, INLIER))
        inl = area & gate
        P, Q, N = moved[idx][inl], near["Q"][idx][inl], N[inl]
        r = _dot(N, P - Q)
        J = np.concatenate([_cross(N, P) if mutant == "right_twist" else _cross(P, N), N], axis=1).astype(F)
        counts = np.zeros((m, 4), np.int64)
        counts[:, 0] = where == INLIER
        counts[:, 1] = np.ones(m, bool) if mutant == "bad_counted" else where != BAD
        counts[:, 2] = where >= COLLINEAR
        launch = mutant if mutant in ("waves_reversed", "lanes_strided", "slabs_reversed", "clamp255") else None
        sums = te.launch_sum(m, idx[inl], te._rows(J, r, r), np.zeros(0, np.int64), np.zeros((0, 28)), counts, False, launch)
    return sums, dict(where=where, t=near["t"], d2=near["d2"], moved=moved, m=m)


def exact_call(mesh, pts, nrm, T_init, params, bound, recorded=None, mutant=None):
    """The whole call.  recorded: the implementation's records (dicts with Tf and x): every iteration's sums are then evaluated at
    the recorded Tf and the poses follow the recorded twists (the restatement's own solve is returned as x_ref, to be compared
    with a tolerance).  Returns a dict: records (level, stride, status, sums, x, x_ref, Tf, Tf_own, detail), status,
    iterations_run, T (float64 [3, 4]), scene_T_points float32 [3, 4], inliers, points_used, rms_residual, last_update_rotation,
    last_update_translation, information float32 [6, 6]."""
    T = np.asarray(T_init, F).astype(f64).reshape(3, 4)
    T_prev = T.copy()
    status, records, converged_level = tr.OK, [], -1
    cos_max = params.cos_max()
    for level, (stride, iters, q) in enumerate(params.levels):
        for _ in range(iters):
            if status >= tr.TOO_FEW_INLIERS or converged_level == level:
                break
            own = T.astype(F)
            k = len(records)
            Tf = np.asarray(recorded[k]["Tf"], F).reshape(3, 4) if recorded is not None and k < len(recorded) else own
            sums, detail = iteration(mesh, pts, nrm, Tf, stride, q if q != 0 else bound, cos_max, mutant)
            st, x_ref, _ = tr.solve(sums, T, params)
            x = np.asarray(recorded[k]["x"], f64) if recorded is not None and k < len(recorded) else x_ref
            if st < tr.TOO_FEW_INLIERS:
                conv = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) < params.convergence_rotation and \
                    math.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]) < params.convergence_translation
                st = tr.CONVERGED if conv else tr.OK
                T_prev, T = T, te.next_pose(x, Tf)
            status = st
            records.append(dict(level=level, stride=stride, status=st, sums=sums, x=x, x_ref=x_ref, Tf=Tf, Tf_own=own, detail=detail))
            if st == tr.CONVERGED:
                converged_level = level
    last = records[-1] if records else None
    if last is not None and status < tr.TOO_FEW_INLIERS and last["sums"][tr.S_INLIERS] < params.min_inlier_fraction * last["sums"][tr.S_PIXELS]:
        status, T = tr.TOO_FEW_INLIERS, T_prev
    s = last["sums"] if last else np.zeros(N_SUMS)
    x = last["x"] if last else np.zeros(6)
    info = np.zeros((6, 6), F)
    e = 0
    for i in range(6):
        for j in range(i, 6):
            info[i, j] = info[j, i] = F(s[e])
            e += 1
    return dict(records=records, status=status, iterations_run=len(records), T=T, scene_T_points=T.astype(F),
                inliers=int(s[tr.S_INLIERS]), points_used=int(s[tr.S_PIXELS]),
                rms_residual=F(math.sqrt(s[tr.S_RR] / s[tr.S_INLIERS])) if s[tr.S_INLIERS] > 0 else F(0),
                last_update_rotation=F(math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])),
                last_update_translation=F(math.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])), information=info)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
def pose(rotvec, t):
    """A [3, 4] float32 pose from a rotation vector (radians) and a translation."""
    R = tr.se3_exp(np.concatenate([np.asarray(rotvec, f64), np.zeros(3)]))[:, :3]
    return np.concatenate([R, np.asarray(t, f64).reshape(3, 1)], axis=1).astype(F)


IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def world_mesh():
    pos, nrm, r2, tri, _ = dr.world()
    return Mesh(pos, nrm, r2, tri)


@functools.lru_cache(maxsize=None)
def hand_mesh():
    """The world's map under its twelve hand-made triangles alone: few enough for half a million DISTINCT samples."""
    pos, nrm, r2, tri, info = dr.world()
    return Mesh(pos, nrm, r2, tri[info["hand_tri"]:])


CORNER_N, CORNER_SPACING = 24, 0.02


@functools.lru_cache(maxsize=None)
def corner():
    """(pos, nrm, r2, tri): three mutually perpendicular 24 x 24 vertex grids at 0.02 m spacing meeting at the origin (the planes
    z = 0, x = 0 and y = 0 over the positive quadrant, each vertex jittered by up to 0.4 mm), triangulated directly, two
    triangles per grid square wound counter-clockwise about the grid's normal.  1728 slots, 3174 triangles.  Read-only."""
    rng = np.random.default_rng(5)
    n, s = CORNER_N, CORNER_SPACING
    u, v = np.meshgrid(np.arange(n) * s + 0.01, np.arange(n) * s + 0.01, indexing="ij")
    u, v, z = u.reshape(-1), v.reshape(-1), np.zeros(n * n)
    # (axis of the normal, then the two in-plane axes in right-handed order: normal = e_a x e_b)
    grids, normals, tris = [], [], []
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = (i * n + j).reshape(-1), ((i + 1) * n + j).reshape(-1), ((i + 1) * n + j + 1).reshape(-1), (i * n + j + 1).reshape(-1)
    quad = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])
    for k, axes in enumerate(((0, 1, 2), (1, 2, 0), (2, 0, 1))):          # (u axis, v axis, normal axis)
        p = np.zeros((n * n, 3))
        p[:, axes[0]], p[:, axes[1]], p[:, axes[2]] = u, v, z
        grids.append(p + rng.uniform(-0.0004, 0.0004, p.shape))
        nn = np.zeros((n * n, 3))
        nn[:, axes[2]] = 1.0
        normals.append(nn)
        tris.append(quad + k * n * n)
    pos = dr._f32(np.concatenate(grids))
    nrm = np.concatenate(normals)
    r2 = np.full(pos.shape[0], (0.7 * s) ** 2)
    tri = np.ascontiguousarray(np.concatenate(tris), np.uint32)
    for arr in (pos, nrm, r2, tri):
        arr.setflags(write=False)
    return pos, nrm, r2, tri


@functools.lru_cache(maxsize=None)
def corner_mesh():
    return Mesh(*corner())


# 2 degrees about the corner's diagonal and 5 mm: the normal displacement of a grid point stays below 10 mm and its slide along
# the grid below 10 mm, so that every sample lies within the 20 mm bound of the mesh before the first iteration
CORNER_TRUE = (np.deg2rad(2.0) * np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0), 0.005 * np.array([0.6, -0.48, 0.64]))


@functools.lru_cache(maxsize=None)
def corner_points():
    """(points, normals, T_true): the vertices of corner() and one area sample of every other triangle, with their grid's normal,
    moved by the INVERSE of T_true: registering them from the identity should find T_true."""
    pos, nrm, r2, tri = corner()
    rng = np.random.default_rng(6)
    T3 = tri[::2].astype(np.int64)
    w = rng.dirichlet(np.ones(3), T3.shape[0])
    area = (w[:, :, None] * pos[T3]).sum(axis=1)
    P = np.concatenate([pos, area])
    Nn = np.concatenate([nrm, nrm[T3[:, 0]]])
    T_true = pose(*CORNER_TRUE).astype(f64)
    inv = tr.se3_inv(T_true)
    pts = (P @ inv[:, :3].T + inv[:, 3]).astype(F)
    nr = (Nn @ inv[:, :3].T).astype(F)
    for arr in (pts, nr):
        arr.setflags(write=False)
    return pts, nr, T_true.astype(F)


@functools.lru_cache(maxsize=None)
def base_set():
    """(points [257, 3], normals [257, 3], T): the set behind most cases, on the world of distance_ref.py.  Under the pose T (0.3
    degrees, 1.5 mm) its moved points reach: BAD inputs (NaN, inf, 65 m), a point the pose moves beyond 64 m, unmatched points,
    the collinear hand triangle as the winner, the long triangle (on the wide list at a cell of 0.0225 m), the triangle given
    twice and once more with the other winding (a tie the earlier wins; the sample normal passes for it and fails for the other
    winding), sample normals on both sides of the gate, and sphere and plane points for the bulk."""
    pos, nrm, r2, tri, info = dr.world()
    rng = np.random.default_rng(23)
    T = pose(np.deg2rad(0.3) * np.array([0.0, 0.6, 0.8]), [0.001, -0.001, 0.0005])
    inv = tr.se3_inv(T.astype(f64))
    back = lambda p: np.asarray(p, f64) @ inv[:, :3].T + inv[:, 3]                 # noqa: E731
    ns = info["n_sphere"]
    used = np.unique(tri[:info["n_sphere_tri"]])
    pick = used[rng.permutation(used.size)[:150]].astype(np.int64)
    sp = pos[pick] * (1.0 + rng.uniform(-0.004, 0.004, (150, 1)))
    sp_n = pos[pick] / np.linalg.norm(pos[pick], axis=1, keepdims=True)
    sp_n[::5] = -sp_n[::5]                                                       # every fifth fails the normal gate
    plane_slots = np.unique(tri[info["n_sphere_tri"]:info["n_sphere_tri"] + info["n_plane_tri"]])
    pp = pos[plane_slots[rng.permutation(plane_slots.size)[:40]].astype(np.int64)] + np.array([0.0, 0.0, 0.003])
    pp_n = np.tile([0.0, 0.0, 1.0], (40, 1))
    H = dr.HAND_AT
    above = H + np.stack([rng.uniform(0.01, 0.05, 12), rng.uniform(0.01, 0.04, 12), np.full(12, 0.004)], axis=1)    # the tie of the windings
    above_n = np.tile([0.0, 0.0, 1.0], (12, 1))
    col = H + np.stack([np.linspace(0.51, 0.59, 8), np.linspace(0.01, 0.09, 8) - 0.004, np.full(8, 0.001)], axis=1)     # beside the collinear one
    col_n = np.tile([0.0, 0.0, 1.0], (8, 1))
    ln = np.array([-0.00632443, -0.9486643, 0.3162215])
    long_ = H + np.array([0.5, 0.53, 0.1]) + np.outer(np.linspace(-0.2, 0.2, 10), [1.0, 0.0, 0.02]) + 0.003 * ln
    long_n = np.tile(ln, (10, 1))
    far = rng.uniform(-1.0, 1.0, (20, 3)) * 0.3 + np.array([0.0, 0.0, 2.0])
    far_n = np.tile([0.0, 0.0, 1.0], (20, 1))
    good = np.concatenate([sp, pp, above, col, long_, far])
    good_n = np.concatenate([sp_n, pp_n, above_n, col_n, long_n, far_n])
    pts = back(good)
    nr = good_n @ inv[:, :3].T
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [65.0, 0, 0], [0, 0, -1e30]])
    # within 64 m before the move and beyond it after, and the other way round (BAD is judged on the moved point)
    edge = np.concatenate([back([[64.0005, 0.1, 0.2], [0.0, -64.0004, 0.1]]), [[-64.0003, 0.0, 0.0]]])
    pts = np.concatenate([pts[:100], bad[:2], edge, pts[100:], bad[2:]])
    nr = np.concatenate([nr[:100], np.tile([0.0, 0.0, 1.0], (5, 1)), nr[100:], np.tile([0.0, 0.0, 1.0], (2, 1))])
    rest = 257 - pts.shape[0]
    assert rest >= 0, pts.shape
    more = pick[:rest]
    pts = np.concatenate([pts, back(pos[more] * 1.002)])
    nr = np.concatenate([nr, (pos[more] / np.linalg.norm(pos[more], axis=1, keepdims=True)) @ inv[:, :3].T])
    pts, nr = np.ascontiguousarray(pts, F), np.ascontiguousarray(nr, F)
    assert pts.shape == (257, 3) and nr.shape == (257, 3)
    for arr in (pts, nr):
        arr.setflags(write=False)
    return pts, nr, T


@functools.lru_cache(maxsize=None)
def shell_set():
    """(points, normals): the decisions that need exact float32 equality, for the identity pose and q = 0.02: points straight
    above corner a of the hand triangle (-3, 0, 0), (-2.9, 0, 0), (-3, 0.1, 0), whose closest point is a itself, at q exactly,
    one float below and one above (d^2 == q^2 exactly for the first); and points above its inside whose normals (s, 0, c) make m
    . N equal cos(max angle) exactly, one float below and one above (N = (0, 0, 1) exactly)."""
    q = F(0.02)
    c = Params().cos_max()
    zs = [q, np.nextafter(q, F(0)), np.nextafter(q, F(1))]
    pts = [[-3.0, 0.0, float(z)] for z in zs]
    nr = [[0.0, 0.0, 1.0]] * 3
    for k, cz in enumerate((c, np.nextafter(c, F(0)), np.nextafter(c, F(2)))):
        pts.append([-2.97 + 0.01 * k, 0.02, 0.005])
        nr.append([float(np.sqrt(1.0 - float(cz) ** 2)), 0.0, float(cz)])
    filler = np.array([[-2.96 + 0.001 * k, 0.03, 0.002] for k in range(60)])
    pts = np.ascontiguousarray(np.concatenate([np.array(pts), filler]), F)
    nr = np.ascontiguousarray(np.concatenate([np.array(nr), np.tile([0.0, 0.0, 1.0], (60, 1))]), F)
    for arr in (pts, nr):
        arr.setflags(write=False)
    return pts, nr


SAMPLE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 2048, 2049, 524289)


def _tiled(a, m):
    return np.ascontiguousarray(np.tile(a, (-(-m // a.shape[0]), 1))[:m]) if m else np.zeros((0, 3), F)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(mesh, points, normals, T_init, params): every case runs against both BUILDS.  One iteration unless the name
    says otherwise; min_inliers 1 so that the small ones solve."""
    pts, nr, T = base_set()
    one = lambda stride=1, q=0.0, **kw: Params(levels=((stride, 1, q),), min_inliers=1, **kw)              # noqa: E731
    out = {}
    for m in SAMPLE_COUNTS:
        out["%d samples" % m] = dict(mesh="world", points=_tiled(pts, m), normals=_tiled(nr, m), T_init=T, params=one())
    # Distinct points, and many of them, at distances from 1e-8 m to 2 cm from the surface: the two thousand float products a
    # workgroup adds are EXACT in double, whatever the order, while they are of one size, so the order of the sums shows only
    # where r^2 spans forty bits.  Around the hand-made triangles alone (brute force stays small): 256 workgroups, nine samples
    # for the first lanes.
    rng = np.random.default_rng(31)
    m = SAMPLE_COUNTS[-1]
    box = dr.HAND_AT + rng.uniform([-0.02, -0.02, 0.0], [0.12, 0.12, 0.0], (m, 3))
    box[:, 2] = np.where(rng.random(m) < 0.5, 0.0, 0.2 + 0.5 * (box[:, 1] - dr.HAND_AT[1]))      # (z = 0, or near the tilted pair's plane)
    box[:, 2] += rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-8.0, -1.7, m)
    inv = tr.se3_inv(T.astype(f64))
    out["%d distinct samples on the hand-made triangles" % m] = dict(
        mesh="hand", points=np.ascontiguousarray(box @ inv[:, :3].T + inv[:, 3], F), normals=np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (m, 1)), F),
        T_init=T, params=one())
    # (2048 of them: one workgroup, so that a last bit of a wavefront's sum is not rounded away by 255 later additions; of the
    # slices of 2048 the one on which the last bit of both the lane tree and the wavefront order shows in the sums)
    big = out["%d distinct samples on the hand-made triangles" % m]
    out["2048 distinct samples on the hand-made triangles"] = dict(big, points=big["points"][7 * 2048:8 * 2048], normals=big["normals"][7 * 2048:8 * 2048])
    out["257 samples, no normals"] = dict(mesh="world", points=pts, normals=None, T_init=T, params=one())
    out["stride 3 of 257"] = dict(mesh="world", points=pts, normals=nr, T_init=T, params=one(3))
    out["stride 2 of 257"] = dict(mesh="world", points=pts, normals=nr, T_init=T, params=one(2))
    out["stride 300 of 257"] = dict(mesh="world", points=pts, normals=nr, T_init=T, params=one(300))
    sp, sn = shell_set()
    out["shell at q and at the angle"] = dict(mesh="world", points=sp, normals=sn, T_init=IDENTITY, params=one(1, 0.02))
    out["three levels on the world"] = dict(mesh="world", points=pts, normals=nr, T_init=T,
                                            params=Params(levels=((4, 2, 0.0), (2, 2, 0.02), (1, 2, 0.01)), min_inliers=10))
    return out


def mesh_of(case):
    return dict(world=world_mesh, hand=hand_mesh, corner=corner_mesh)[case["mesh"]]()


_CALLS = {}


def model_call(name, bound, mutant=None):
    """exact_call of a case against a scene built for `bound`, computed once per process (the restatement's own chain)."""
    key = (name, float(bound), mutant)
    if key not in _CALLS:
        c = cases()[name]
        _CALLS[key] = exact_call(mesh_of(c), c["points"], c["normals"], c["T_init"], c["params"], bound, mutant=mutant)
    return _CALLS[key]
