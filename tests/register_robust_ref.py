"""The exact model of smx_distscene_register_robust (include/smx.h), shared by the host, API and GPU tests.  Test
infrastructure; numpy, no GPU.  It imports tests/register_ref.py and leaves it as it is: the move, the association by
distance_ref.brute, the plane normal, the gates, the sum order (track_exact.launch_sum) and the solve are that model's.  What
this file adds, each float32 operation one numpy operation:
  * the region of the closest point, by distance_ref._closest on the winner's corners (the computation Q came from);
  * the rim test on the bytes of tests/rim_ref.py: (rim[t] >> region) & 1;
  * the weights: Huber s = sqrt(c / a) beyond c, Tukey s = 1 - (a / c)^2 below c and a rejection from c on;
  * the two counts, sums [31] and [32] (integers: their order does not matter).
The order of decisions per sample: BAD -> not matched -> collinear winner -> rim -> normal gate -> weight -> inlier.

`mutant` turns one decision the other way (MUTANTS); tests/test_register_robust_kernel_host.py shows that each of them changes
the sums of a named case."""
import functools
import math

import numpy as np

import distance_ref as dr
import register_ref as rr
import rim_ref as rf
import track_exact as te
import track_ref as tr

F, f64 = np.float32, np.float64
N_SUMS = 33
S_RIM, S_WEIGHT = 31, 32
NONE, HUBER, TUKEY = 0, 1, 2
WHERE = ("BAD", "not matched", "collinear winner", "on the rim", "normal gate failed", "rejected by Tukey", "inlier, down-weighted", "inlier")
BAD, UNMATCHED, COLLINEAR, RIM, NORMAL_GATE, REJECTED, DOWN, INLIER = range(8)
BUILDS = rr.BUILDS

MUTANTS = {
    "rim_ignores_vertices": "only the edge bits of the rim byte count",
    "rim_after_normal_gate": "the rim test comes after the normal gate (changes [31])",
    "huber_lt": "Huber leaves the row alone for a < c only",
    "tukey_le": "Tukey rejects for !(a <= c) only",
    "weight_squared": "Huber's factor is c / a",
    "rr_weighted": "e = s r: [27] becomes the weighted sum",
}


class Robust:
    """Mirror of smx_register_robust_params."""

    def __init__(self, kernel=NONE, scale=0.0, reject_rim=False):
        s = np.asarray(scale, f64).reshape(-1)
        self.kernel, self.reject_rim = int(kernel), bool(reject_rim)
        self.level_scale = tuple(float(F(v)) for v in (np.tile(s, 3) if s.size == 1 else s))

    def fields(self):
        return dict(kernel=self.kernel, scale=self.level_scale, reject_rim=self.reject_rim)


@functools.lru_cache(maxsize=None)
def _rim_by_id(key):
    mesh = _MESHES[key]
    out = rf.rim(mesh.pos, mesh.r2, mesh.tri)[0]
    out.setflags(write=False)
    return out


_MESHES = {}


def rim_of(mesh):
    """The rim bytes of a register_ref.Mesh, computed once."""
    _MESHES[id(mesh)] = mesh
    return _rim_by_id(id(mesh))


def weights(kernel, c, r, mutant=None):
    """(kept, s, applied, counted) of the residuals r (float32) at scale c (float32 > 0)."""
    a = np.abs(r)
    one = np.ones_like(r)
    with np.errstate(all="ignore"):
        if kernel == HUBER:
            inside = (a < c) if mutant == "huber_lt" else (a <= c)
            s = (c / a) if mutant == "weight_squared" else np.sqrt(c / a)
            return np.ones(r.shape, bool), np.where(inside, one, s).astype(F), ~inside, ~inside
        if kernel == TUKEY:
            out = ~(a <= c) if mutant == "tukey_le" else ~(a < c)
            u = a / c
            s = F(1.0) - u * u
            return ~out, s.astype(F), ~out, out
    return np.ones(r.shape, bool), one, np.zeros(r.shape, bool), np.zeros(r.shape, bool)


def iteration(mesh, pts, nrm, Tf, stride, q, cos_max, robust, c, mutant=None):
    """(sums float64 [33], detail) of one iteration at the pose Tf with gate q and scale c (0 = no weights)."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    m = rr.n_samples(pts.shape[0], stride)
    S = pts[::stride][:m]
    moved = rr.move(Tf, S)
    near = mesh.nearest(moved)
    q2 = F(q) * F(q)
    rim = rim_of(mesh) if robust.reject_rim else None
    with np.errstate(all="ignore"):
        matched = ~near["bad"] & (near["d2"] <= q2)
        where = np.where(near["bad"], BAD, np.where(matched, INLIER, UNMATCHED))
        idx = np.flatnonzero(matched)
        t = near["t"][idx].astype(np.int64)
        A, B, C = (mesh.pos32[mesh.tri[t, k].astype(np.int64)] for k in range(3))
        g = rr._cross(B - A, C - A)
        len2 = rr._dot(g, g)
        area = len2 > 0
        N = g / np.sqrt(len2)[:, None]
        P = moved[idx]
        region = np.full(idx.size, 6, np.uint8)
        on_rim = np.zeros(idx.size, bool)
        if rim is not None and idx.size:
            _, region = dr._closest(tuple(P[:, k] for k in range(3)), *(tuple(X[:, k] for k in range(3)) for X in (A, B, C)))
            byte = rim[t].astype(np.uint32)
            if mutant == "rim_ignores_vertices":
                byte = byte & np.uint32(rf.BIT_AB | rf.BIT_AC | rf.BIT_BC)
            on_rim = ((byte >> region.astype(np.uint32)) & 1) != 0
        gate = np.ones(idx.size, bool)
        if nrm is not None:
            mm = rr.move(Tf, np.ascontiguousarray(nrm, F).reshape(-1, 3)[::stride][:m][idx], rotate_only=True)
            gate = rr._dot(mm, N) >= cos_max
        if mutant == "rim_after_normal_gate":
            state = np.where(~area, COLLINEAR, np.where(~gate, NORMAL_GATE, np.where(on_rim, RIM, INLIER)))
        else:
            state = np.where(~area, COLLINEAR, np.where(on_rim, RIM, np.where(~gate, NORMAL_GATE, INLIER)))
        row = state == INLIER
        Pr, Qr, Nr = P[row], near["Q"][idx][row], N[row]
        r = rr._dot(Nr, Pr - Qr)
        J = np.concatenate([rr._cross(Pr, Nr), Nr], axis=1).astype(F)
        kernel = robust.kernel if F(c) != 0 else NONE
        kept, s, applied, counted = weights(kernel, F(c), r, mutant)
        sub = np.where(~kept, REJECTED, np.where(counted, DOWN, INLIER))
        st = state.copy()
        st[row] = sub
        where[idx] = st
        Jw = np.where(applied[:, None], s[:, None] * J, J).astype(F)
        rw = np.where(applied, s * r, r).astype(F)
        e = rw if mutant == "rr_weighted" else r
        counts = np.zeros((m, 4), np.int64)
        counts[:, 0] = where >= DOWN
        counts[:, 1] = where != BAD
        counts[:, 2] = where >= COLLINEAR
        rows = te._rows(Jw[kept], rw[kept], e[kept])
        sums31 = te.launch_sum(m, idx[row][kept], rows, np.zeros(0, np.int64), np.zeros((0, 28)), counts, False, None)
    sums = np.zeros(N_SUMS, f64)
    sums[:31] = sums31
    sums[S_RIM] = np.sum(where == RIM)
    sums[S_WEIGHT] = np.sum((where == REJECTED) | (where == DOWN))
    full_region = np.full(m, 255, np.uint8)
    full_region[idx] = region
    return sums, dict(where=where, t=near["t"], d2=near["d2"], moved=moved, m=m, region=full_region)


def exact_call(mesh, pts, nrm, T_init, params, robust, bound, recorded=None, mutant=None):
    """register_ref.exact_call with the robust iteration: the same chain, statuses and figures; records hold 33 sums."""
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
            c = robust.level_scale[level] if robust.kernel != NONE else 0.0
            sums, detail = iteration(mesh, pts, nrm, Tf, stride, q if q != 0 else bound, cos_max, robust, c, mutant)
            st, x_ref, _ = tr.solve(sums[:31], T, params)
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
    return dict(records=records, status=status, iterations_run=len(records), T=T, scene_T_points=T.astype(F),
                inliers=int(s[tr.S_INLIERS]), points_used=int(s[tr.S_PIXELS]),
                rms_residual=F(math.sqrt(s[tr.S_RR] / s[tr.S_INLIERS])) if s[tr.S_INLIERS] > 0 else F(0),
                last_update_rotation=F(math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])),
                last_update_translation=F(math.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])))


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
SCALE = 0.002                 # metres: the base set's residuals reach 4 mm, so both sides of every kernel are met
VARIANTS = {"rim": Robust(NONE, 0.0, True), "Huber": Robust(HUBER, SCALE), "Tukey": Robust(TUKEY, SCALE), "rim + Tukey": Robust(TUKEY, SCALE, True)}


@functools.lru_cache(maxsize=None)
def shell_set():
    """Points straight above the inside of the hand-made triangle in the plane z = -0 of distance_ref.world() (N = (0, 0, 1) and
    Q.z = 0 exactly, so r = z exactly under the identity pose) at z = c, one float below and one above, and the same below the
    plane: a == c, a < c and a > c by one float for both kernels."""
    c = F(SCALE)
    zs = [c, np.nextafter(c, F(0)), np.nextafter(c, F(1))]
    pts = [[-2.97 + 0.004 * k, 0.02, sign * float(z)] for sign in (1.0, -1.0) for k, z in enumerate(zs)]
    filler = [[-2.96 + 0.0005 * k, 0.03, 0.0005 + 0.00005 * k] for k in range(58)]
    out = np.ascontiguousarray(np.array(pts + filler), F)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def feature_set():
    """Points whose closest point is a rim vertex, lies on a rim edge, is a vertex or lies on an edge that are not rim, or lies
    inside, on the hand-made triangles of distance_ref.world(): slots 0 1 2 carry the same triangle three times (its edges have
    three triangles and more: not rim) and (1, 2, 5) hangs on its edge 1-2, so slot 1 ends the rim edge 1-5 while slot 0 ends
    none; the pair (14 15 16), (15 17 16) has the rim edge 14-15."""
    H = dr.HAND_AT
    pts = np.array([[0.102, -0.006, 0.003],      # beyond corner B of (0 1 2), a tie with corner A of (1 2 5): region B, slot 1 is a rim vertex
                    [-0.004, -0.004, 0.003],     # beyond corner A of (0 1 2): region A, slot 0 is none
                    [0.05, -0.004, 0.003],       # beside edge AB of (0 1 2): three triangles, not rim
                    [0.05, -0.004, 0.202],       # beside edge AB of (14 15 16): a rim edge
                    [0.03, 0.02, 0.003],         # above the inside of (0 1 2)
                    [0.05, 0.02, 0.215],         # above the inside of (14 15 16)
                    [0.105, -0.005, 0.003]]) + H  # beside edge AC of (1 2 5): the rim edge 1-5
    filler = H + np.array([[0.01 + 0.001 * k, 0.03, 0.002] for k in range(57)])
    out = np.ascontiguousarray(np.concatenate([pts, filler]), F)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(mesh, points, normals, T_init, params, robust): every case runs against both BUILDS, one iteration each unless
    the name says otherwise."""
    pts, nr, T = rr.base_set()
    one = lambda stride=1, q=0.0, **kw: rr.Params(levels=((stride, 1, q),), min_inliers=1, **kw)              # noqa: E731
    out = {}
    for name, rb in VARIANTS.items():
        out["base set, %s" % name] = dict(mesh="world", points=pts, normals=nr, T_init=T, params=one(), robust=rb)
    out["base set, rim, no normals"] = dict(mesh="world", points=pts, normals=None, T_init=T, params=one(), robust=VARIANTS["rim"])
    for name in ("Huber", "Tukey"):
        out["shell at c, %s" % name] = dict(mesh="world", points=shell_set(), normals=None, T_init=rr.IDENTITY, params=one(1, 0.02), robust=VARIANTS[name])
    out["features, rim"] = dict(mesh="world", points=feature_set(), normals=None, T_init=rr.IDENTITY, params=one(1, 0.02), robust=VARIANTS["rim"])
    for m in rr.SAMPLE_COUNTS:
        out["%d samples, rim + Tukey" % m] = dict(mesh="world", points=rr._tiled(pts, m), normals=rr._tiled(nr, m), T_init=T, params=one(),
                                                  robust=VARIANTS["rim + Tukey"])
    out["three levels, rim + Huber, a scale per level"] = dict(
        mesh="world", points=pts, normals=nr, T_init=T, params=rr.Params(levels=((4, 2, 0.0), (2, 2, 0.02), (1, 2, 0.01)), min_inliers=10),
        robust=Robust(HUBER, (0.004, 0.0, 0.001), True))
    return out


_CALLS = {}


def model_call(name, bound, mutant=None):
    """exact_call of a case against a scene built for `bound`, computed once per process (the restatement's own chain)."""
    key = (name, float(bound), mutant)
    if key not in _CALLS:
        c = cases()[name]
        _CALLS[key] = exact_call(rr.mesh_of(c), c["points"], c["normals"], c["T_init"], c["params"], c["robust"], bound, mutant=mutant)
    return _CALLS[key]


# ---- the behaviour fixture: a patch cut out of a larger surface ------------------------------------------------------------------
PATCH_TRUE = (np.deg2rad(1.0) * np.array([0.5, -0.6, 0.62]) / np.linalg.norm([0.5, -0.6, 0.62]), 0.001 * np.array([3.0, -2.0, 2.5]))


@functools.lru_cache(maxsize=None)
def patch():
    """dict(mesh, whole, inner, T_true): a 37 x 37 vertex grid at 0.02 m from -0.12 m with z = 0.03 sin 9x cos 7y + 0.02 sin(5x + 4y +
    1) + 0.5 (x - 0.3)^2 and an in-plane jitter of up to 3 mm; the scene's mesh is the triangles with all corners in [0, 0.48]^2
    (a patch cut out of the surface, about 1 080 triangles); `whole` = 3 000 area samples of ALL the grid's triangles and `inner`
    = 3 000 area samples of the patch's triangles, of which every point with u < 0.15 is lifted off the surface by 4 to 15 mm
    (one-sided outliers).  Both point sets are moved by the INVERSE of T_true (1 degree about (0.5, -0.6, 0.62) and (3, -2, 2.5)
    mm): registering them from the identity should find T_true.  Read-only."""
    rng = np.random.default_rng(41)
    n, s = 37, 0.02
    gx, gy = np.meshgrid(np.arange(n) * s - 0.12, np.arange(n) * s - 0.12, indexing="ij")
    x = gx.reshape(-1) + rng.uniform(-0.003, 0.003, n * n)
    y = gy.reshape(-1) + rng.uniform(-0.003, 0.003, n * n)
    z = 0.03 * np.sin(9 * x) * np.cos(7 * y) + 0.02 * np.sin(5 * x + 4 * y + 1) + 0.5 * (x - 0.3) ** 2
    pos = dr._f32(np.stack([x, y, z], axis=1))
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = (i * n + j).reshape(-1), ((i + 1) * n + j).reshape(-1), ((i + 1) * n + j + 1).reshape(-1), (i * n + j + 1).reshape(-1)
    tri = np.ascontiguousarray(np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]), np.uint32)
    inside = (pos[:, 0] >= 0) & (pos[:, 0] <= 0.48) & (pos[:, 1] >= 0) & (pos[:, 1] <= 0.48)
    cut = np.ascontiguousarray(tri[np.all(inside[tri.astype(np.int64)], axis=1)])
    nrm = np.tile([0.0, 0.0, 1.0], (n * n, 1))
    r2 = np.full(n * n, (0.7 * s) ** 2)

    def area_samples(t, count):
        P = pos[t.astype(np.int64)]
        area = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
        pick = rng.choice(t.shape[0], count, p=area / area.sum())
        w = rng.dirichlet(np.ones(3), count)
        return (w[:, :, None] * P[pick]).sum(axis=1)
    whole = area_samples(tri, 3000)
    inner = area_samples(cut, 3000)
    lifted = rng.random(3000) < 0.15
    inner[lifted, 2] += rng.uniform(0.004, 0.015, int(lifted.sum()))
    T_true = rr.pose(*PATCH_TRUE).astype(f64)
    inv = tr.se3_inv(T_true)
    back = lambda p: np.ascontiguousarray((p @ inv[:, :3].T + inv[:, 3]).astype(F))                 # noqa: E731
    out = dict(mesh=rr.Mesh(pos, nrm, r2, cut), whole=back(whole), inner=back(inner), T_true=T_true, n_lifted=int(lifted.sum()))
    for v in (pos, cut, out["whole"], out["inner"]):
        v.setflags(write=False)
    return out


PATCH_VARIANTS = {
    "plain": ("whole", Robust()), "rim rejected": ("whole", Robust(NONE, 0.0, True)),
    "outliers, plain": ("inner", Robust()), "outliers, Huber 2 mm": ("inner", Robust(HUBER, 0.002)), "outliers, Tukey 4 mm": ("inner", Robust(TUKEY, 0.004)),
    "rim + Tukey 16 / 8 / 4 mm": ("whole", Robust(TUKEY, (0.016, 0.008, 0.004), True)),
}


def patch_call(variant, bound):
    """The model's own chain (default schedule, no normals) of a variant on the patch: (call, translation error in metres, rotation
    error in radians against T_true).  Computed once per process."""
    key = ("patch", variant, float(bound))
    if key not in _CALLS:
        f = patch()
        which, robust = PATCH_VARIANTS[variant]
        call = exact_call(f["mesh"], f[which], None, rr.IDENTITY, rr.Params(), robust, bound)
        dt, drot = tr.pose_difference(call["T"], f["T_true"])
        _CALLS[key] = (call, dt, drot)
    return _CALLS[key]
