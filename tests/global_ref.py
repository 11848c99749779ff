"""The exact model of smx_register_pose_lattice, smx_distscene_score_poses and smx_distscene_register_global (include/smx.h,
DESIGN.md 5s), shared by the CPU, host and GPU tests.  Test infrastructure; numpy, no GPU.

What it is made of, none of it the code under test:
  * the lattice in numpy float64, + - * / only, each value rounded once to float32;
  * the score from register_ref.move (the registration's float32 move), distance_ref.brute (every moved sample against every
    triangle of R, no grid) with the gate applied afterwards, rim_ref's bytes with distance_ref._closest's region, and the 2^-20 m
    word of sample_ref.sums;
  * the selection as a plain sort of (cost, index), the whole call chained from register_ref.exact_call /
    register_robust_ref.exact_call.

`mutant` turns one decision the other way (MUTANTS); tests/test_global_model.py shows that each changes a word of a named case.
The fixture is bracket(): three perpendicular rectangles of three different sizes, which no rotation maps onto themselves (the
corner() of register_ref.py has a three-fold axis)."""
import functools

import numpy as np

import distance_ref as dr
import register_ref as rr
import register_robust_ref as rb
import track_ref as tr

F, f64 = np.float32, np.float64
INVALID = dr.INVALID
SCORE_DTYPE = np.dtype([("cost", "<u8"), ("n_ok", "<u4"), ("n_matched", "<u4"), ("n_rim", "<u4"), ("reserved", "<u4")])
UNIT = F(1048576.0)

MUTANTS = {
    "unmatched_free": "a sample that is not matched pays nothing",
    "bad_free": "a BAD sample pays nothing",
    "anchor_major": "pose index = anchor index * N + rotation index",
    "stride_plus_one": "sample j is point j * (stride + 1)",
    "tie_later": "of two poses of one cost the LATER index comes first",
    "winner_before": "the winner is the start with the smallest cost_before",
}


# ---- the lattice -------------------------------------------------------------------------------------------------------------
def n_rotations(k):
    return ((2 * k + 1) ** 4 - (2 * k - 1) ** 4) // 2


@functools.lru_cache(maxsize=None)
def quaternions(k):
    """[N_k, 4] int64 (w, x, y, z): the largest absolute component is k, the first non-zero one is positive; ascending."""
    r = np.arange(-k, k + 1)
    q = np.stack(np.meshgrid(r, r, r, r, indexing="ij"), axis=-1).reshape(-1, 4)        # (ascending lexicographic as built)
    first = np.zeros(q.shape[0], np.int64)
    for c in (3, 2, 1, 0):
        first = np.where(q[:, c] != 0, q[:, c], first)
    out = q[(np.abs(q).max(axis=1) == k) & (first > 0)].astype(np.int64)
    out.setflags(write=False)
    return out


def rotations(k):
    """[N_k, 3, 3] float64: every entry one exact integer numerator divided once by n."""
    q = quaternions(k)
    w, x, y, z = (q[:, c] for c in range(4))
    n = (w * w + x * x + y * y + z * z).astype(f64)
    num = np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                    2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                    2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], axis=1)
    return (num.astype(f64) / n[:, None]).reshape(-1, 3, 3)


def lattice(k, centre, anchors, mutant=None):
    """[N_k * A, 3, 4] float32: t_i = a_i - ((R_i0 c_0 + R_i1 c_1) + R_i2 c_2); pose index = rotation index * A + anchor index."""
    R = rotations(k)
    c = np.asarray(centre, f64).reshape(3)
    a = np.asarray(anchors, f64).reshape(-1, 3)
    Rc = (R[:, :, 0] * c[0] + R[:, :, 1] * c[1]) + R[:, :, 2] * c[2]                    # [N, 3]
    t = a[None, :, :] - Rc[:, None, :]                                                   # [N, A, 3]
    poses = np.concatenate([np.broadcast_to(R[:, None, :, :], (R.shape[0], a.shape[0], 3, 3)), t[:, :, :, None]], axis=3)
    if mutant == "anchor_major":
        poses = poses.transpose(1, 0, 2, 3)
    return np.ascontiguousarray(poses.reshape(-1, 3, 4).astype(F))


# ---- the score ---------------------------------------------------------------------------------------------------------------
def q_word(q):
    return int((F(q) * UNIT).astype(np.uint32))


_NEAR = {}


def association(mesh, moved, q, with_rim=False):
    """What the query answers for every moved sample at gate q, and what the rim decision reads: dict of ok (not BAD), matched, t
    (INVALID where not matched), distance (float32, +inf where not matched), and with_rim byte (the winner's rim byte, 0 where not
    matched) and A, B, C (the winner's corners, NaN where not matched)."""
    moved = np.ascontiguousarray(moved, F).reshape(-1, 3)
    key = (id(mesh), moved.tobytes())
    if key not in _NEAR:                                   # (the winner over all of R does not depend on the gate: one search for every q)
        n_r = max(1, dr.classify(mesh.pos, mesh.r2, mesh.tri)[0].shape[0])
        step = max(1, dr.MAX_PAIRS // n_r)
        parts = [dr.brute(mesh.pos, mesh.r2, mesh.tri, moved[lo:lo + step]) for lo in range(0, moved.shape[0], step)]
        if len(_NEAR) >= 6:
            _NEAR.pop(next(iter(_NEAR)))
        _NEAR[key] = {k: np.concatenate([p[k] for p in parts]) for k in ("d2", "t", "bad")}
    near = _NEAR[key]
    q = F(q)
    with np.errstate(all="ignore"):
        ok = ~near["bad"]
        matched = ok & (near["d2"] <= q * q)
        out = dict(ok=ok, matched=matched, t=np.where(matched, near["t"], INVALID).astype(np.uint32),
                   distance=np.where(matched, np.sqrt(np.where(matched, near["d2"], F(0))), F(np.inf)).astype(F))
    if with_rim:
        n = moved.shape[0]
        out.update(byte=np.zeros(n, np.uint32), A=np.full((n, 3), np.nan, F), B=np.full((n, 3), np.nan, F), C=np.full((n, 3), np.nan, F))
        idx = np.flatnonzero(matched)
        t = out["t"][idx].astype(np.int64)
        for c, name in enumerate("ABC"):
            out[name][idx] = mesh.pos32[mesh.tri[t, c].astype(np.int64)]
        out["byte"][idx] = rb.rim_of(mesh)[t]
    return out


def sample_words(mesh, moved, q, reject_rim):
    """Per moved sample: (ok, matched, on_rim, word) with word = the distance word of a matched sample."""
    moved = np.ascontiguousarray(moved, F).reshape(-1, 3)
    a = association(mesh, moved, q, reject_rim)
    ok, matched = a["ok"], a["matched"]
    with np.errstate(all="ignore"):
        word = (np.where(matched, a["distance"], F(0)) * UNIT).astype(np.uint32).astype(np.uint64)
        on_rim = np.zeros(moved.shape[0], bool)
        if reject_rim:
            idx = np.flatnonzero(matched)
            A, B, C, P = a["A"][idx], a["B"][idx], a["C"][idx], moved[idx]
            g = rr._cross(B - A, C - A)
            area = rr._dot(g, g) > 0                       # (the registration's order: a winner without an area is never on the rim)
            _, region = dr._closest(tuple(P[:, c] for c in range(3)), *(tuple(X[:, c] for c in range(3)) for X in (A, B, C)))
            on_rim[idx] = area & (((a["byte"][idx] >> region.astype(np.uint32)) & 1) != 0)
    return ok, matched, on_rim, word


def score(mesh, pts, poses, stride=1, q=0.05, reject_rim=False, mutant=None):
    """SCORE_DTYPE [P]: every word of smx_pose_score for every pose."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    poses = np.ascontiguousarray(poses, F).reshape(-1, 3, 4)
    m = rr.n_samples(pts.shape[0], stride)
    S = pts[::stride + 1][:m] if mutant == "stride_plus_one" else pts[::stride][:m]
    m = S.shape[0]
    out = np.zeros(poses.shape[0], SCORE_DTYPE)
    if m == 0:
        return out
    moved = np.concatenate([rr.move(T, S) for T in poses])
    ok, matched, on_rim, word = sample_words(mesh, moved, q, reject_rim)
    qw = np.uint64(q_word(q))
    pays = np.where(matched & ~on_rim, word, qw)
    if mutant == "unmatched_free":
        pays = np.where(ok & ~matched, np.uint64(0), pays)
    if mutant == "bad_free":
        pays = np.where(~ok, np.uint64(0), pays)
    shape = (poses.shape[0], m)
    out["cost"] = pays.reshape(shape).sum(axis=1, dtype=np.uint64)
    out["n_ok"] = ok.reshape(shape).sum(axis=1)
    out["n_matched"] = matched.reshape(shape).sum(axis=1)
    out["n_rim"] = (matched & on_rim).reshape(shape).sum(axis=1)
    return out


# ---- the choice and the whole call -------------------------------------------------------------------------------------------
def select(cost, n_starts, mutant=None):
    """The first min(n_starts, P) pose indices by (cost, index) ascending."""
    cost = np.asarray(cost, np.uint64)
    index = np.arange(cost.size)
    order = np.lexsort((-index if mutant == "tie_later" else index, cost))
    return order[:min(int(n_starts), cost.size)].astype(np.int64)


def found(status, n_matched, n_ok, min_matched_fraction):
    return status in (tr.OK, tr.CONVERGED) and F(n_matched) >= F(min_matched_fraction) * F(n_ok)


def register_global(mesh, pts, nrm, poses, params, bound, robust=None, stride=1, q=0.0, reject_rim=False, n_starts=8,
                    min_matched_fraction=0.5, scores=None, mutant=None):
    """The whole call on the model's own chain: dict(scores, order, calls (exact_call of every start), after (SCORE_DTYPE [M]),
    winner_rank, found, T (the winner's float32 pose)).  scores: the P scores if the caller has them."""
    poses = np.ascontiguousarray(poses, F).reshape(-1, 3, 4)
    gate = q if q != 0 else bound
    if scores is None:
        scores = score(mesh, pts, poses, stride, gate, reject_rim, mutant)
    order = select(scores["cost"], n_starts, mutant)
    asks = robust is not None and (robust.kernel != rb.NONE or robust.reject_rim)
    calls = [rb.exact_call(mesh, pts, nrm, poses[i], params, robust, bound) if asks else rr.exact_call(mesh, pts, nrm, poses[i], params, bound)
             for i in order]
    after = score(mesh, pts, np.stack([c["scene_T_points"] for c in calls]), stride, gate, reject_rim, mutant)
    key = scores["cost"][order] if mutant == "winner_before" else after["cost"]
    win = int(np.lexsort((np.arange(order.size), key))[0])
    return dict(scores=scores, order=order, calls=calls, after=after, winner_rank=win,
                found=bool(found(calls[win]["status"], int(after["n_matched"][win]), int(after["n_ok"][win]), min_matched_fraction)),
                T=calls[win]["scene_T_points"])


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
BRACKET_SPACING, BRACKET_BOUND, BRACKET_CELL = 0.04, 0.05, 0.05625
BRACKET_PANELS = ((13, 7), (7, 5), (5, 13))            # vertices along u and v: 0.48 x 0.24, 0.24 x 0.16 and 0.16 x 0.48 m
BRACKET_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def bracket():
    """(pos, nrm, r2, tri): an open bracket of three mutually perpendicular rectangles meeting at the origin -- 0.48 x 0.24 m in z =
    0, 0.24 x 0.16 m in x = 0, 0.16 x 0.48 m in y = 0, so that the three extents 0.48, 0.24 and 0.16 m differ and no rotation maps
    the surface onto itself -- as vertex grids at 0.04 m, each vertex jittered by up to 0.4 mm, two triangles per square wound
    counter-clockwise about the panel's normal.  191 slots, 288 triangles.  Read-only."""
    rng = np.random.default_rng(41)
    s = BRACKET_SPACING
    grids, normals, tris, base = [], [], [], 0
    for (nu, nv), axes in zip(BRACKET_PANELS, ((0, 1, 2), (1, 2, 0), (2, 0, 1))):       # (u axis, v axis, normal axis)
        u, v = np.meshgrid(np.arange(nu) * s, np.arange(nv) * s, indexing="ij")
        p = np.zeros((nu * nv, 3))
        p[:, axes[0]], p[:, axes[1]] = u.reshape(-1), v.reshape(-1)
        grids.append(p + rng.uniform(-0.0004, 0.0004, p.shape))
        nn = np.zeros((nu * nv, 3))
        nn[:, axes[2]] = 1.0
        normals.append(nn)
        i, j = np.meshgrid(np.arange(nu - 1), np.arange(nv - 1), indexing="ij")
        a, b, c, d = (i * nv + j).reshape(-1), ((i + 1) * nv + j).reshape(-1), ((i + 1) * nv + j + 1).reshape(-1), (i * nv + j + 1).reshape(-1)
        tris.append(np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]) + base)
        base += nu * nv
    pos = dr._f32(np.concatenate(grids))
    nrm = np.concatenate(normals)
    r2 = np.full(pos.shape[0], (0.7 * s) ** 2)
    tri = np.ascontiguousarray(np.concatenate(tris), np.uint32)
    assert pos.shape[0] == 191 and tri.shape[0] == 288
    for arr in (pos, nrm, r2, tri):
        arr.setflags(write=False)
    return pos, nrm, r2, tri


@functools.lru_cache(maxsize=None)
def bracket_mesh():
    return rr.Mesh(*bracket())


@functools.lru_cache(maxsize=None)
def bracket_anchor():
    """[1, 3] float64: the centroid of the bracket's surface, the one anchor of the end-to-end cases."""
    pos, _, _, tri = bracket()
    P = np.asarray(pos, f64)[tri.astype(np.int64)]
    area = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    return ((P.mean(axis=1) * area[:, None]).sum(axis=0) / area.sum()).reshape(1, 3)


def random_rotation(rng):
    """A uniformly distributed rotation from a normalised Gaussian quaternion."""
    w, x, y, z = (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def bracket_points(seed):
    """(points [256, 3], normals [256, 3], T_true [3, 4] float64, scene <- points): 256 area samples of bracket() with their panel's
    normal, moved by the INVERSE of a seeded uniformly random rotation and a translation of up to 1 m per axis: registering them
    should find T_true.  Of BRACKET_SEEDS, seeds 2 and 3 turn by more than 90 degrees."""
    pos, nrm, r2, tri = bracket()
    rng = np.random.default_rng(1000 + seed)
    P3 = np.asarray(pos, f64)[tri.astype(np.int64)]
    area = 0.5 * np.linalg.norm(np.cross(P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0]), axis=1)
    t = rng.choice(tri.shape[0], 256, p=area / area.sum())
    w = rng.dirichlet(np.ones(3), 256)
    S = (w[:, :, None] * P3[t]).sum(axis=1)
    N = np.asarray(nrm, f64)[tri[t, 0].astype(np.int64)]
    T_true = np.concatenate([random_rotation(rng), rng.uniform(-1.0, 1.0, (3, 1))], axis=1)
    inv = tr.se3_inv(T_true)
    pts = np.ascontiguousarray((S @ inv[:, :3].T + inv[:, 3]).astype(F))
    nr = np.ascontiguousarray((N @ inv[:, :3].T).astype(F))
    for arr in (pts, nr, T_true):
        arr.setflags(write=False)
    return pts, nr, T_true


def centre_of(pts):
    """The float64 mean of the finite points: meshing.register_global's default centre."""
    p = np.asarray(pts, f64).reshape(-1, 3)
    return p[np.all(np.isfinite(p), axis=1)].mean(axis=0)


def bracket_poses(seed, k):
    """The lattice of order k about the points' mean, on the bracket's centroid."""
    return lattice(k, centre_of(bracket_points(seed)[0]), bracket_anchor())


def rotation_angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, f64)[:, :3].T @ np.asarray(Rb, f64)[:, :3]) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def nearest_lattice_angle_deg(k, R):
    """The angle from R to the nearest rotation of the lattice, and that rotation's index."""
    L = rotations(k)
    c = (np.einsum("nij,ij->n", L, np.asarray(R, f64)[:, :3]) - 1.0) / 2.0
    i = int(np.argmax(c))
    return float(np.degrees(np.arccos(np.clip(c[i], -1.0, 1.0)))), i


GOLDEN = "global_bracket.npz"       # tests/golden: the model's 888 scores of every seed (tests/golden/make_global_bracket.py)


@functools.lru_cache(maxsize=None)
def golden_scores(seed):
    """SCORE_DTYPE [888]: the recorded scores of bracket_poses(seed, 3) at stride 1 and gate 0.05 m."""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as g:
        out = np.zeros(g["cost_%d" % seed].size, SCORE_DTYPE)
        for name in ("cost", "n_ok", "n_matched", "n_rim"):
            out[name] = g["%s_%d" % (name, seed)]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def world_poses():
    """[40, 3, 4] float32: the k = 1 lattice about the base set's pose -- T L_i with L_i the lattice's rotations about the median of
    the set's finite points, composed in float64 and rounded once.  L of the identity is the identity exactly, so that pose is
    register_ref.base_set()'s own and reaches every decision that set was made for."""
    pts, _, T = rr.base_set()
    p = np.asarray(pts, f64)
    c = np.median(p[np.all(np.isfinite(p), axis=1)], axis=0)
    L = lattice(1, c, c.reshape(1, 3)).astype(f64)
    out = np.stack([tr.se3_mul(T.astype(f64), Li) for Li in L]).astype(F)
    assert out[quaternions(1).tolist().index([1, 0, 0, 0])].tobytes() == np.asarray(T, F).tobytes()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(mesh ("world" / "bracket"), points, poses, stride, rim): the score cases; the world's run against both
    register_ref.BUILDS with q = the build's bound, the bracket's against (BRACKET_BOUND, BRACKET_CELL)."""
    pts = rr.base_set()[0]
    out = {}
    for stride in (1, 3):
        out["base set, k = 1 about its pose, stride %d" % stride] = dict(mesh="world", points=pts, poses=world_poses(), stride=stride, rim=False)
    bp = bracket_points(2)[0]
    for rim in (False, True):
        out["bracket, k = 2, stride 4%s" % (", rim rejected" if rim else "")] = dict(mesh="bracket", points=bp, poses=bracket_poses(2, 2), stride=4, rim=rim)
    out["bracket, one pose"] = dict(mesh="bracket", points=bp, poses=bracket_poses(2, 2)[100:101], stride=4, rim=False)
    return out


def mesh_of(case):
    return dict(world=rr.world_mesh, bracket=bracket_mesh)[case["mesh"]]()


def gates_of(name):
    """The gates a case runs at: the bound of every build of its scene."""
    return tuple(b for b, _ in rr.BUILDS) if cases()[name]["mesh"] == "world" else (BRACKET_BOUND,)


def golden_case(name, q):
    """SCORE_DTYPE [P]: the recorded model_scores(name, q)."""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as g:
        out = np.zeros(g["cost|%s|%g" % (name, q)].size, SCORE_DTYPE)
        for word in ("cost", "n_ok", "n_matched", "n_rim"):
            out[word] = g["%s|%s|%g" % (word, name, q)]
    return out


_SCORES = {}


def model_scores(name, q, mutant=None):
    """score() of a case at gate q, computed once per process."""
    key = (name, float(q), mutant)
    if key not in _SCORES:
        c = cases()[name]
        _SCORES[key] = score(mesh_of(c), c["points"], c["poses"], c["stride"], q, c["rim"], mutant)
    return _SCORES[key]
