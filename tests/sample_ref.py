"""The model of smx_recon_sample_mesh and smx_recon_compare_meshes (include/smx.h), shared by the model, host, API and GPU tests.

The model is BRUTE FORCE: one uint64 cumsum over all weights in input order and one searchsorted (side "right") on the inclusive
sums -- no blocks, no two-level prefix, so it cannot share a mistake of the device's search -- and the float32 expressions of
the contract written out as one numpy operation each (one rounding each, no contraction).  The comparison is the chain the
contract defines it by: sample() of one array, then the brute-force distance model of tests/distance_ref.py against the other."""
import numpy as np

import distance_ref as dr

F = np.float32
NONE = 0xFFFFFFFF
SAT = 1 << 62
LIMIT = 1 << 28
U64 = np.uint64
SAMPLE_STAT_NAMES = ("n_in", "n_not_live", "n_repeated", "n_out_of_range", "n_zero_weight", "n_samples", "n_none", "n_triangles_hit",
                     "total_weight", "stride")


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def faces(pos, tri):
    """Step 2 for every row of tri ([m,3] indices in range): (A, ab, ac, N as tuples of three float32 arrays, a)."""
    pos32 = np.asarray(pos).astype(F)
    idx = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3).astype(np.int64)
    A, B, C = (tuple(pos32[idx[:, c], k] for k in range(3)) for c in range(3))
    with np.errstate(all="ignore"):
        ab, ac = tuple(B[k] - A[k] for k in range(3)), tuple(C[k] - A[k] for k in range(3))
        N = _cross(ab, ac)
        a = np.sqrt(_dot(N, N)).astype(F)
    return A, ab, ac, N, a


def weights(pos, r2, tri):
    """Steps 1 and 2: (q [n_in] uint64, dict of the four counts and n_in).  ValueError on an index >= n."""
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    _, t_of, counts = dr.classify(pos, r2, tri)
    q = np.zeros(tri.shape[0], U64)
    if t_of.size:
        a = faces(pos, tri[t_of.astype(np.int64)])[4]
        with np.errstate(all="ignore"):
            q[t_of.astype(np.int64)] = np.where(a > 0, a * F(1073741824.0), F(0)).astype(U64)
    counts["n_zero_weight"] = int(np.sum(q[t_of.astype(np.int64)] == 0))
    return q, counts


def mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def rand(k, j, seed):
    return mix(mix(np.uint32(3) * np.asarray(k, np.uint32) + np.uint32(j)) ^ np.uint32(seed))


def strata(n_samples, S, seed):
    """Step 5 in the split 32-bit formula: u [n_samples] uint64."""
    k = np.arange(n_samples, dtype=np.uint32)
    r0 = rand(k, 0, seed).astype(U64)
    S = int(S)
    return k.astype(U64) * U64(S) + (U64(S >> 32) * r0 + ((U64(S & 0xFFFFFFFF) * r0) >> U64(32)))


def bary(n_samples, seed):
    k = np.arange(n_samples, dtype=np.uint32)
    v = (rand(k, 1, seed) >> np.uint32(8)).astype(F) * F(2.0 ** -24)
    w = (rand(k, 2, seed) >> np.uint32(8)).astype(F) * F(2.0 ** -24)
    flip = (v + w) > F(1.0)
    return np.where(flip, F(1.0) - v, v).astype(F), np.where(flip, F(1.0) - w, w).astype(F)


def sample(pos, r2, tri, n_samples, seed):
    """The whole call: dict of points [n,3], tri [n], bary [n,2], normals [n,3], stats, q.  ValueError on what the call refuses
    (an index out of range, a limit, W == 2^62)."""
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    n_samples, seed = int(n_samples), int(seed)
    if tri.shape[0] > LIMIT or not 0 <= n_samples <= LIMIT:
        raise ValueError("limits")
    q, counts = weights(pos, r2, tri)
    assert tri.shape[0] <= 1 << 18, "the plain uint64 cumsum must not wrap (q < 2^46)"
    incl = np.cumsum(q, dtype=U64)
    W = min(SAT, int(incl[-1])) if incl.size else 0
    if W == SAT:
        raise ValueError("total area too large")
    S = W // n_samples if n_samples else 0
    none = W < n_samples
    stats = dict(counts, n_samples=n_samples, n_none=n_samples if none else 0, total_weight=W, stride=S, n_triangles_hit=0)
    out = dict(points=np.full((n_samples, 3), np.nan, F), tri=np.full(n_samples, NONE, np.uint32), bary=np.full((n_samples, 2), np.nan, F),
               normals=np.full((n_samples, 3), np.nan, F), stats=stats, q=q)
    if none or n_samples == 0:
        return out
    u = strata(n_samples, S, seed)
    t = np.searchsorted(incl, u, side="right")
    assert np.all(t < tri.shape[0]) and np.all(q[t] > 0)
    A, ab, ac, N, a = faces(pos, tri[t])
    v, w = bary(n_samples, seed)
    for k in range(3):
        out["points"][:, k] = (A[k] + v * ab[k]) + w * ac[k]
        out["normals"][:, k] = N[k] / a
    out["tri"][:] = t.astype(np.uint32)
    out["bary"][:, 0], out["bary"][:, 1] = v, w
    stats["n_triangles_hit"] = 1 + int(np.sum(t[1:] != t[:-1]))
    return out


def sums(distance, matched):
    """The three words over the matched samples: (sum_d, sum_sq_lo, sum_sq_hi) as Python integers."""
    dq = (np.asarray(distance, F)[matched] * F(1048576.0)).astype(np.uint32).astype(U64)
    sq = dq * dq
    return int(dq.sum(dtype=U64)), int((sq & U64(0xFFFFFFFF)).sum(dtype=U64)), int((sq >> U64(32)).sum(dtype=U64))


def compare_side(pos, r2, a, b, max_distance, n_samples, seed, cell_size=0.0):
    """Side a -> b: dict(sample=..., distance=..., sum_d, sum_sq_lo, sum_sq_hi) plus the per-sample arrays under "_"."""
    smp = sample(pos, r2, a, n_samples, seed)
    nearest, distance, _, dst = dr.answer(dr.brute(pos, r2, b, smp["points"]), max_distance)
    if cell_size > 0:
        dst.update(dr.structure(pos, r2, b, cell_size, max_distance))
    s = sums(distance, nearest != NONE)
    return dict(sample=smp["stats"], distance=dst, sum_d=s[0], sum_sq_lo=s[1], sum_sq_hi=s[2], _=dict(sample=smp, nearest=nearest, distance=distance))


def point_error_bound(pos, tri_rows):
    """A bound on the distance of a sample from the exact point A + v (B-A) + w (C-A) of its triangle, from the roundings of step 7.
    Per coordinate, with m the largest corner magnitude of the triangle and eps = 2^-24 (half an ulp, relative): ab and ac are
    rounded differences of magnitude <= 2m (eps 2m each, carried through v, w <= 1 unchanged); the two products round values of
    magnitude <= 2m (eps 2m each); A + v ab rounds a value <= 3m (eps 3m) and the last sum one <= 5m (eps 5m): 16 eps m.  The
    test v + w > 1.0f is itself rounded, so v + w may pass 1 by 2^-24, which moves the exact point off the triangle by at most
    eps 2m.  Second-order terms are below eps^2 16 m; 20 eps m per coordinate covers all of it, sqrt(3) times that in space."""
    p = np.abs(np.asarray(pos).astype(F).astype(np.float64))[np.asarray(tri_rows, np.int64)]
    m = p.max(axis=(1, 2))
    return np.sqrt(3.0) * 20.0 * 2.0 ** -24 * m


def big_map():
    """Nine slots: a triangle with corners at +-64 m (q about 2^45) between two triangles with 1 mm edges."""
    pos = np.array([[0.0, 0.0, 0.0], [0.001, 0.0, 0.0], [0.0, 0.001, 0.0],
                    [-64.0, -64.0, -64.0], [64.0, -64.0, 64.0], [-64.0, 64.0, 64.0],
                    [1.0, 1.0, 1.0], [1.001, 1.0, 1.0], [1.0, 1.0, 1.001]])
    return pos, np.full(9, 0.01), np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.uint32)
