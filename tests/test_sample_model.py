"""The model of smx_recon_sample_mesh (tests/sample_ref.py) against what the contract promises, on the world of
tests/distance_ref.py (9 574 triangles; W = 28 834 702 933 units of 2^-30 m^2, about 2^34.75).  No GPU: these tests say that the
definition the device is held to for equality is itself area-weighted, stratified, on the triangles and uniform inside them."""
import numpy as np
import pytest

import decimate_ref as dec
import distance_ref as dr
import sample_ref as sr

COUNTS = (1, 63, 64, 65, 255, 256, 257, 4097, 100000)


@pytest.fixture(scope="module")
def world():
    pos, nrm, r2, tri, info = dr.world()
    q, counts = sr.weights(pos, r2, tri)
    return dict(pos=pos, r2=r2, tri=tri, q=q, counts=counts, W=int(q.sum(dtype=np.uint64)))


def test_no_sample_is_none_at_any_count_the_tests_use(world):
    for n in COUNTS:
        for seed in (0, 0xFFFFFFFF):
            s = sr.sample(world["pos"], world["r2"], world["tri"], n, seed)
            assert s["stats"]["n_none"] == 0 and np.all(s["tri"] != sr.NONE) and np.all(np.isfinite(s["points"])), (n, seed)
            assert s["stats"]["total_weight"] == world["W"] and s["stats"]["stride"] == world["W"] // n
    assert sr.sample(world["pos"], world["r2"], world["tri"], 0, 0)["stats"]["n_none"] == 0


def test_the_split_formula_is_the_integer_stratum(world):
    # the world's S, then strides with S >> 32 != 0 up to the largest a call can meet
    for S in (world["W"] // 4097, world["W"], (1 << 45) + 12345, (1 << 62) - 1):
        for seed in (0, 1, 0xFFFFFFFF):
            n = 2000
            u = sr.strata(n, S, seed)
            r0 = sr.rand(np.arange(n, dtype=np.uint32), 0, seed)
            want = [k * S + ((S * int(r0[k])) >> 32) for k in range(n)]
            if (n - 1) * S + S < 1 << 64:
                assert [int(v) for v in u] == want, (S, seed)
            else:                        # (k S itself passes 2^64 only for strides no call can have with this many samples)
                assert [int(v) for v in u[:4]] == want[:4], (S, seed)
            assert all(k * S <= want[k] < (k + 1) * S for k in range(n))


def test_the_random_words_are_the_contracts():
    def mix(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    k = np.array([0, 1, 2, 12345, (1 << 28) - 1, 0x55555555, 0xFFFFFFFF], np.uint32)
    for seed in (0, 1, 12345, 0xFFFFFFFF):
        for j in range(3):
            assert [int(v) for v in sr.rand(k, j, seed)] == [mix(mix((3 * int(x) + j) & 0xFFFFFFFF) ^ seed) for x in k]


def test_counts_per_triangle_follow_the_area(world):
    """Triangle t covers the units [C_t, C_t + q_t); a stratum of S units holds exactly one sample, so t receives between
    floor(q_t / S) - 1 and ceil(q_t / S) + 1 of them: |count_t - q_t / S| < 2."""
    q = world["q"].astype(np.float64)
    worst = {}
    for n in COUNTS:
        s = sr.sample(world["pos"], world["r2"], world["tri"], n, 0)
        count = np.bincount(s["tri"], minlength=q.size).astype(np.float64)
        S = s["stats"]["stride"]
        worst[n] = (float(np.abs(count - q / S).max()), float(np.abs(count - q * n / world["W"]).max()))
        assert worst[n][0] < 2.0, (n, worst[n])
        assert np.all(np.diff(s["tri"].astype(np.int64)) >= 0)                     # the output is in input-triangle order
        assert s["stats"]["n_triangles_hit"] == np.unique(s["tri"]).size
    print("largest |count - q/S| and |count - q n/W| by n_samples:", worst)


def test_every_point_lies_on_its_triangle(world):
    pos, tri = world["pos"], world["tri"]
    p64 = np.asarray(pos).astype(np.float32).astype(np.float64)
    largest = 0.0
    for n, seed in ((4097, 0), (100000, 0xFFFFFFFF)):
        s = sr.sample(pos, world["r2"], tri, n, seed)
        rows = tri[s["tri"].astype(np.int64)].astype(np.int64)
        A, B, C = p64[rows[:, 0]], p64[rows[:, 1]], p64[rows[:, 2]]
        v, w = s["bary"][:, 0].astype(np.float64), s["bary"][:, 1].astype(np.float64)
        assert np.all(v >= 0) and np.all(w >= 0) and np.all(v + w <= 1.0 + 2.0 ** -24)
        exact = A + v[:, None] * (B - A) + w[:, None] * (C - A)
        err = np.linalg.norm(s["points"].astype(np.float64) - exact, axis=1)
        bound = sr.point_error_bound(pos, rows)
        largest = max(largest, float((err / bound).max()))
        assert np.all(err <= bound)
        # the normal is the unit normal of the triangle
        nrm = np.cross(B - A, C - A)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        assert np.abs(s["normals"].astype(np.float64) - nrm).max() < 1e-4
    print("largest distance from the exact point, as a fraction of the bound: %.3f" % largest)


def test_another_seed_moves_the_points_and_keeps_the_counts(world):
    a = sr.sample(world["pos"], world["r2"], world["tri"], 4097, 0)
    b = sr.sample(world["pos"], world["r2"], world["tri"], 4097, 1)
    assert a["points"].tobytes() != b["points"].tobytes() and a["bary"].tobytes() != b["bary"].tobytes()
    ca, cb = (np.bincount(x["tri"], minlength=world["q"].size).astype(np.int64) for x in (a, b))
    # both are within 2 of q_t / S, and they are integers
    assert np.abs(ca - cb).max() <= 3


@pytest.mark.parametrize("n", (4096, 65536))
@pytest.mark.parametrize("seed", (0, 1, 12345, 0xFFFFFFFF))
def test_points_are_uniform_inside_one_triangle(n, seed):
    """One triangle: the counts in its four midpoint sub-triangles stay within 4 sigma of a quarter, sigma = sqrt(n 3/16)."""
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    s = sr.sample(pos, np.full(3, 0.01), np.array([[0, 1, 2]], np.uint32), n, seed)
    v, w = s["bary"][:, 0].astype(np.float64), s["bary"][:, 1].astype(np.float64)
    at_b, at_c, at_a = v > 0.5, w > 0.5, v + w < 0.5
    middle = ~(at_a | at_b | at_c)
    counts = np.array([at_a.sum(), at_b.sum(), at_c.sum(), middle.sum()])
    sigma = np.sqrt(n * 3.0 / 16.0)
    dev = np.abs(counts - n / 4.0) / sigma
    print("n %d seed %d: %s, largest deviation %.2f sigma" % (n, seed, counts.tolist(), dev.max()))
    assert counts.sum() == n and dev.max() < 4.0


def test_dropped_and_zero_area_triangles_get_no_sample(world):
    tri, q = world["tri"], world["q"]
    _, t_of, counts = dr.classify(world["pos"], world["r2"], tri)
    dropped = np.setdiff1d(np.arange(tri.shape[0]), t_of)
    assert dropped.size == 9 and counts["n_not_live"] == 7 and world["counts"]["n_zero_weight"] == 2
    assert np.all(q[dropped] == 0) and int(np.sum(q == 0)) == 11
    s = sr.sample(world["pos"], world["r2"], tri, 100000, 0)
    assert not np.any(np.isin(s["tri"], np.flatnonzero(q == 0)))


def test_vertices_cannot_measure_coarse_to_fine_and_samples_can(world):
    """The motivating case: decimation collapses every cell onto an existing surfel, so every vertex of the coarse mesh is a
    vertex of the fine one and lies at distance exactly 0 from it; points on the coarse faces do not."""
    pos, r2, fine = world["pos"], world["r2"], world["tri"]
    coarse = dec.decimate(pos, r2, fine, 0.1)[0]
    R = dr.classify(pos, r2, coarse)[0]
    used = np.unique(R)
    verts = np.asarray(pos).astype(np.float32)[used.astype(np.int64)]
    vd = dr.answer(dr.brute(pos, r2, fine, verts), 0.5)
    assert vd[3]["n_matched"] == used.size and vd[3]["max_dist2_bits"] == 0 and np.all(vd[1] == 0)
    side = sr.compare_side(pos, r2, coarse, fine, 0.5, 1500, 0)
    assert side["distance"]["max_dist2_bits"] > 0 and side["sum_d"] > 0 and side["distance"]["n_matched"] == 1500
