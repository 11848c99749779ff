"""smx_recon_sample_mesh on the device.  The contract (include/smx.h) is made of integers and of float32 expressions that numpy
reproduces bit for bit, so everything here is compared for EQUALITY with the brute-force model of tests/sample_ref.py: points,
tri, bary, normals and every statistic."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dr
import mesh_ref as mr
import sample_ref as sr
import trigrid_cases as tc

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
ARRAYS = ("points", "tri", "bary", "normals")
PER = dict(points=3, tri=1, bary=2, normals=3)


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


def _up(pos):
    return np.tile(np.array([0.0, 0.0, 1.0]), (pos.shape[0], 1))


@pytest.fixture(scope="module")
def world(smx):
    pos, nrm, r2, tri, info = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    yield dict(m=(pos, nrm, r2), rec=rec, tri=tri)
    rec.close()


@pytest.fixture(scope="module")
def big(smx):
    pos, r2, tri = sr.big_map()
    rec = _rec_of(smx, (pos, _up(pos), r2), spare=100)
    yield dict(m=(pos, _up(pos), r2), rec=rec, tri=tri)
    rec.close()


def _check(rec, m, tri, n, seed, what):
    want = sr.sample(m[0], m[2], tri, n, seed)
    points, t, bary, normals, st = rec.SampleMesh(None, tri, n, seed, return_bary=True, return_normals=True)
    assert st == want["stats"], (what, st, want["stats"])
    assert points.dtype == np.float32 and t.dtype == np.uint32 and bary.dtype == np.float32 and normals.dtype == np.float32
    for name, got in zip(ARRAYS, (points, t, bary, normals)):
        assert got.shape == want[name].shape and got.tobytes() == want[name].tobytes(), (what, name)
    return want


@pytest.mark.parametrize("seed", (0, 0xFFFFFFFF))
def test_the_world_mesh_equals_the_model(world, seed):
    rec, tri, m = world["rec"], world["tri"], world["m"]
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 4097):
        want = _check(rec, m, tri, n, seed, "world n %d seed %d" % (n, seed))
        assert want["stats"]["n_none"] == 0
        # bary and normals NULL: the other two outputs are the same bytes
        points, t, st = rec.SampleMesh(None, tri, n, seed)
        assert st == want["stats"] and points.tobytes() == want["points"].tobytes() and t.tobytes() == want["tri"].tobytes()
    tm = rec.debug_sample_timings()
    assert list(tm) == ["weights", "scan", "draw"] and all(np.isfinite(v) and v >= 0 for v in tm.values()) and tm["draw"] > 0


def test_block_edges(smx):
    pos, nrm, r2, sheet = tc.world()
    rec = _rec_of(smx, (pos, nrm, r2), spare=100)
    arrays = {k: c["tri"] for k, c in tc.cases().items()}
    arrays["n_in = 513"] = sheet[:513]                        # a third workgroup and its offset
    for name, tri in arrays.items():
        for n in (300, 1):
            want = _check(rec, (pos, nrm, r2), tri, n, 3, name)
        if name in ("n_in = 0", "no triangle in R"):
            assert want["stats"]["total_weight"] == 0 and want["stats"]["n_none"] == 1
    rec.close()


def test_64_bit_weights_and_more_samples_than_units(smx, big):
    rec, m, tri = big["rec"], big["m"], big["tri"]
    for n in (1, 7, 4096):
        want = _check(rec, m, tri, n, 5, "big %d" % n)
        assert want["stats"]["stride"] >> 32 != 0 and want["stats"]["total_weight"] > 1 << 44
        tiny = int(np.sum(want["tri"] != 1))
        assert tiny <= 2
    # W < n_samples: every sample is "none"
    want = _check(rec, m, tri[[0, 2]], 1000000, 0, "tiny")
    assert want["stats"]["n_none"] == 1000000 and 0 < want["stats"]["total_weight"] < 1000000
    line = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [3.0, 3.0, 0.0]])
    lrec = _rec_of(smx, (line, _up(line), np.full(4, 0.01)), spare=100)
    want = _check(lrec, (line, None, np.full(4, 0.01)), np.array([[0, 1, 2], [1, 2, 3]], np.uint32), 10, 0, "collinear")
    assert want["stats"]["total_weight"] == 0 and want["stats"]["n_zero_weight"] == 2 and want["stats"]["n_none"] == 10
    lrec.close()


def _raw(rec, tri, n_in, n_samples, seed, points, out_tri, bary, normals, on_device=0, stats=True):
    """The C call itself; arrays: numpy arrays, device addresses (int) or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    st = _lib.SampleStats()
    rc = _lib.load().smx_recon_sample_mesh(rec._h, None, ptr(tri), C.c_uint32(n_in), C.c_uint32(n_samples), C.c_uint32(seed), ptr(points),
                                           ptr(out_tri), ptr(bary), ptr(normals), C.c_int32(on_device), C.byref(st) if stats else None)
    return rc, st


def _guards(P, extra=4):
    return [np.full(PER[k] * P + extra, GUARD, np.uint32) for k in ARRAYS]


def _untouched(g):
    return all(np.all(a == GUARD) for a in g)


def test_saturation_is_refused_and_the_largest_accepted_sum_equals_the_model(big):
    """The largest triangle the coordinate range allows has q = 2^44.79: 262 144 copies sum to 2^62.79 and the call is refused
    with nothing written; 131 072 (2^61.79) and 32 768 copies are accepted."""
    rec, m, tri = big["rec"], big["m"], big["tri"]
    many = np.ascontiguousarray(np.tile(tri[1:2], (262144, 1)))
    g = _guards(1000)
    rc, _ = _raw(rec, many, many.shape[0], 1000, 9, *g)
    assert rc == -1 and _untouched(g)
    from surfelmeshing_amd import _lib
    assert b"total area too large" in _lib.load().smx_last_error()
    for count in (131072, 32768):
        want = _check(rec, m, many[:count], 1000, 9, "%d large triangles" % count)
        assert want["stats"]["total_weight"] > 1 << 59


def test_calling_rules_on_host_and_device_arrays(smx, world):
    from surfelmeshing_amd import api
    rec, tri, m = world["rec"], world["tri"], world["m"]
    P, n_in, n = 777, tri.shape[0], m[0].shape[0]
    want = sr.sample(m[0], m[2], tri, P, 21)
    rows_before = rec.debug_download_surfels(n)
    # host arrays pre-filled with a guard word; room to spare stays untouched
    g = _guards(P)
    rc, st = _raw(rec, tri, n_in, P, 21, *g)
    assert rc == 0 and api.sample_stats_dict(st) == want["stats"]
    for name, a in zip(ARRAYS, g):
        assert a[:PER[name] * P].tobytes() == want[name].tobytes() and np.all(a[PER[name] * P:] == GUARD), name
    # two calls give the same bytes; bary, normals and stats NULL leave the others as they are
    g2 = _guards(P)
    rc, _ = _raw(rec, tri, n_in, P, 21, g2[0], g2[1], None, None, stats=False)
    assert rc == 0 and g2[0].tobytes() == g[0].tobytes() and g2[1].tobytes() == g[1].tobytes() and _untouched(g2[2:])
    assert rec.debug_sample_timings()["draw"] > 0
    # an index >= n, anywhere: refused, nothing written, only the weights phase published
    for where in (0, 3 * (n_in // 2) + 1, 3 * n_in - 1):
        bad = tri.copy()
        bad.reshape(-1)[where] = n
        gb = _guards(P)
        assert _raw(rec, bad, n_in, P, 21, *gb)[0] == -1 and _untouched(gb)
        tm = rec.debug_sample_timings()
        assert tm["scan"] == 0.0 and tm["draw"] == 0.0 and tm["weights"] >= 0.0
    # an output over the input: refused, nothing written
    both = np.concatenate([tri.reshape(-1), np.full(8, GUARD, np.uint32)])
    snapshot = both.copy()
    gb = _guards(P)
    assert _raw(rec, both, n_in, P, 21, gb[0], both[3 * n_in - 1:], gb[2], gb[3])[0] == -1 and both.tobytes() == snapshot.tobytes()
    assert _raw(rec, both, n_in, P, 21, gb[0], gb[1], gb[2], both[3 * n_in - 2:])[0] == -1 and _untouched(gb)
    # more than 2^28 samples or triangles: refused with nothing launched
    gb = _guards(4)
    assert _raw(rec, tri, n_in, (1 << 28) + 1, 21, *gb)[0] == -1 and _untouched(gb)
    assert _raw(rec, tri, (1 << 28) + 1, 4, 21, *gb)[0] == -1 and _untouched(gb)
    # device arrays with guard words beyond the end give the same bytes
    din = smx.CUDABuffer(1, 3 * n_in, np.uint32)
    sizes = [PER[k] * P + 4 for k in ARRAYS]
    outs = [smx.CUDABuffer(1, k, np.uint32) for k in sizes]
    din.Upload(tri.reshape(1, -1))
    for b, k in zip(outs, sizes):
        b.Upload(np.full((1, k), GUARD, np.uint32))
    a = [b.ToCUDA().address for b in [din] + outs]
    rc, st = _raw(rec, a[0], n_in, P, 21, a[1], a[2], a[3], a[4], on_device=1)
    assert rc == 0 and api.sample_stats_dict(st) == want["stats"]
    for b, host in zip(outs, g):
        assert b.Download()[0].tobytes() == host.tobytes()
    assert din.Download()[0].tobytes() == tri.tobytes()
    assert _raw(rec, a[0], n_in, P, 21, a[0] + 8, a[2], a[3], a[4], on_device=1)[0] == -1          # overlap on the device
    bad = tri.copy()
    bad[n_in // 3, 2] = n
    din.Upload(bad.reshape(1, -1))
    outs[1].Upload(np.full((1, sizes[1]), GUARD, np.uint32))
    assert _raw(rec, a[0], n_in, P, 21, a[1], a[2], a[3], a[4], on_device=1)[0] == -1 and np.all(outs[1].Download()[0] == GUARD)
    for b in [din] + outs:
        b.close()
    # the map is as it was
    assert rec.debug_download_surfels(n).tobytes() == rows_before.tobytes() and rec.surfels_size() == n


def test_a_device_tensor_through_the_python_call(world):
    import torch
    rec, tri, m = world["rec"], world["tri"], world["m"]
    P = 777
    want = sr.sample(m[0], m[2], tri, P, 21)
    tt = torch.from_numpy(tri.astype(np.int32)).cuda()
    tp, ti, tb, tn, tst = rec.SampleMesh(None, tt, P, 21, return_bary=True, return_normals=True)
    torch.cuda.synchronize()
    assert tst == want["stats"] and ti.cpu().numpy().view(np.uint32).tobytes() == want["tri"].tobytes()
    for name, got in (("points", tp), ("bary", tb), ("normals", tn)):
        assert got.cpu().numpy().tobytes() == want[name].tobytes(), name


def test_a_failed_allocation_writes_nothing_and_close_frees_everything(smx):
    base = smx.DebugLiveAllocations()
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    P, n_in = 500, tri.shape[0]
    want = sr.sample(m[0], m[2], tri, P, 2)
    failed = []
    try:
        for nth in range(20):
            g = _guards(P, 0)
            smx.DebugFailAllocation(nth)
            rc = _raw(rec, tri, n_in, P, 2, *g)[0]
            if rc == 0:
                break
            failed.append(rc)
            assert rc == -2 and _untouched(g), nth        # the allocation error, nothing written
            smx.DebugFailAllocation(-1)
            rec.close()                                   # a fresh object for the next allocation in line
            rec = _rec_of(smx, m)
    finally:
        smx.DebugFailAllocation(-1)
    # the counters, the two prefix arrays, the staged input and the four staged outputs
    assert rc == 0 and 8 <= len(failed) < 20, "the call reached %d allocations" % len(failed)
    for name, a in zip(ARRAYS, g):
        assert a.tobytes() == want[name].tobytes(), name
    assert smx.DebugLiveAllocations() > base
    rec.close()
    assert smx.DebugLiveAllocations() == base
