"""smx_recon_mesh_rim on the device.  The contract (include/smx.h) is made of integers, so everything here is compared for
EQUALITY with the model of tests/rim_ref.py: every byte and every statistic, with host and with device arrays, twice."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dr
import mesh_ref as mr
import rim_ref as rf

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5


def _rec_of(smx, pos, r2, spare=64):
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (pos.shape[0], 1))
    with np.errstate(over="ignore"):
        rows = mr.rows_of_map(pos, nrm, r2)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(np.asarray(r2) < 0)))
    return rec


@pytest.fixture(scope="module")
def maps(smx):
    """One object per map of the cases (the grid with its dead, far and NaN slots; corner(); the distance tests' world), and
    the model's answers, computed once and left unchanged."""
    recs, models = {}, {}

    def rec_for(pos, r2):
        k = id(pos)
        if k not in recs:
            recs[k] = _rec_of(smx, pos, r2)
        return recs[k]

    def model(name, pos, r2, tri):
        if name not in models:
            want, wst = rf.rim(pos, r2, tri)
            want.setflags(write=False)
            models[name] = (want, wst)
        return models[name]
    yield rec_for, model
    for r in recs.values():
        r.close()


def _raw(rec, tin, n_in, out, on_device=0, stats=True):
    """The C call itself; tin / out: numpy arrays, device addresses (int) or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    st = _lib.RimStats()
    for n, _ in _lib.RimStats._fields_:
        setattr(st, n, 0xDEAD)
    rc = _lib.load().smx_recon_mesh_rim(rec._h, None, ptr(tin), C.c_uint32(n_in), C.c_int32(on_device), ptr(out), C.byref(st) if stats else None)
    return rc, {n: int(getattr(st, n)) for n, _ in _lib.RimStats._fields_}


CASES = rf.cases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_every_case_equals_the_model_on_host_and_device_arrays_twice(smx, maps, k):
    name, pos, r2, tri, _, _ = CASES[k]
    rec_for, model = maps
    rec = rec_for(pos, r2)
    want, wst = model(name, pos, r2, tri)
    n_in = tri.shape[0]
    for _ in range(2):
        got, st = rec.MeshRim(None, tri)
        assert got.dtype == np.uint8 and got.shape == (n_in,) and st == wst, (name, st, wst)
        assert got.tobytes() == want.tobytes(), name
    din, dout = smx.CUDABuffer(1, 3 * n_in, np.uint32), smx.CUDABuffer(1, n_in + 8, np.uint8)
    din.Upload(tri.reshape(1, -1))
    for _ in range(2):
        dout.Upload(np.full((1, n_in + 8), GUARD, np.uint8))
        rc, st = _raw(rec, din.ToCUDA().address, n_in, dout.ToCUDA().address, on_device=1)
        back = dout.Download()[0]
        assert rc == 0 and st == wst and back[:n_in].tobytes() == want.tobytes() and np.all(back[n_in:] == GUARD), name
    assert din.Download()[0].tobytes() == tri.tobytes()          # the input is left alone
    din.close()
    dout.close()


def test_the_world_of_the_distance_tests(smx, maps):
    """About 10 000 triangles in 38 workgroups: the noisy sphere, the holed plane, the hand-made triangles."""
    pos, _, r2, tri, _ = dr.world()
    rec_for, model = maps
    rec = rec_for(pos, r2)
    want, wst = model("world", pos, r2, tri)
    for arr, w in ((tri, want), (tri[::-1].copy(), want[::-1])):
        got, st = rec.MeshRim(None, arr)
        assert st == wst and got.tobytes() == w.tobytes()
    assert wst["n_nonmanifold_edges"] >= 1 and wst["n_rim_edges"] > 100


def test_calling_rules(smx, maps):
    rec_for, _ = maps
    pos, r2 = rf.grid_map()
    rec = rec_for(pos, r2)
    g = rf.grid_triangles()
    out = np.full(g.shape[0] + 8, GUARD, np.uint8)
    # an index >= n, anywhere: refused, nothing written, the statistics untouched
    for _, _, bad in rf.refused():
        rc, st = _raw(rec, bad, bad.shape[0], out)
        assert rc == -1 and np.all(out == GUARD) and st["n_in"] == 0xDEAD
    # n_in = 0, with and without arrays
    rc, st = _raw(rec, None, 0, None)
    assert rc == 0 and all(v == 0 for v in st.values())
    rc, st = _raw(rec, g, 0, out)
    assert rc == 0 and np.all(out == GUARD)
    # NULL statistics; room to spare stays untouched
    rc, _ = _raw(rec, g, g.shape[0], out, stats=False)
    assert rc == 0 and out[:g.shape[0]].tobytes() == rf.rim(pos, r2, g)[0].tobytes() and np.all(out[g.shape[0]:] == GUARD)
    # the call after a refusal equals the model
    got, st = rec.MeshRim(None, g)
    assert (got.tobytes(), st) == (rf.rim(pos, r2, g)[0].tobytes(), rf.rim(pos, r2, g)[1])
    # a map without slots: every index is out of range
    empty = smx.CUDASurfelReconstruction(64, smx.PinholeCamera4f(*CAM))
    assert _raw(empty, np.zeros((1, 3), np.uint32), 1, out[:1].copy())[0] == -1
    assert _raw(empty, None, 0, None)[0] == 0
    empty.close()


def test_no_side_effects(smx):
    pos, nrm, r2 = mr.sphere_map(n=1500)
    rec = _rec_of(smx, pos, r2)
    tri, _ = rec.Triangulate(None)
    n = rec.surfels_size()
    rows_before, stats_before = rec.debug_download_surfels(n), rec.stats()
    got, st = rec.MeshRim(None, tri)
    want, wst = rf.rim(pos, r2, tri)
    assert got.tobytes() == want.tobytes() and st == wst and st["n_rim_edges"] > 0
    assert rec.stats() == stats_before and rec.surfels_size() == n
    assert rec.debug_download_surfels(n).tobytes() == rows_before.tobytes()
    # the rim edges are what FillHoles calls boundary edges
    assert rec.FillHoles(None, tri)[1]["n_boundary_edges"] == st["n_rim_edges"]
    rec.close()


def test_a_failed_allocation_writes_nothing_and_the_next_call_succeeds(smx):
    base = smx.DebugLiveAllocations()
    pos, r2 = rf.grid_map()
    g = rf.grid_triangles()
    want, wst = rf.rim(pos, r2, g)
    rec = _rec_of(smx, pos, r2)
    out = np.full(g.shape[0], GUARD, np.uint8)
    try:
        for nth in range(12):
            smx.DebugFailAllocation(nth)
            rc, st = _raw(rec, g, g.shape[0], out)
            if rc == 0:
                break
            assert np.all(out == GUARD) and st["n_in"] == 0xDEAD, nth
            smx.DebugFailAllocation(-1)
            got, st = rec.MeshRim(None, g)                 # the object is usable, the next call equals the model
            assert st == wst and got.tobytes() == want.tobytes()
            rec.close()                                   # a fresh object for the next allocation in line
            rec = _rec_of(smx, pos, r2)
    finally:
        smx.DebugFailAllocation(-1)
    assert rc == 0 and nth == 5, "the call reached %d allocations" % nth      # counters, table, bitmap, bytes, staging
    assert out.tobytes() == want.tobytes() and st == wst
    rec.close()
    assert smx.DebugLiveAllocations() == base


def test_create_call_destroy_frees_everything(smx):
    base = smx.DebugLiveAllocations()
    pos, r2 = rf.grid_map()
    for _ in range(2):
        rec = _rec_of(smx, pos, r2)
        rec.MeshRim(None, rf.grid_triangles())
        assert smx.DebugLiveAllocations() > base
        rec.close()
        assert smx.DebugLiveAllocations() == base
