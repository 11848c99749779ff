"""smx_recon_triangulate_update on the chains of tests/mesh_update_cases.py: maps that put the coarse filter, the D
condition, the ghost rows, the kept runs, the kept buffers' re-allocation and the path choice where they decide.  Every
step keeps the margin rule (tests/test_mesh_update_cases.py), so the comparison with the float64 / Qhull model is exact:
the bytes and the five statistics of smx_recon_triangulate on a fresh object holding the same rows and of the model, and
mode, n_changed, n_dirty, n_reagreed and n_kept_triangles of tests/mesh_update_ref.model_call."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as mr
import mesh_update_cases as uc

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
SMX_ERR_HIP = -2
CHAINS = uc.chains()
# (chain, the cell the update is called with): each chain with its own, F, Ff and D again with one under which no slot is filtered
RUNS = [(c, None) for c in CHAINS] + [(uc.chain(name), cell) for name, cell in uc.H_UNFILTERED.items()]
RUN_IDS = [c.name if cell is None else "%s_cell_%g" % (c.name, cell) for c, cell in RUNS]


def _pod(prm):
    from surfelmeshing_amd._lib import MeshParams
    return MeshParams.defaults(max_angle_between_normals_deg=prm.max_angle_between_normals_deg,
                               min_triangle_angle_deg=prm.min_triangle_angle_deg,
                               max_triangle_angle_deg=prm.max_triangle_angle_deg,
                               search_radius_factor=prm.search_radius_factor, max_neighbors=prm.max_neighbors)


def _upload(rec, m):
    rec.debug_upload_surfels(mr.rows_of_map(*m), int(np.sum(m[2] < 0)))


def _new(smx, ch):
    n_max = max(s.n for s in ch.steps)
    return smx.CUDASurfelReconstruction(n_max + 64, smx.PinholeCamera4f(*CAM)), smx.SurfelNeighborIndex()


def _update(rec, nn, s, cell=None):
    return rec.TriangulateUpdate(None, _pod(s.prm), index=nn, cell_size=s.cell if cell is None else cell, full_above_fraction=s.fraction)


def _raw(smx, rec, nn, s, buf, capacity, on_device=0):
    """One smx_recon_triangulate_update call through the C interface: (rc, n_triangles, stats, update stats)."""
    from surfelmeshing_amd import _lib
    p = _pod(s.prm)
    n, st, us = C.c_uint32(0), _lib.MeshStats(), _lib.MeshUpdateStats()
    ptr = None if buf is None else (C.c_void_p(buf) if on_device else buf.ctypes.data_as(C.c_void_p))
    rc = _lib.load().smx_recon_triangulate_update(rec._h, None, nn._h, C.c_float(s.cell), C.byref(p),
                                                  C.c_float(-1.0 if s.fraction is None else s.fraction), ptr, C.c_uint32(capacity),
                                                  C.c_int32(on_device), C.byref(n), C.byref(st), C.byref(us))
    return rc, n.value, {k: int(getattr(st, k)) for k, _ in _lib.MeshStats._fields_}, {k: int(getattr(us, k)) for k, _ in _lib.MeshUpdateStats._fields_}


@pytest.mark.parametrize("ch,cell", RUNS, ids=RUN_IDS)
def test_update_follows_every_chain_step_by_step(smx, ch, cell):
    truths, calls = uc.truths(ch), uc.model_calls(ch, cell=cell)
    own = uc.model_calls(ch)
    rec, nn = _new(smx, ch)
    for k, s in enumerate(ch.steps):
        _upload(rec, s.map)
        tri, st, us = _update(rec, nn, s, cell)
        ref, ref_nn = _new(smx, ch)                                        # a fresh object holding the same rows
        _upload(ref, s.map)
        full, fst = ref.Triangulate(None, _pod(s.prm), index=ref_nn, cell_size=s.cell if cell is None else cell)
        ref_nn.close()
        ref.close()
        want, c = truths[k], calls[k]
        print("%s, cell %g: update %s, stats %s; model %s, %s" % (s.name, s.cell if cell is None else cell, us, st, c.stats(), want.stats))
        assert tri.dtype == np.uint32 and tri.shape == full.shape
        assert tri.tobytes() == full.tobytes() and st == fst                       # equals the full call on a fresh object
        assert tri.tobytes() == want.tri.tobytes() and st == want.stats           # and the model
        assert (us["mode"], us["n_changed"], us["n_dirty"]) == (c.mode, c.n_changed, c.n_dirty)
        assert us["n_dirty"] <= us["n_reagreed"] <= s.n
        assert us["n_reagreed"] == c.n_reagreed                                    # |A|: D and the old and new rings of its slots
        assert us["n_kept_triangles"] == c.n_kept_triangles
        assert c.n_dirty == own[k].n_dirty                                         # (whatever the cell: the filter decides nothing)
        for key in ("mode", "n_changed", "n_dirty"):
            if key in s.designed:
                assert us[key] == s.designed[key], (s.name, key)
    nn.close()
    rec.close()


@pytest.mark.parametrize("on_device", [0, 1], ids=["host_pointer", "device_pointer"])
def test_capacity_rule_on_the_incremental_path(smx, on_device):
    """Step W1 (one changed slot, 64 kept and 16 new triangles): a buffer one triangle short gets nothing, the state has
    advanced all the same, and the second call finds nothing changed and copies the kept array out."""
    ch = uc.chain("W")
    s, want, c = ch.steps[1], uc.truths(ch)[1], uc.model_calls(ch)[1]
    T = want.tri.shape[0]
    assert c.mode == 0 and c.n_changed == 1 and 0 < c.n_kept_triangles < T
    rec, nn = _new(smx, ch)
    _upload(rec, ch.steps[0].map)
    assert _update(rec, nn, ch.steps[0])[2]["mode"] == 1
    _upload(rec, s.map)
    words = 3 * T + 8
    host = np.full(words, GUARD, np.uint32)
    dbuf = smx.CUDABuffer(1, words, np.uint32) if on_device else None

    def fill():
        host[:] = GUARD
        if on_device:
            dbuf.Upload(host.reshape(1, words))
        return dbuf.ToCUDA().address if on_device else host

    def read():
        return dbuf.Download()[0] if on_device else host
    rc, n, st, us = _raw(smx, rec, nn, s, fill(), T - 1, on_device)
    assert rc == -1 and n == T and st == want.stats
    assert us == dict(mode=0, n_changed=c.n_changed, n_dirty=c.n_dirty, n_reagreed=us["n_reagreed"], n_kept_triangles=c.n_kept_triangles)
    assert np.all(read() == GUARD)                                                 # nothing is written
    rc, n, st, us = _raw(smx, rec, nn, s, fill(), T, on_device)
    assert rc == 0 and n == T and st == want.stats
    assert us == dict(mode=0, n_changed=0, n_dirty=0, n_reagreed=0, n_kept_triangles=T)
    back = read()
    assert back[:3 * T].tobytes() == want.tri.tobytes() and np.all(back[3 * T:] == GUARD)
    if dbuf is not None:
        dbuf.close()
    nn.close()
    rec.close()


@pytest.mark.parametrize("name,k", [("Wr", 1), ("F", 1)], ids=["growth_that_reallocates", "incremental_step"])
def test_an_allocation_failure_anywhere_in_the_update_is_recovered_from(smx, name, k):
    """The failure is injected at allocation 0, 1, 2, ... of the call of step k, each time on a fresh object taken through
    the steps before (so that Wr1 re-allocates its kept buffers every time), until the call succeeds: that counts the
    call's allocations.  A failed call returns an error, writes nothing and holds no more than a successful one; the next
    call has no state (mode 1) and equals the full call; destroying the object gives everything back."""
    ch = uc.chain(name)
    s, want = ch.steps[k], uc.truths(ch)[k]
    c = uc.model_calls(ch)[k]
    T = want.tri.shape[0]
    if name == "Wr":
        assert all(uc.reallocates(ch.steps[0].n, s.n).values())                    # (reserve_keep copies in this call)
    start = smx.DebugLiveAllocations()
    held = None
    try:
        for nth in range(-1, 81):
            assert nth < 80, "%s still fails with allocation %d armed" % (s.name, nth)
            rec, nn = _new(smx, ch)
            for prev in ch.steps[:k]:
                _upload(rec, prev.map)
                _update(rec, nn, prev)
            _upload(rec, s.map)
            buf = np.full(3 * T + 8, GUARD, np.uint32)
            before = smx.DebugLiveAllocations()
            smx.DebugFailAllocation(nth)
            rc, n, st, us = _raw(smx, rec, nn, s, buf, T)
            smx.DebugFailAllocation(-1)
            after = smx.DebugLiveAllocations()
            if rc == 0:
                assert buf[:3 * T].tobytes() == want.tri.tobytes() and np.all(buf[3 * T:] == GUARD) and st == want.stats
                assert (us["mode"], us["n_changed"], us["n_dirty"]) == (c.mode, c.n_changed, c.n_dirty)
                if held is None:
                    held = (after[0] - before[0], after[1] - before[1])
                assert (after[0] - before[0], after[1] - before[1]) == held
            else:
                assert rc == SMX_ERR_HIP, (nth, rc)
                assert np.all(buf == GUARD), "the call that failed at allocation %d wrote to the caller's buffer" % nth
                assert after[0] - before[0] <= held[0] and after[1] - before[1] <= held[1], (nth, before, after, held)
                rc2, n2, st2, us2 = _raw(smx, rec, nn, s, buf, T)                  # the next call: no state, the full path
                assert rc2 == 0 and us2["mode"] == 1 and n2 == T and st2 == want.stats
                assert buf[:3 * T].tobytes() == want.tri.tobytes() and np.all(buf[3 * T:] == GUARD)
            nn.close()
            rec.close()
            assert smx.DebugLiveAllocations() == start, "allocation %d: something stayed behind after destroy" % nth
            if rc == 0 and nth >= 0:
                break
    finally:
        smx.DebugFailAllocation(-1)
    print("%s: the call makes %d allocations and keeps %d blocks, %d bytes" % (s.name, nth, held[0], held[1]))
    assert nth >= held[0] > 0       # every block the call keeps was visited (it also frees and replaces blocks on the way)


@pytest.mark.parametrize("ch", CHAINS, ids=[c.name for c in CHAINS])
def test_two_objects_fed_the_same_chain_agree_at_every_step(smx, ch):
    """Nothing depends on scheduling: the ghosts' order, the racing byte stores into the A row, the atomicOr into the bit table."""
    a, b = _new(smx, ch), _new(smx, ch)
    for s in ch.steps:
        outs = []
        for rec, nn in (a, b):
            _upload(rec, s.map)
            tri, st, us = _update(rec, nn, s)
            outs.append((tri.tobytes(), st, us))
        assert outs[0] == outs[1], s.name
    for rec, nn in (a, b):
        nn.close()
        rec.close()
