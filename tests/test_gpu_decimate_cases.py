"""smx_recon_decimate_mesh on the device at the cases of tests/decimate_cases.py: hand-built maps and triangle arrays that sit
on the cell faces, the tie, the ends of the key fields and of the coordinate range, a cell larger than any coordinate, probe
chains that wrap in both tables, one corner set held by thousands of triangles, the switches of the table sizes and every
pass count of the two sorts.  Everything is compared for EQUALITY with the model of tests/decimate_ref.py -- the triangle
array, the vertex map and every statistic -- which tests/test_decimate_cases.py holds to a brute force and to the host walk
of the kernels, and whose census and mutants say what each case is there for."""
import ctypes as C

import numpy as np
import pytest

import decimate_cases as dc
import decimate_ref as dr
import mesh_ref as mr

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5A5A5A5
NAMES = [c.name for c in dc.cases()]

_MODEL = {}


def _model(c, label):
    if (c.name, label) not in _MODEL:
        _MODEL[(c.name, label)] = dr.decimate(c.pos, c.r2, dict(c.arrays)[label], c.cell)
    return _MODEL[(c.name, label)]


def _upload(rec, c):
    rec.debug_upload_surfels(mr.rows_of_map(*c.map()), int(np.sum(c.r2 < 0)))
    assert rec.surfels_size() == c.n


def _rec_of(smx, c, spare=8):
    rec = smx.CUDASurfelReconstruction(c.n + spare, smx.PinholeCamera4f(*CAM))
    _upload(rec, c)
    return rec


def _equals_model(rec, c, label):
    tri = dict(c.arrays)[label]
    got, st, vmap = rec.DecimateMesh(None, tri, c.cell, return_vertex_map=True)
    want, wmap, wst = _model(c, label)
    print("%s/%s, cell %g: GPU %s" % (c.name, label, c.cell, st))
    assert got.dtype == np.uint32 and got.shape == (st["n_triangles"], 3) and vmap.shape == (c.n,)
    assert st == wst
    assert got.tobytes() == want.tobytes()
    assert vmap.tobytes() == wmap.tobytes()
    dr.check_properties(got, vmap, st)
    return got, st, vmap


def _raw(rec, cell, tin, n_in, out, capacity, vmap, on_device=0):
    """The C call itself; tin / out / vmap: numpy arrays, device addresses (int) or None."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p)
    n, st = C.c_uint32(0xDEAD), _lib.DecimateStats()
    rc = _lib.load().smx_recon_decimate_mesh(rec._h, None, C.c_float(cell), ptr(tin), C.c_uint32(n_in), ptr(out),
                                             C.c_uint32(capacity), ptr(vmap), C.c_int32(on_device), C.byref(n), C.byref(st))
    return rc, n.value, st


def _refused_writes_nothing(rec, c, tri):
    from surfelmeshing_amd import _lib
    n_in = tri.shape[0]
    out, vmap = np.full(3 * n_in + 8, GUARD, np.uint32), np.full(c.n + 8, GUARD, np.uint32)
    rc, _, _ = _raw(rec, c.cell, tri, n_in, out, n_in, vmap)
    assert rc == -1
    assert np.all(out == GUARD) and np.all(vmap == GUARD)
    assert b"too small" in _lib.load().smx_last_error()


def _run_case(rec, c):
    """Every array of the case on an object that holds its map."""
    for label, _ in c.arrays:
        _equals_model(rec, c, label)
    for _, tri in c.refused:
        _refused_writes_nothing(rec, c, tri)


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_model(smx, name):
    c = dc.case(name)
    rec = _rec_of(smx, c)
    for label, _ in c.arrays:
        got, st, vmap = _equals_model(rec, c, label)
        for k, v in c.expect.get(label, {}).items():      # what the case says by hand
            if k == "vmap":
                assert {i: int(vmap[i]) for i in v} == v, (name, label)
            elif k == "out":
                assert got.tolist() == [list(t) for t in v], (name, label)
            else:
                assert st[k] == v, (name, label, k)
    rec.close()


def test_range_edges_refused_arrays_write_nothing(smx):
    from surfelmeshing_amd import _lib
    c = dc.case("range_edges")
    rec = _rec_of(smx, c)
    assert len(c.refused) == 2
    for label, tri in c.refused:
        with pytest.raises(dr.CellRangeError):
            dr.decimate(c.pos, c.r2, tri, c.cell)
        _refused_writes_nothing(rec, c, tri)
        with pytest.raises(_lib.SmxError):
            rec.DecimateMesh(None, tri, c.cell)
        # the refusal leaves the object as it was: the accepted extremes right behind it
        for accepted, _ in c.arrays:
            _equals_model(rec, c, accepted)
    rec.close()


@pytest.mark.parametrize("name", ["one_corner_set", "cell_table_wrap", "tri_table_wrap", "ties"])
def test_twice_and_with_device_arrays(smx, name):
    c = dc.case(name)
    rec = _rec_of(smx, c)
    for label, tri in c.arrays:
        got, st, vmap = _equals_model(rec, c, label)
        again, st2, vmap2 = rec.DecimateMesh(None, tri, c.cell, return_vertex_map=True)
        assert again.tobytes() == got.tobytes() and st2 == st and vmap2.tobytes() == vmap.tobytes()
        # the device-pointer form, twice as well: the same bytes, nothing behind them
        T, n_in, n = got.shape[0], tri.shape[0], c.n
        din, dout, dmap = (smx.CUDABuffer(1, k, np.uint32) for k in (3 * n_in, 3 * T + 8, n + 8))
        din.Upload(tri.reshape(1, -1))
        for _ in range(2):
            dout.Upload(np.full((1, 3 * T + 8), GUARD, np.uint32))
            dmap.Upload(np.full((1, n + 8), GUARD, np.uint32))
            rc, nt, dst = _raw(rec, c.cell, din.ToCUDA().address, n_in, dout.ToCUDA().address, T, dmap.ToCUDA().address, on_device=1)
            assert rc == 0 and nt == T and {k: int(getattr(dst, k)) for k in st} == st
            back, mback = dout.Download()[0], dmap.Download()[0]
            assert back[:3 * T].tobytes() == got.tobytes() and np.all(back[3 * T:] == GUARD)
            assert mback[:n].tobytes() == vmap.tobytes() and np.all(mback[n:] == GUARD)
        assert din.Download()[0].tobytes() == tri.tobytes()          # the input is left alone
        for b in (din, dout, dmap):
            b.close()
    rec.close()


def _walk_order():
    """Largest, smallest, largest; then every other case; the largest once more."""
    big, small = dc.case("sort_widths/65537"), dc.case("table_sizes/one_in_1000")
    assert big.n == max(c.n for c in dc.cases()) and dict(small.arrays)["all"].shape[0] == 1
    assert dict(big.arrays)["all"].shape[0] > 2048
    rest = [c for c in dc.cases() if c.name not in (big.name, small.name)]
    return [big, small, big] + rest + [big]


@pytest.mark.parametrize("direction", ["forwards", "reversed"])
def test_one_object_runs_every_case_large_small_large(smx, direction):
    """The workspace is kept between calls and only the current call's prefix of each table is reset: a small call behind a
    large one, and a large one behind that, each on a re-uploaded map, have to see nothing of what the other left."""
    before = smx.DebugLiveAllocations()
    order = _walk_order()
    if direction == "reversed":
        order = order[::-1]
    rec = smx.CUDASurfelReconstruction(max(c.n for c in order) + 8, smx.PinholeCamera4f(*CAM))
    for c in order:
        _upload(rec, c)
        _run_case(rec, c)
    held = smx.DebugLiveAllocations()
    assert held[0] > before[0]                      # the workspace belongs to the object ...
    rec.close()
    assert smx.DebugLiveAllocations() == before     # ... and goes with it
