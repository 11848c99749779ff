"""smx_recon_triangulate and smx_recon_triangulate_update on the maps of tests/mesh_cases.py: hand-built maps that reach
the ends of the star logic (a full ring row and its wrap, overflow, open stars, every drop, every rejection), each clear
of every tie by the margin rule that tests/test_mesh_cases.py asserts on the CPU.  So the comparison with the float64 /
Qhull model of tests/mesh_ref.py is exact here: the same bytes and the same five statistics, with no cap."""
import ctypes as C

import numpy as np
import pytest

import mesh_cases as mc
import mesh_ref as mr
import mesh_update_ref as mu

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
CELLS = (1.25, 2.5)      # (the maps' unit is a ring's radius; with 2.5 the update's coarse filter is in use, with 1.25 it is not)
CASES = mc.cases()


def _pod(prm):
    from surfelmeshing_amd._lib import MeshParams
    return MeshParams.defaults(max_angle_between_normals_deg=prm.max_angle_between_normals_deg,
                               min_triangle_angle_deg=prm.min_triangle_angle_deg,
                               max_triangle_angle_deg=prm.max_triangle_angle_deg,
                               search_radius_factor=prm.search_radius_factor, max_neighbors=prm.max_neighbors)


def _upload(rec, m):
    rec.debug_upload_surfels(mr.rows_of_map(*m), int(np.sum(m[2] < 0)))


@pytest.fixture(scope="module")
def models():
    """mesh_ref.triangulate of every case and every update step, computed once."""
    out = {c.name: mr.triangulate(*c.map, c.prm)[:2] for c in CASES}
    steps, _ = mc.update_steps()
    for name, m, _ in steps:
        out[name] = mr.triangulate(*m, mr.Params())[:2]
    return out, steps


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_full_call_equals_the_model_exactly(smx, models, case):
    want, wst = models[0][case.name]
    rec = smx.CUDASurfelReconstruction(case.pos.shape[0] + 64, smx.PinholeCamera4f(*CAM))
    _upload(rec, case.map)
    for cell in CELLS:
        got, st = rec.Triangulate(None, _pod(case.prm), cell_size=cell)
        print("%s, cell %g: GPU %s, model %s" % (case.name, cell, st, wst))
        assert got.dtype == np.uint32 and got.shape == want.shape, (got.shape, want.shape)
        assert got.tobytes() == want.tobytes()
        assert st == wst
    rec.close()


def test_guard_words_behind_an_owner_of_sixteen_at_the_end_of_the_output(smx, models):
    from surfelmeshing_amd import _lib
    case = next(c for c in CASES if c.name == "trip")
    want, _ = models[0]["trip"]
    T = want.shape[0]
    assert np.all(want[-16:, 0] == case.roles["owners"][2])
    rec = smx.CUDASurfelReconstruction(case.pos.shape[0] + 64, smx.PinholeCamera4f(*CAM))
    _upload(rec, case.map)
    L, nn, p = _lib.load(), smx.SurfelNeighborIndex(), _pod(case.prm)
    guard = 0xA5A5A5A5
    for capacity in (T - 1, T):
        buf = np.full(3 * T + 8, guard, np.uint32)
        n, st = C.c_uint32(0), _lib.MeshStats()
        rc = L.smx_recon_triangulate(rec._h, None, nn._h, C.c_float(CELLS[0]), C.byref(p), buf.ctypes.data_as(C.c_void_p),
                                     C.c_uint32(capacity), C.c_int32(0), C.byref(n), C.byref(st))
        assert n.value == T and st.n_triangles == T
        if capacity < T:
            assert rc == -1 and np.all(buf == guard)                 # nothing is written
        else:
            assert rc == 0 and buf[:3 * T].tobytes() == want.tobytes() and np.all(buf[3 * T:] == guard)
    nn.close()
    rec.close()


@pytest.mark.parametrize("cell", CELLS)
def test_update_follows_the_composite_through_its_steps(smx, models, cell):
    model, steps = models
    n_max = max(m[0].shape[0] for _, m, _ in steps)
    rec = smx.CUDASurfelReconstruction(n_max + 64, smx.PinholeCamera4f(*CAM))
    nn = smx.SurfelNeighborIndex()
    pod = _pod(mr.Params())
    before = prev_map = None
    for name, m, touched in steps:
        _upload(rec, m)
        tri, st, us = rec.TriangulateUpdate(None, pod, index=nn, cell_size=cell)
        ref = smx.CUDASurfelReconstruction(n_max + 64, smx.PinholeCamera4f(*CAM))      # a fresh object holding the same rows
        _upload(ref, m)
        full, fst = ref.Triangulate(None, pod, cell_size=cell)
        ref.close()
        want, wst = model[name]
        print("%s, cell %g: update %s, stats %s, model %s" % (name, cell, us, st, wst))
        assert tri.tobytes() == full.tobytes() and st == fst              # equals the full call on a fresh object
        assert tri.tobytes() == want.tobytes() and st == wst              # and the model
        if name == "U0":
            assert us["mode"] == 1
        else:
            assert us["mode"] == 0 and us["n_changed"] == touched
            assert us["n_dirty"] == int(mu.dirty_mask(prev_map, m, mr.Params()).sum())
        if name == "U1":
            assert st["star_overflow"] == before[1]["star_overflow"] - 1 and st["n_triangles"] == before[1]["n_triangles"] + 16
        if name == "U2":
            assert us["n_kept_triangles"] > 0 and st["n_triangles"] == before[1]["n_triangles"] - 16
        if name == "U5":
            assert us["n_dirty"] == 0 and us["n_kept_triangles"] == tri.shape[0] and (tri.tobytes(), st) == before
        before, prev_map = (tri.tobytes(), st), m
    nn.close()
    rec.close()
