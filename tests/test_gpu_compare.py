"""smx_recon_compare_meshes on the device.  A side of the comparison is by definition smx_recon_sample_mesh followed by
smx_recon_mesh_distance, so every word of its statistics is compared for EQUALITY with the chain of the two brute-force models
(tests/sample_ref.py, tests/distance_ref.py): the sample statistics, the distance statistics with the histogram, and the three
exact sums.  The grid's three counts are defined only for an explicit cell size and compared then; cell_size_used never."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dr
import mesh_ref as mr
import sample_ref as sr

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
N, SEED = 600, 17            # 600 samples x 10 000 triangles: a brute-force side in about a second
GRID = ("n_wide", "n_entries", "n_cells")


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


@pytest.fixture(scope="module")
def world(smx):
    """The world of tests/distance_ref.py with three meshes derived from its triangle array on the device (each service is
    pinned to its own model elsewhere), and the model sides computed once per (from, onto, max_distance, cell_size)."""
    pos, nrm, r2, tri, info = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    meshes = dict(fine=tri, coarse10=rec.DecimateMesh(None, tri, 0.1)[0], coarse3=rec.DecimateMesh(None, tri, 0.03)[0],
                  filled=rec.FillHoles(None, tri)[0])
    sides = {}

    def model(a, b, max_distance, cell_size):
        key = (a, b, max_distance, cell_size)
        if key not in sides:
            s = sr.compare_side(pos, r2, meshes[a], meshes[b], max_distance, N, SEED, cell_size)
            s.pop("_")
            sides[key] = s
        return sides[key]
    yield dict(m=(pos, nrm, r2), rec=rec, meshes=meshes, model=model)
    rec.close()


def _same_side(got, want, cell_size, what):
    got = dict(got, distance=dict(got["distance"]))
    want = dict(want, distance=dict(want["distance"]))
    got["distance"].pop("cell_size_used")
    if not cell_size > 0:
        for k in GRID:
            got["distance"].pop(k)
    assert got == want, (what, got, want)


def _is_zero(side):
    flat = [v for v in side["sample"].values()] + [v for k, v in side["distance"].items() if k not in ("histogram", "max_distance")]
    return not any(flat) and not any(side["distance"]["histogram"]) and side["sum_d"] == side["sum_sq_lo"] == side["sum_sq_hi"] == 0


@pytest.mark.parametrize("other,max_distance,cell_size", (("coarse10", 0.5, 0.0), ("coarse3", 0.02, 0.05), ("filled", 0.02, 0.0)))
def test_both_sides_equal_the_chain_of_the_two_models(world, other, max_distance, cell_size):
    from surfelmeshing_amd import meshing
    rec, meshes = world["rec"], world["meshes"]
    got = rec.CompareMeshes(None, meshes["fine"], meshes[other], max_distance, N, SEED, cell_size)
    want_ab, want_ba = world["model"]("fine", other, max_distance, cell_size), world["model"](other, "fine", max_distance, cell_size)
    _same_side(got["a_to_b"], want_ab, cell_size, "fine -> " + other)
    _same_side(got["b_to_a"], want_ba, cell_size, other + " -> fine")
    assert want_ab["distance"]["n_matched"] > N // 2 and want_ba["sum_d"] > 0
    print(meshing.format_mesh_comparison(meshing.comparison_summary(got), ("fine", other)))
    tm = rec.debug_compare_timings()
    assert len(tm) == 6 and all(np.isfinite(v) and v >= 0 for v in tm.values()) and tm["a_to_b.distance"] > 0 and tm["b_to_a.sample"] > 0


def test_directions_and_a_side_not_asked_for_is_zeros(world):
    rec, meshes = world["rec"], world["meshes"]
    want_ab, want_ba = world["model"]("fine", "coarse10", 0.5, 0.0), world["model"]("coarse10", "fine", 0.5, 0.0)
    one = rec.CompareMeshes(None, meshes["fine"], meshes["coarse10"], 0.5, N, SEED, directions=1)
    _same_side(one["a_to_b"], want_ab, 0.0, "directions 1")
    assert _is_zero(one["b_to_a"])
    tm = rec.debug_compare_timings()
    assert tm["b_to_a.sample"] == tm["b_to_a.distance"] == tm["b_to_a.sums"] == 0.0 and tm["a_to_b.distance"] > 0
    two = rec.CompareMeshes(None, meshes["fine"], meshes["coarse10"], 0.5, N, SEED, directions=2)
    _same_side(two["b_to_a"], want_ba, 0.0, "directions 2")
    assert _is_zero(two["a_to_b"])
    # the motivating case: the coarse vertices are fine vertices, yet the coarse surface is not the fine one
    assert want_ba["distance"]["max_dist2_bits"] > 0


def test_a_mesh_against_itself_matches_every_sample(world):
    rec, meshes = world["rec"], world["meshes"]
    got = rec.CompareMeshes(None, meshes["fine"], meshes["fine"], 0.001, 5000, 3)
    for side in (got["a_to_b"], got["b_to_a"]):
        assert side["sample"]["n_none"] == 0 and side["distance"]["n_matched"] == 5000 and side["distance"]["n_bad_points"] == 0
        assert side["sum_d"] <= 8 * 5000 and side["sum_sq_hi"] == 0       # (float32 rounding: sample_ref.point_error_bound, 6e-6 m at 3 m)
    assert got["a_to_b"] == got["b_to_a"]
    # every sample "none": none of them matches, and the distance half counts them as bad points
    pos, r2 = world["m"][0], world["m"][2]
    dead = np.array([[0, 0, 1], [2, 2, 3]], np.uint32)
    got = rec.CompareMeshes(None, dead, meshes["fine"], 0.02, 100, 3, directions=1)["a_to_b"]
    assert got["sample"]["n_none"] == 100 and got["distance"]["n_bad_points"] == 100 and got["distance"]["n_matched"] == 0
    _same_side(got, {k: v for k, v in sr.compare_side(pos, r2, dead, meshes["fine"], 0.02, 100, 3).items() if k != "_"}, 0.0, "none")


def _raw(rec, prm, a, n_a, b, n_b, on_device, fill=0xA5):
    from surfelmeshing_amd import _lib
    st = _lib.CompareStats()
    C.memset(C.byref(st), fill, C.sizeof(st))
    ptr = lambda x: None if x is None else C.c_void_p(x) if isinstance(x, int) else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = _lib.load().smx_recon_compare_meshes(rec._h, None, C.byref(prm), ptr(a), C.c_uint32(n_a), ptr(b), C.c_uint32(n_b),
                                              C.c_int32(on_device), C.byref(st))
    return rc, st


def test_host_and_device_arrays_refusals_and_the_workspace(smx, world):
    from surfelmeshing_amd import _lib, api
    rec, meshes, m = world["rec"], world["meshes"], world["m"]
    a, b = meshes["fine"], meshes["coarse10"]
    n = m[0].shape[0]
    rows_before = rec.debug_download_surfels(n)
    prm = _lib.CompareParams(0.5, 0.0, N, SEED, 3)
    rc, host = _raw(rec, prm, a, a.shape[0], b, b.shape[0], 0)
    assert rc == 0
    da, db = smx.CUDABuffer(1, a.size, np.uint32), smx.CUDABuffer(1, b.size, np.uint32)
    da.Upload(a.reshape(1, -1))
    db.Upload(b.reshape(1, -1))
    rc, dev = _raw(rec, prm, da.ToCUDA().address, a.shape[0], db.ToCUDA().address, b.shape[0], 1)
    assert rc == 0 and bytes(dev) == bytes(host)
    assert da.Download()[0].tobytes() == a.tobytes() and db.Download()[0].tobytes() == b.tobytes()
    _same_side(api.compare_stats_dict(host, 0.5)["a_to_b"], world["model"]("fine", "coarse10", 0.5, 0.0), 0.0, "raw")
    zeros = bytes(C.sizeof(_lib.CompareStats))
    # a refusal by the distance half, by the sampling half, of the directions, of an index: `out` is zeroed
    for bad in (_lib.CompareParams(0.0, 0.0, N, SEED, 3), _lib.CompareParams(0.5, -1.0, N, SEED, 3), _lib.CompareParams(0.5, 0.0, (1 << 28) + 1, SEED, 3),
                _lib.CompareParams(0.5, 0.0, N, SEED, 0), _lib.CompareParams(0.5, 0.0, N, SEED, 4)):
        rc, st = _raw(rec, bad, a, a.shape[0], b, b.shape[0], 0)
        assert rc == -1 and bytes(st) == zeros
    wrong = b.copy()
    wrong[5, 1] = n
    for args in ((a, a.shape[0], wrong, wrong.shape[0]), (wrong, wrong.shape[0], a, a.shape[0])):
        rc, st = _raw(rec, prm, *args, 0)
        assert rc == -1 and bytes(st) == zeros
    # a failed allocation of the call's own workspace and of either half
    live = smx.DebugLiveAllocations()
    fresh = _rec_of(smx, m)
    try:
        for nth in (0, 6, 9):
            smx.DebugFailAllocation(nth)
            rc, st = _raw(fresh, prm, a, a.shape[0], b, b.shape[0], 0)
            assert rc == -2 and bytes(st) == zeros, nth
    finally:
        smx.DebugFailAllocation(-1)
    rc, st = _raw(fresh, prm, a, a.shape[0], b, b.shape[0], 0)
    assert rc == 0 and bytes(st) == bytes(host)
    fresh.close()
    assert smx.DebugLiveAllocations() == live
    for buf in (da, db):
        buf.close()
    # two calls give the same bytes, and the map is as it was
    rc, again = _raw(rec, prm, a, a.shape[0], b, b.shape[0], 0, fill=0)
    assert rc == 0 and bytes(again) == bytes(host)
    assert rec.debug_download_surfels(n).tobytes() == rows_before.tobytes()
