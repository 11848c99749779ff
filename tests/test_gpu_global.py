"""smx_distscene_score_poses and smx_distscene_register_global on the device, against the exact model of tests/global_ref.py.
Every word of every smx_pose_score is compared for EQUALITY with the model (its words recorded in
tests/golden/global_bracket.npz, which tests/test_global_model.py holds to the model); the counts are cross-checked against the
registration's own sums; the whole search against the model's choice of starts, against Register from every start byte for
byte, against ScorePoses of the poses it returns, and against the TRUE pose within the tolerance measured on the CPU model."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dr
import global_ref as gr
import mesh_ref as mr
import register_ref as rr
import track_ref as tr
from test_global_model import BRACKET_MODEL_ROTATION, BRACKET_MODEL_TRANSLATION

pytestmark = pytest.mark.gpu

CAM = (160, 120, 131.25, 131.25, 80.0, 60.0)
GUARD = 0xA5
U = 2.0 ** -24


def _rec_of(smx, m, spare=1000):
    rows = mr.rows_of_map(*m)
    rec = smx.CUDASurfelReconstruction(rows.shape[1] + spare, smx.PinholeCamera4f(*CAM))
    rec.debug_upload_surfels(rows, int(np.sum(m[2] < 0)))
    return rec


@pytest.fixture(scope="module")
def scenes(smx):
    """(mesh name, bound) -> a scene: the world at both builds, its hand-made triangles alone, the bracket with its rim."""
    pos, nrm, r2, tri, info = dr.world()
    rec = _rec_of(smx, (pos, nrm, r2))
    bp, bn, br, bt = gr.bracket()
    brec = _rec_of(smx, (bp, bn, br))
    out = {}
    for bound, cell in rr.BUILDS:
        out["world", bound] = rec.BuildDistanceScene(None, tri, bound, cell)
    out["hand", gr.BRACKET_BOUND] = rec.BuildDistanceScene(None, tri[info["hand_tri"]:], gr.BRACKET_BOUND, gr.BRACKET_CELL)
    out["bracket", gr.BRACKET_BOUND] = brec.BuildDistanceScene(None, bt, gr.BRACKET_BOUND, gr.BRACKET_CELL, rim=True)
    out["bracket, no rim", gr.BRACKET_BOUND] = brec.BuildDistanceScene(None, bt, gr.BRACKET_BOUND, gr.BRACKET_CELL)
    rec.close()            # (a scene is a snapshot: the maps may go)
    brec.close()
    yield out
    for sc in out.values():
        sc.close()


def _same(got, want, what):
    for word in ("cost", "n_ok", "n_matched", "n_rim", "reserved"):
        differ = np.flatnonzero(got[word] != want[word])
        assert differ.size == 0, (what, word, differ[:5], got[word][differ[:5]], want[word][differ[:5]])


def _score(smx, scene, c, q, poses=None):
    from surfelmeshing_amd import api
    return scene.ScorePoses(None, c["points"], c["poses"] if poses is None else poses, api.score_params(c["stride"], q, c["rim"]))


@pytest.mark.parametrize("bound", [b for b, _ in rr.BUILDS])
@pytest.mark.parametrize("stride", [1, 3])
def test_the_base_set_under_the_k1_lattice_equals_the_model(smx, scenes, stride, bound):
    name = "base set, k = 1 about its pose, stride %d" % stride
    c = gr.cases()[name]
    got = _score(smx, scenes["world", bound], c, bound)
    want = gr.golden_case(name, bound)
    print("%s bound %g: n_ok %d .. %d, n_matched %d .. %d, cost %d .. %d" % (name, bound, got["n_ok"].min(), got["n_ok"].max(), got["n_matched"].min(),
                                                                           got["n_matched"].max(), got["cost"].min(), got["cost"].max()))
    _same(got, want, (name, bound))
    m = -(-257 // stride)
    assert np.all(got["n_ok"] < m) and np.any(got["n_matched"] < got["n_ok"]), "BAD and unmatched samples are met"
    # q = 0 is the scene's bound
    _same(_score(smx, scenes["world", bound], c, 0.0), want, (name, "q = 0"))


@pytest.mark.parametrize("chunk", [None, 1000, 1])
@pytest.mark.parametrize("rim", [False, True])
def test_the_bracket_under_the_k2_lattice_equals_the_model_at_every_chunking(smx, scenes, rim, chunk):
    """272 poses of 64 samples: one chunk; chunks of 15 poses (272 = 18 x 15 + 2); one pose per chunk."""
    name = "bracket, k = 2, stride 4" + (", rim rejected" if rim else "")
    c = gr.cases()[name]
    scene = scenes["bracket", gr.BRACKET_BOUND]
    scene.debug_set_score_chunk(chunk if chunk is not None else 1 << 22)
    try:
        got = _score(smx, scene, c, gr.BRACKET_BOUND)
    finally:
        scene.debug_set_score_chunk(1 << 22)
    _same(got, gr.golden_case(name, gr.BRACKET_BOUND), (name, chunk))
    assert (int(got["n_rim"].sum()) > 0) == rim


def test_one_pose_and_no_points(smx, scenes):
    name = "bracket, one pose"
    c = gr.cases()[name]
    scene = scenes["bracket", gr.BRACKET_BOUND]
    _same(_score(smx, scene, c, gr.BRACKET_BOUND), gr.golden_case(name, gr.BRACKET_BOUND), name)
    none = scene.ScorePoses(None, np.zeros((0, 3), np.float32), c["poses"])
    assert none.shape == (1,) and none.tobytes() == bytes(24)


def test_the_counts_are_the_registrations_own_sums(smx, scenes):
    """n_ok and n_matched against sums [29] and [30] of iteration 0 of Register from the same pose at the same stride and gate;
    n_rim against sum [31] of the robust call with reject_rim: code that existed before this one."""
    from surfelmeshing_amd import meshing
    for name, key, q in (("base set, k = 1 about its pose, stride 3", ("world", 0.02), 0.02), ("bracket, k = 2, stride 4, rim rejected", ("bracket", gr.BRACKET_BOUND), gr.BRACKET_BOUND)):
        c, scene = gr.cases()[name], scenes[key]
        got = _score(smx, scene, c, q)
        prm = meshing.register_params(levels=[(c["stride"], 1, q)], min_inliers=1)
        robust = meshing.register_robust_params(reject_rim=True) if c["rim"] else None
        identity = gr.quaternions(1 if c["mesh"] == "world" else 2).tolist().index([1 if c["mesh"] == "world" else 2, 0, 0, 0])
        for i in (0, 7, identity, 21, 33, c["poses"].shape[0] - 1):
            scene.Register(None, c["points"], None, c["poses"][i], prm, robust=robust)
            sums = scene.RegisterIterations()[0]["sums"]
            assert (got["n_ok"][i], got["n_matched"][i]) == (sums[29], sums[30]), (name, i, got[i], sums[29], sums[30])
            if c["rim"]:
                assert got["n_rim"][i] == scene.RegisterRobustCounts()[0][0], (name, i)


def test_two_calls_and_a_call_after_the_map_is_gone_give_the_same_bytes(smx):
    import torch
    from surfelmeshing_amd import api
    bp, bn, br, bt = gr.bracket()
    rec = _rec_of(smx, (bp, bn, br))
    c = gr.cases()["bracket, k = 2, stride 4, rim rejected"]
    sp = api.score_params(4, 0.0, True)
    with rec.BuildDistanceScene(None, bt, gr.BRACKET_BOUND, gr.BRACKET_CELL, rim=True) as scene:
        first = scene.ScorePoses(None, c["points"], c["poses"], sp)
        _same(first, gr.golden_case("bracket, k = 2, stride 4, rim rejected", gr.BRACKET_BOUND), "first")
        assert scene.ScorePoses(None, c["points"], c["poses"], sp).tobytes() == first.tobytes()
        # a registration in between uses the same query workspace; device points
        scene.Register(None, c["points"], None, c["poses"][3])
        tp = torch.from_numpy(np.ascontiguousarray(c["points"]).copy()).cuda()
        assert scene.ScorePoses(None, tp, c["poses"], sp).tobytes() == first.tobytes()
        assert tp.cpu().numpy().tobytes() == c["points"].tobytes()
        moved_r2 = br.copy()
        moved_r2[::3] = -1.0
        rec.debug_upload_surfels(mr.rows_of_map(bp + np.array([0.004, -0.003, 0.002]), bn, moved_r2), int(np.sum(moved_r2 < 0)))
        assert scene.ScorePoses(None, c["points"], c["poses"], sp).tobytes() == first.tobytes(), "after the upload"
        rec.close()
        assert scene.ScorePoses(None, c["points"], c["poses"], sp).tobytes() == first.tobytes(), "after the reconstruction is gone"
        t = scene.debug_global_timings()
        assert set(t) == {"score", "move", "query", "score_kernel", "select", "refine", "rescore"} and all(np.isfinite(v) and v >= 0 for v in t.values())
        assert t["score"] > 0 and t["query"] > 0 and t["score"] >= t["move"] + t["query"] + t["score_kernel"] and t["refine"] == 0


def _raw_score(scene, sp, pts, poses, out, n=None, P=None):
    """The C call itself; returns its code.  out: a numpy byte array."""
    from surfelmeshing_amd import _lib

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    n = n if n is not None else (0 if pts is None else pts.shape[0])
    P = P if P is not None else poses.size // 12
    return _lib.load().smx_distscene_score_poses(scene._h, None, C.byref(sp), ptr(pts), C.c_uint32(n), C.c_int32(0), ptr(poses), C.c_uint32(P), ptr(out))


def test_every_refusal_writes_nothing(smx, scenes):
    from surfelmeshing_amd import _lib
    c = gr.cases()["bracket, k = 2, stride 4"]
    pts, poses = np.ascontiguousarray(c["points"]), np.ascontiguousarray(c["poses"][:10])
    rim, plain = scenes["bracket", gr.BRACKET_BOUND], scenes["bracket, no rim", gr.BRACKET_BOUND]
    out = np.full(24 * 10, GUARD, np.uint8)
    untouched = lambda: bool(np.all(out == GUARD))                                    # noqa: E731
    sp = lambda stride=4, q=0.0, reject=0: _lib.ScoreParams(stride, q, reject)        # noqa: E731
    with smx.DistanceScene() as empty:
        assert _raw_score(empty, sp(), pts, poses, out) == -1 and untouched(), "an empty scene"
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        broken = poses.copy()
        broken.reshape(-1)[17 * k + 3] = bad
        assert _raw_score(rim, sp(), pts, broken, out) == -1 and untouched(), "a pose entry that is not finite"
    assert _raw_score(rim, sp(q=0.0500001), pts, poses, out) == -1 and untouched(), "q above the bound"
    assert _raw_score(rim, sp(q=0.0005), pts, poses, out) == -1 and untouched(), "q below 1e-3"
    assert _raw_score(rim, sp(q=float("nan")), pts, poses, out) == -1 and untouched()
    assert _raw_score(plain, sp(reject=1), pts, poses, out) == -1 and untouched(), "reject_rim on a scene without a rim"
    assert _raw_score(rim, sp(reject=2), pts, poses, out) == -1 and untouched()
    assert _raw_score(rim, sp(), None, poses, out, n=5) == -1 and untouched(), "points == NULL with n > 0"
    assert _raw_score(rim, sp(stride=0), pts, poses, out) == -1 and _raw_score(rim, sp(stride=65537), pts, poses, out) == -1 and untouched()
    assert _raw_score(rim, sp(), pts, poses, out, P=0) == -1 and _raw_score(rim, sp(), pts, poses, out, P=(1 << 20) + 1) == -1 and untouched()
    assert _raw_score(rim, sp(stride=1), np.zeros(((1 << 16) + 1, 3), np.float32), poses, out) == -1 and untouched(), "more than 2^16 samples"
    # scores overlapping an input: the poses, the host points
    both = np.zeros(24 * 10 + 48 * 10, np.uint8)
    both[:480] = poses.view(np.uint8).reshape(-1)
    before = both.copy()
    assert _raw_score(rim, sp(), pts, both[:480].view(np.float32), both[240:]) == -1 and np.array_equal(both, before)
    held = pts.copy()
    assert _raw_score(rim, sp(), held, poses, held.view(np.uint8).reshape(-1)[24:]) == -1 and held.tobytes() == pts.tobytes()
    assert _raw_score(rim, sp(), pts, poses, None) == -1
    # ... and the same call as it should be goes through
    assert _raw_score(rim, sp(), pts, poses, out) == 0 and not untouched()
    assert out.view(gr.SCORE_DTYPE).tobytes() == gr.golden_case("bracket, k = 2, stride 4", gr.BRACKET_BOUND)[:10].tobytes()
    with pytest.raises(ValueError):
        rim.ScorePoses(None, pts, poses * np.float32(np.nan))


def test_the_search_refuses_outputs_that_overlap_and_a_registration_it_cannot_run(smx, scenes):
    from surfelmeshing_amd import _lib, meshing
    scene = scenes["bracket", gr.BRACKET_BOUND]
    pts, nrm, _ = gr.bracket_points(1)
    pts, nrm, poses = np.ascontiguousarray(pts), np.ascontiguousarray(nrm), np.ascontiguousarray(gr.bracket_poses(1, 1))
    P = poses.shape[0]
    gp = _lib.GlobalParams(_lib.ScoreParams(4, 0.0, 0), 8, 0.5)
    room = np.full(C.sizeof(_lib.GlobalResult) + 24 * P, GUARD, np.uint8)          # the result, then room for the scores

    def call(prm, out_at, scores_at, gp=gp):
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                # noqa: E731
        return _lib.load().smx_distscene_register_global(
            scene._h, None, C.byref(gp), C.byref(prm), None, ptr(pts), ptr(nrm), C.c_uint32(pts.shape[0]), C.c_int32(0), ptr(poses), C.c_uint32(P),
            C.c_void_p(room.ctypes.data + out_at), None if scores_at is None else C.c_void_p(room.ctypes.data + scores_at))
    prm = meshing.register_params()
    size = C.sizeof(_lib.GlobalResult)
    assert call(prm, 0, size - 8) == -1 and np.all(room == GUARD), "all_scores reaches into out"
    assert call(prm, 24, 0) == -1 and np.all(room == GUARD), "out reaches into all_scores"
    # what the registration refuses is found by its first call, after the scores: still nothing written
    assert call(meshing.register_params(levels=[(1, 2, 0.06)]), 0, size) == -1 and np.all(room == GUARD), "a level's gate above the bound"
    assert call(prm, 0, size, _lib.GlobalParams(_lib.ScoreParams(4, 0.0, 0), 65, 0.5)) == -1 and np.all(room == GUARD), "65 starts"
    assert call(prm, 0, size) == 0
    got = _lib.GlobalResult.from_buffer_copy(room[:size].tobytes())
    assert got.n_starts_run == 8 and room[size:].view(gr.SCORE_DTYPE).tobytes() == scene.ScorePoses(None, pts, poses, _lib.ScoreParams(4, 0.0, 0)).tobytes()


def test_a_failed_allocation_writes_nothing_and_leaks_nothing(smx):
    from surfelmeshing_amd import _lib
    base = smx.DebugLiveAllocations()
    bp, bn, br, bt = gr.bracket()
    rec = _rec_of(smx, (bp, bn, br))
    c = gr.cases()["bracket, k = 2, stride 4, rim rejected"]
    pts, poses = np.ascontiguousarray(c["points"]), np.ascontiguousarray(c["poses"])
    want = gr.golden_case("bracket, k = 2, stride 4, rim rejected", gr.BRACKET_BOUND)
    sp = _lib.ScoreParams(4, 0.0, 1)
    failed = []
    rec.BuildDistanceScene(None, bt, gr.BRACKET_BOUND, gr.BRACKET_CELL, rim=True).close()       # (the object's own workspace has grown)
    try:
        for nth in range(40):           # every allocation of a call, on a fresh scene each time
            without = smx.DebugLiveAllocations()
            scene = rec.BuildDistanceScene(None, bt, gr.BRACKET_BOUND, gr.BRACKET_CELL, rim=True)
            live = smx.DebugLiveAllocations()
            out = np.full(24 * poses.shape[0], GUARD, np.uint8)
            smx.DebugFailAllocation(nth)
            rc = _raw_score(scene, sp, pts, poses, out)
            smx.DebugFailAllocation(-1)
            if rc == 0:
                break
            failed.append(rc)
            assert rc == -2 and np.all(out == GUARD), nth
            assert smx.DebugLiveAllocations()[0] <= live[0] + nth, nth            # (what it got before the failure it keeps for the next call)
            assert scene.ScorePoses(None, pts, poses, sp).tobytes() == want.tobytes(), nth     # the next call succeeds
            scene.close()
            assert smx.DebugLiveAllocations() == without, nth                     # a closed scene has given everything back
        # the query's counters, keys, two sort pairs and its workspace; moved, nearest, distance, poses, scores; the staging
        assert rc == 0 and 12 <= len(failed) < 40, "the call reached %d allocations" % len(failed)
        assert out.view(gr.SCORE_DTYPE).tobytes() == want.tobytes()
    finally:
        smx.DebugFailAllocation(-1)
    scene.close()
    rec.close()
    assert smx.DebugLiveAllocations() == base


@pytest.mark.parametrize("seed", gr.BRACKET_SEEDS)
def test_the_bracket_is_found_from_nowhere(smx, scenes, seed):
    from surfelmeshing_amd import api, meshing
    scene = scenes["bracket", gr.BRACKET_BOUND]
    pts, nrm, T_true = gr.bracket_points(seed)
    poses = gr.bracket_poses(seed, 3)
    assert api.pose_lattice(3, gr.centre_of(pts), gr.bracket_anchor()).tobytes() == poses.tobytes()
    prm = meshing.register_params()
    out, scores = scene.RegisterGlobal(None, pts, nrm, poses, prm, n_starts=8, return_scores=True)
    t = scene.debug_global_timings()
    # step 1 and step 2: the model's words, the model's choice
    want = gr.golden_scores(seed)
    _same(scores, want, ("all scores", seed))
    order = gr.select(want["cost"], 8)
    M = out["n_starts_run"]
    assert M == 8 == len(out["starts"])
    assert [s["pose_index"] for s in out["starts"]] == order.tolist()
    assert [s["cost_before"] for s in out["starts"]] == want["cost"][order].tolist()
    # step 3: byte for byte Register from that pose
    results = {}
    for r in (0, M - 1, out["winner_rank"]):
        results[r] = scene.Register(None, pts, nrm, poses[order[r]], prm)
        assert (results[r]["status"], results[r]["iterations_run"]) == (out["starts"][r]["status"], out["starts"][r]["iterations_run"]), r
    win = out["winner_rank"]
    assert b"".join(np.asarray(out["result"][k]).tobytes() for k in sorted(out["result"])) == \
        b"".join(np.asarray(results[win][k]).tobytes() for k in sorted(results[win])), "the winner's result is Register's from its start"
    # smx_global_result carries the winner's smx_register_result only.  For ranks 0 and M - 1 the whole result is brought out by
    # the same call on that start's pose alone (P = 1: it is the one start and the winner): Register's bytes, and the figures the
    # search filed for that rank.
    for r in (0, M - 1):
        alone = scene.RegisterGlobal(None, pts, nrm, poses[order[r]][None], prm, n_starts=8)
        assert alone["n_starts_run"] == 1 and alone["winner_rank"] == 0 and alone["starts"][0]["pose_index"] == 0
        assert b"".join(np.asarray(alone["result"][k]).tobytes() for k in sorted(alone["result"])) == \
            b"".join(np.asarray(results[r][k]).tobytes() for k in sorted(results[r])), ("rank %d's result is Register's from its start" % r)
        assert {k: v for k, v in alone["starts"][0].items() if k != "pose_index"} == {k: v for k, v in out["starts"][r].items() if k != "pose_index"}, r
    # step 4: cost_after is ScorePoses of the poses returned (for the starts whose pose is at hand)
    ranks = sorted(results)
    again = scene.ScorePoses(None, pts, np.stack([results[r]["scene_T_points"] for r in ranks]))
    for r, s in zip(ranks, again):
        assert (out["starts"][r]["cost_after"], out["starts"][r]["n_matched_after"]) == (s["cost"], s["n_matched"]), r
    # step 5: the winner obeys the rule
    after = [(s["cost_after"], r) for r, s in enumerate(out["starts"])]
    assert win == min(after)[1]
    dt, dr_ = tr.pose_difference(out["result"]["scene_T_points"].astype(np.float64), T_true)
    print("seed %d: winner rank %d of %s, status %d, %.3g rad and %.3g m from the truth; cost %s -> %s; ms %s" % (
        seed, win, [s["pose_index"] for s in out["starts"]], out["result"]["status"], dr_, dt, [s["cost_before"] for s in out["starts"]],
        [s["cost_after"] for s in out["starts"]], {k: round(v, 3) for k, v in t.items()}))
    assert out["found"] == 1 and out["result"]["status"] in (tr.OK, tr.CONVERGED)
    # the device's chain is the model's within the registration tests' 4 U per pose entry, a metre from the origin: below the
    # margin of the CPU-measured constants
    assert dr_ <= 4 * BRACKET_MODEL_ROTATION and dt <= 4 * BRACKET_MODEL_TRANSLATION, (dr_, dt)
    assert t["score"] > 0 and t["refine"] > 0 and t["rescore"] > 0


def test_nothing_to_match_is_not_found_and_the_helper_takes_a_device_tensor(smx, scenes):
    import torch
    from surfelmeshing_amd import meshing
    pts, nrm, T_true = gr.bracket_points(2)
    # the hand-made triangles of the world, three metres away: nothing thrown, nothing found
    hand = scenes["hand", gr.BRACKET_BOUND]
    out = meshing.register_global(hand, pts, nrm, k=1, anchors=gr.bracket_anchor())
    assert out["found"] == 0 and out["n_starts_run"] == 8 and out["result"]["status"] >= tr.TOO_FEW_INLIERS, out
    # the helper on a device tensor: the same winner as the call on host arrays, the centre its own default
    scene = scenes["bracket", gr.BRACKET_BOUND]
    want = scene.RegisterGlobal(None, pts, nrm, gr.bracket_poses(2, 3))
    got = meshing.register_global(scene, torch.from_numpy(pts.copy()).cuda(), torch.from_numpy(nrm.copy()).cuda(), k=3, anchors=gr.bracket_anchor())
    assert got["found"] == 1 and got["winner_rank"] == want["winner_rank"] and got["starts"] == want["starts"]
    assert got["result"]["scene_T_points"].tobytes() == want["result"]["scene_T_points"].tobytes()
    with pytest.raises(ValueError):
        meshing.register_global(scene, pts, nrm)            # no anchors and no mesh
