"""How many record gathers of the neighbour update can change a link?  (CPU only, oracle alone.)

The bench's regime at a reduced size: a synthetic room stream, yaw 2 deg/frame, grown over a full turn, then the start of
the trajectory re-traversed under new frame indices.  For every re-traversal frame the lane tests of
update_neighbors_body (smx_recon.hip) are evaluated in numpy (update_gather_cases.lane_tests) on the rows the oracle's integration left behind, and for the
lanes that reach the gathers the candidates are counted that are a surfel, not the lane's slot and not yet one of its links.

    python tests/tools/update_gather_census.py [width height [turn_frames [frames]]]  > profiles/r11_update_gather_census.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as orc                                   # noqa: E402
from common import small_pre, small_stream             # noqa: E402
from oracle_pipeline import OraclePipeline             # noqa: E402
from update_gather_cases import lane_tests             # noqa: E402

INVALID = 0xFFFFFFFF


def lanes(before, after, n_before, frame, pose, cam, depth, radius, supporting, p, inv_scaling, W, H):
    """(reaches the gathers [n_before], candidates to evaluate per lane [n_before]); the lane tests themselves are
    update_gather_cases.lane_tests, the restatement the tests use."""
    ok, cand = lane_tests(after[:, :n_before], frame, pose, cam, p, depth, inv_scaling, radius, supporting, W, H)
    links = before[19:23, :n_before].view(np.uint32).copy()
    replaced = after[17, :n_before].view(np.uint32) == np.uint32(frame)   # (a replaced surfel's links were reset by the integration)
    links[:, replaced & (before[17, :n_before].view(np.uint32) != np.uint32(frame))] = INVALID
    idx = np.arange(n_before, dtype=np.uint32)
    n_eval = np.zeros(n_before, np.int64)
    for d in range(4):
        n_eval += (cand[d] != INVALID) & (cand[d] != idx) & (cand[d] != links).all(0)
    return ok, n_eval


def main():
    W = int(sys.argv[1]) if len(sys.argv) > 1 else 160
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 120
    turn = int(sys.argv[3]) if len(sys.argv) > 3 else 180
    frames = int(sys.argv[4]) if len(sys.argv) > 4 else 40
    s = small_stream(W, H, yaw_deg_per_frame=2.0, obstacle_until=-1)
    pre = small_pre(W)
    params = orc.IntegrateParams.defaults()
    po = OraclePipeline(W, H, s.fx, s.fy, s.cx, s.cy, 400000, pre, params)
    cam = (s.fx, s.fy, s.cx, s.cy)

    def step(logical, pose_index, count):
        for o in range(pose_index - 4, pose_index + 5):
            lf = logical + (o - pose_index)
            if lf not in po.raw_depth:
                po.upload(lf, *s.frame(o))
        po.release(logical - 6)
        others = [logical + (o - pose_index) for o in s.outlier_frames(pose_index)]
        po.preprocess(logical, others, s.others_TR_reference(pose_index))
        n_before = po.recon.surfels_size
        before = po.recon.surfels()[:, :n_before].copy() if count else None
        po.integrate(logical, s.pose(pose_index))
        if not count:
            return None
        ok, n_eval = lanes(before, po.recon.surfels(), n_before, logical, s.pose(pose_index), cam, po.depth_final, po.radius,
                           po.recon.scratch()["supporting"], params, 1.0 / pre.depth_scaling, W, H)
        return ok, n_eval

    for f in range(4, 4 + turn):
        step(f, f, False)
    first = 4 + turn + 10
    for f in list(po.raw_depth):
        po.release(f)
    settle = 34                                   # (past the regulariser window, like the bench's untimed frames)
    tot_lanes = tot_zero = tot_eval = 0
    hist = np.zeros(5, np.int64)
    print("# %d x %d, grown over %d frames to %d slots (%d merged); re-traversal, %d frames after %d settle frames" %
          (W, H, turn, po.recon.surfels_size, po.recon.merge_count, frames, settle))
    for j in range(settle + frames):
        r = step(first + j, 4 + j, j >= settle)
        if r is None:
            continue
        ok, n_eval = r
        tot_lanes += int(ok.sum())
        tot_zero += int((ok & (n_eval == 0)).sum())
        tot_eval += int(n_eval[ok].sum())
        hist += np.bincount(n_eval[ok], minlength=5)[:5]
    zero_share, mean_eval = tot_zero / tot_lanes, tot_eval / tot_lanes
    print("lanes reaching the gathers, per frame          %.0f" % (tot_lanes / frames))
    print("share of them with no candidate to evaluate    %.4f" % zero_share)
    print("candidates to evaluate per lane, mean          %.4f" % mean_eval)
    print("lanes by candidates to evaluate (0..4)         %s" % " ".join("%.4f" % (h / tot_lanes) for h in hist))
    print("record gathers per lane: 12 -> 4 x %.4f + 2 x %.4f = %.3f (%.1f %% saved)" %
          (1 - zero_share, mean_eval, 4 * (1 - zero_share) + 2 * mean_eval,
           100 * (1 - (4 * (1 - zero_share) + 2 * mean_eval) / 12)))


if __name__ == "__main__":
    main()
