"""The arithmetic of smx_track.hip without a GPU: smx_track.hpp holds the per-pixel work, the accumulation order, the solve
and the exponential as plain inline functions, so this test compiles them for the host with the project's
-ffp-contract=off, drives them the way k_track_reduce / k_track_solve do (one lane that visits every sampled pixel in index
order, so the cross-lane sums have nothing to add) and compares them with the float64 restatement of tests/track_ref.py on
the oracle's map -- the same comparison tests/test_gpu_track.py makes on the device, with the same derived bound.  The same
launches are then walked with the launch's own lanes, wavefronts, workgroups and slabs (tests/track_host.py, which holds the
host program) and must give the exact model's sums (tests/track_exact.py) bit for bit."""
import ctypes as C

import numpy as np

import track_exact as tx
import track_host
import track_ref as tr
import viz_ref as vr
from common import small_stream
from test_track_api import oracle_map
from track_host import host_reduce, ptr as _ptr

U = 2.0 ** -24


def _host_library(tmp_path):
    return track_host.host_library(tmp_path)


def _sum_bounds(inliers, flagged, B, max_distance):
    """The bound of tests/test_gpu_track.py::_sum_bounds (derived there)."""
    c = np.array([B, B, B, 1.0, 1.0, 1.0])
    out = np.zeros(28)
    e = 0
    for a in range(6):
        for b in range(a, 6):
            out[e] = inliers * 32 * U * c[a] * c[b] + 2 * flagged * c[a] * c[b]
            e += 1
    out[21:27] = inliers * 64 * U * B * c + 2 * flagged * c * max_distance
    out[27] = inliers * 64 * U * B * max_distance + 2 * flagged * max_distance ** 2
    return out


# Per stride: the inlier floor under which the comparison would mean little, the floor of photometric inliers (for
# tests/test_track_rgbd_kernel_host.py), and the min_inliers the solve is asked with.  Stride 8 leaves 20 x 15 samples of the
# 160x120 frame, a quarter of stride 4's, and the restatement finds 23 to 132 inliers among them: too few for the default
# min_inliers of 50, so stride 8 runs with the floors tests/test_gpu_track.py and tests/test_gpu_track_rgbd.py use for all
# their strides (min_inliers = 10, inliers >= min_inliers, photometric inliers > 0).
FLOORS = {1: (90, 20, 50), 2: (90, 20, 50), 4: (90, 20, 50), 8: (10, 0, 10)}


def test_kernel_arithmetic_on_the_host_matches_the_restatement(orc, tmp_path):
    L = _host_library(tmp_path)
    s = small_stream(yaw_deg_per_frame=2.0, obstacle_until=8)
    po = oracle_map(s)
    rows, n = po.recon.surfels(), po.recon.surfels_size
    D, M = tr.model_images(rows, n, vr.render, s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.pose(11))
    D, M = np.ascontiguousarray(D), np.ascontiguousarray(M)
    p = tr.Params()
    g2, ca = p.gates()
    intr = (s.fx, s.fy, s.cx, s.cy)
    for g in (12, 16):
        po.preprocess(g, [], None)
        depth = np.ascontiguousarray(po.depth_final, np.uint16)
        normals = np.ascontiguousarray(np.asarray(po.normals).reshape(s.height, s.width, 2), np.float32)
        T1 = tr.se3_exp([0.001, 0.027 * (g - 11), 0.0005, 0.003, -0.002, 0.004])
        for T in (tr.IDENTITY, T1):
            for stride in (1, 2, 4, 8):
                _, _, _, inl, pix, mg = tr.iteration(D, M, depth, normals, intr, T, stride, p.gates(), s.depth_scaling)
                Tf = np.ascontiguousarray(T, np.float32)
                slab = host_reduce(L, s, stride, (g2, ca), Tf, depth, normals, D, M)
                assert inl >= FLOORS[stride][0] and mg["flagged"] <= 0.01 * pix
                assert slab[tr.S_PIXELS] == pix
                assert abs(slab[tr.S_ASSOCIATED] - mg["associated"]) <= mg["flagged"]
                assert abs(slab[tr.S_INLIERS] - inl) <= mg["flagged"]
                bound = _sum_bounds(inl, mg["flagged"], max(mg["p_max"], 1.0), p.max_distance)
                assert np.all(np.abs(slab[:28] - mg["sums"][:28]) <= bound), (g, stride)
                # the same launch walked with its lanes, wavefronts, workgroups and slabs: the exact model's bits
                exact, _ = tx.exact_sums(D, M, depth, normals, intr, Tf, stride, p.gates(), s.depth_scaling)
                walked, grid = track_host.walk_reduce(L, D, M, depth, normals, intr, Tf, stride, p, s.depth_scaling)
                assert grid == tx.grid_of(tx.samples(s.width, stride) * tx.samples(s.height, stride))
                assert np.array_equal(walked.view(np.uint64), exact.view(np.uint64)), (g, stride)
                assert np.array_equal(slab[28:31], exact[28:31])
                # the solve: status, twist and new pose against the restatement's, from the same sums
                p.min_inliers = FLOORS[stride][2]
                status, x, Tn = tr.solve(mg["sums"], T, p)
                S = (C.c_double * 31)(*mg["sums"])
                xo, To = (C.c_double * 6)(), (C.c_double * 12)()
                got = L.host_solve(S, p.min_inliers, C.c_double(p.min_pivot_ratio), C.c_double(p.convergence_rotation),
                                   C.c_double(p.convergence_translation), _ptr(Tf), xo, To)
                assert got == status and status in (tr.OK, tr.CONVERGED)
                assert np.allclose(np.array(xo), x, rtol=1e-9, atol=1e-15)
                assert np.allclose(np.array(To).reshape(3, 4), Tn, rtol=0, atol=1e-14)
    # the statuses that need no image
    Tf = np.ascontiguousarray(tr.IDENTITY, np.float32)
    xo, To = (C.c_double * 6)(), (C.c_double * 12)()

    def status_of(sums):
        return L.host_solve((C.c_double * 31)(*sums), 50, C.c_double(1e-6), C.c_double(1e-5), C.c_double(1e-5), _ptr(Tf), xo, To)
    z = np.zeros(31)
    z[tr.S_PIXELS] = 100
    assert status_of(z) == tr.DEGENERATE            # pixels with depth, nothing associated: an empty render
    z[tr.S_ASSOCIATED] = 100
    assert status_of(z) == tr.TOO_FEW_INLIERS
    z[3] = np.nan
    assert status_of(z) == tr.NOT_FINITE
    assert np.all(np.array(xo) == 0)
