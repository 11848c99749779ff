"""The arithmetic of the kernels of smx_recon_track_rgbd without a GPU, in the manner of tests/test_track_kernel_host.py and
through its host library: track_photo_pixel, track_pixel<true> and the solve with colour, the inline functions of
smx_track.hpp that k_track_photo_prepare, k_track_reduce_rgbd and k_track_solve call.  The prepare output must equal the
float32 restatement of tests/track_rgbd_ref.py bit for bit; the 33 sums stay within the bound derived there and in
tests/test_gpu_track.py -- the comparison tests/test_gpu_track_rgbd.py makes on the device -- and, walked in the launch's
order (tests/track_host.py), equal the exact model's (tests/track_exact.py) bit for bit."""
import ctypes as C

import numpy as np

import track_exact as tx
import track_host
import track_ref as tr
import track_rgbd_ref as trr
import viz_ref as vr
from common import small_stream
from test_track_api import oracle_map
from test_track_kernel_host import FLOORS, _host_library, _ptr, _sum_bounds, host_reduce
from test_track_rgbd_api import frame_color


def test_rgbd_kernel_arithmetic_on_the_host_matches_the_restatement(orc, tmp_path):
    from surfelmeshing_amd._lib import TrackRGBDIteration, TrackRGBDResult
    L = _host_library(tmp_path)
    s = small_stream(yaw_deg_per_frame=2.0, obstacle_until=8)
    po = oracle_map(s)
    rows, n = po.recon.surfels(), po.recon.surfels_size
    p = trr.Params()
    D, M, Cm, P = trr.model_images(rows, n, vr.render, s.width, s.height, s.fx, s.fy, s.cx, s.cy, s.pose(11), p)
    D, M, Cm = np.ascontiguousarray(D), np.ascontiguousarray(M), np.ascontiguousarray(Cm)
    # the prepare kernel: bit for bit, on a map with empty pixels and depth steps
    got = np.full((s.height, s.width, 4), 7.0, np.float32)
    L.host_prepare(s.width, s.height, C.c_float(p.gradient_max_relative_depth_step), _ptr(D), _ptr(Cm), _ptr(got))
    assert np.array_equal(got.view(np.uint32), P.view(np.uint32))
    valid = P[..., 3] != 0
    assert (~valid[1:-1, 1:-1] & (D[1:-1, 1:-1] > 0)).sum() > 50 and valid.sum() > 0.3 * valid.size
    P = np.ascontiguousarray(P)
    g2, ca = p.gates()
    intr = (s.fx, s.fy, s.cx, s.cy)
    for g in (12, 16):
        po.preprocess(g, [], None)
        depth = np.ascontiguousarray(po.depth_final, np.uint16)
        normals = np.ascontiguousarray(np.asarray(po.normals).reshape(s.height, s.width, 2), np.float32)
        color = frame_color(s, g)
        T1 = tr.se3_exp([0.001, 0.027 * (g - 11), 0.0005, 0.003, -0.002, 0.004])
        for T in (tr.IDENTITY, T1):
            for stride in (8, 1, 2, 4):   # (4 last: the checks after the loops go on from its slabs)
                Tf = np.ascontiguousarray(T, np.float32)

                def reduce(weight, photo):
                    return host_reduce(L, s, stride, (g2, ca), Tf, depth, normals, D, M,
                                       (weight, p.max_intensity_difference, p.min_gradient_sq(), color, P if photo else None))
                want, mg = trr.iteration(D, M, P, depth, normals, color, intr, T, stride, p, s.depth_scaling)
                slab = reduce(p.photometric_weight, True)
                pix, fl = want[tr.S_PIXELS], mg["flagged"]
                assert fl <= 0.01 * pix and slab[tr.S_PIXELS] == pix and mg["photo"]["inliers"] > FLOORS[stride][1]
                assert want[tr.S_INLIERS] >= FLOORS[stride][2]
                for e in (tr.S_ASSOCIATED, tr.S_INLIERS, trr.S_PHOTO_INLIERS):
                    assert abs(slab[e] - want[e]) <= fl, (g, stride, e)
                diff, bound = trr.compare_sums(slab, want, mg, p, _sum_bounds)
                assert np.all(diff <= bound), (g, stride, int(np.argmax(diff / bound)), float((diff / bound).max()))
                # the same launch walked with its lanes, wavefronts, workgroups and slabs: the exact model's bits, all 33
                exact, _ = tx.exact_sums(D, M, depth, normals, intr, Tf, stride, p.gates(), s.depth_scaling, (P, color, p))
                walked, _ = track_host.walk_reduce(L, D, M, depth, normals, intr, Tf, stride, p, s.depth_scaling, (P, color))
                assert np.array_equal(walked.view(np.uint64), exact.view(np.uint64)), (g, stride)
                assert np.array_equal(slab[28:31], exact[28:31]) and slab[32] == exact[32]
                # the term is there: the same bound would not cover leaving it out
                geo = reduce(0.0, False)
                assert np.all(geo[31:33] == 0) and np.any(np.abs(geo[:28] - want[:28]) > bound[:28])
                # the solve: status, twist, record and result from the kernel's own sums against the restatement's solve
                p.min_inliers = FLOORS[stride][2]
                status, x, Tn = trr.solve(slab[:33], T, p)
                rec, res = TrackRGBDIteration(), TrackRGBDResult()
                st = L.host_solve_rgbd(_ptr(slab), p.min_inliers, C.c_double(p.min_pivot_ratio),
                                       C.c_double(p.convergence_rotation), C.c_double(p.convergence_translation), _ptr(Tf),
                                       C.byref(rec), C.byref(res))
                assert st == status == rec.status == res.icp.status and status in (tr.OK, tr.CONVERGED)
                assert np.array_equal(np.array(rec.sums), slab[:33])
                assert np.allclose(np.array(rec.x), x, rtol=1e-9, atol=1e-15)
                assert np.allclose(np.array(res.icp.global_T_frame).reshape(3, 4), Tn, rtol=0, atol=1e-6)
                assert res.photometric_inliers == slab[32] and res.icp.inliers == slab[tr.S_INLIERS]
                assert abs(res.rms_intensity_residual - np.sqrt(slab[31] / slab[32])) < 1e-6
    # weight 0 (the kernel without the term) leaves the geometric sums: the restatement's, within the geometric bound alone
    _, _, _, inl, pix, mg0 = tr.iteration(D, M, depth, normals, intr, T1, 4, p.gates(), s.depth_scaling)
    assert np.all(np.abs(geo[:28] - mg0["sums"][:28]) <= _sum_bounds(inl, mg0["flagged"], max(mg0["p_max"], 1.0), p.max_distance))
    # a non-finite photometric sum is NOT_FINITE before anything is solved
    bad = slab.copy()
    bad[31] = np.nan
    rec, res = TrackRGBDIteration(), TrackRGBDResult()
    assert L.host_solve_rgbd(_ptr(bad), 50, C.c_double(1e-6), C.c_double(1e-5), C.c_double(1e-5), _ptr(Tf), C.byref(rec),
                             C.byref(res)) == tr.NOT_FINITE
    assert np.all(np.array(rec.x) == 0) and res.icp.status == tr.NOT_FINITE
