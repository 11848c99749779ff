"""The exact model of the tracking sums: what k_track_reduce / k_track_reduce_rgbd and k_track_solve must produce bit for bit,
and the whole call around them.  Test infrastructure; numpy, no GPU.

The per-sample terms are the float32 evaluation of tests/track_ref.py::iteration and its photometric twin in
tests/track_rgbd_ref.py (every operation of track_pixel is one correctly rounded float operation: -ffp-contract=off, float
`/` and sqrtf correctly rounded).  This file adds them in the order of the launch, restated from DESIGN.md 5c without looking
at the kernel's loops:

  * 256 lanes per workgroup, grid = clamp(ceil(n / 2048), 1, 256) workgroups for n samples;
  * lane t of workgroup b visits the samples i = 256 b + t + 256 grid j, j = 0, 1, ..., and adds their terms one after the
    other into its own doubles, starting from +0.0 -- a sample's geometric row first, then its photometric row;
  * per wavefront of 64 lanes v[l] += v[l + off] for off = 32, 16, ..., 1 (all lanes at once); lane 0 holds the result;
  * the four wavefronts are added in order, 0 + 1 + 2 + 3, and stored as the workgroup's slab at b * 32 doubles (31 used),
    b * 40 with the photometric term (33 used);
  * the slabs are added in index order starting from +0.0; the counts are integers.

The sequential parts are explicit loops over elementwise adds (np.sum / np.add.reduce are pairwise).  A sample without a term
adds +0.0, which leaves every bit of an accumulator that started at +0.0 (it can never hold -0.0).

`mutant` turns one decision of the model the other way (MUTANTS); tests/test_track_cases.py shows that each of them changes
the sums of a named case of tests/track_cases.py."""
import math

import numpy as np

import track_ref as tr
import track_rgbd_ref as trr

f32, f64 = np.float32, np.float64
BLOCK, WAVE, PER_LANE, MAX_SLABS = 256, 64, 8, 256
SLAB_STRIDE, SLAB_STRIDE_RGBD = 32, 40

MUTANTS = {
    "distance_lt": "d^2 < max_distance^2 ('<' for '<=')",
    "angle_gt": "n_f . n_m > cos(max angle) ('>' for '>=')",
    "gradient_gt": "|g|^2 > min_gradient^2",
    "intensity_lt": "|e| < max_intensity_difference",
    "rint": "the model pixel is rint(u), rint(w) instead of floor",
    "photo_angle": "a failed angle gate also stops the photometric term",
    "no_half": "L is expanded about the pixel's corner: uc - uf without the half",
    "slab32": "slab stride 32 used with colour: sum [32] of slab b lies under sum [0] of slab b + 1",
    "waves_reversed": "the four wavefronts added 3 + 2 + 1 + 0",
    "clamp255": "the grid clamped at 255 workgroups",
    "lanes_strided": "the shift tree adds lane l + 1, l + 2, l + 4, ... (offsets ascending)",
    "slabs_reversed": "the slabs added from the last to the first",
}

# photometric exits, behind tr.EXITS: where the photometric term of a sample that passed the distance gate ends
PHOTO_EXITS = ("P.w = 0", "gradient below min_gradient", "|e| above max_intensity_difference", "photometric inlier")


def grid_of(n, mutant=None):
    return int(min(max(-(-n // (BLOCK * PER_LANE)), 1), 255 if mutant == "clamp255" else MAX_SLABS))


def samples(size, stride):
    return len(range(stride // 2, size, stride))


def _rows(J, r, e):
    """The 28 doubles one row adds: the 21 float products of the upper triangle row by row, the 6 with r, e * e."""
    k = J.shape[0]
    out = np.zeros((k, 28), f64)
    c = 0
    for a in range(6):
        for b in range(a, 6):
            out[:, c] = (J[:, a] * J[:, b]).astype(f64)
            c += 1
    for a in range(6):
        out[:, 21 + a] = (J[:, a] * r).astype(f64)
    out[:, 27] = (e * e).astype(f64)
    return out


def launch_sum(n, geo_index, geo_rows, photo_index, photo_rows, counts, photo, mutant=None):
    """The 31 / 33 sums of one launch over n samples: geo_rows [k, 28] belong to the samples geo_index, photo_rows likewise
    (column 27 is e * e, which has its own accumulator); counts [n, 4] of 0 / 1: inliers, pixels, associated, photometric
    inliers."""
    grid = grid_of(n, mutant)
    lanes = BLOCK * grid
    visits = -(-n // lanes) if n else 0
    acc = np.zeros((lanes, 29), f64)          # [28] = sum e^2 of the photometric term
    for j in range(visits):                   # a lane's samples one after the other
        g = np.zeros((lanes, 28), f64)
        sel = geo_index // lanes == j
        g[geo_index[sel] % lanes] = geo_rows[sel]
        acc[:, :28] += g
        if photo:
            p = np.zeros((lanes, 28), f64)
            sel = photo_index // lanes == j
            p[photo_index[sel] % lanes] = photo_rows[sel]
            acc[:, :27] += p[:, :27]
            acc[:, 28] += p[:, 27]
    v = acc.reshape(grid, BLOCK // WAVE, WAVE, 29)
    if mutant == "lanes_strided":
        while v.shape[2] > 1:
            v = v[:, :, 0::2] + v[:, :, 1::2]
    else:
        off = WAVE // 2
        while off:                            # lanes l < off take lane l + off; lane 0 ends with the wavefront's sum
            v = v[:, :, :off] + v[:, :, off:2 * off]
            off //= 2
    part = v[:, :, 0]                         # [grid, 4, 29]
    order = (3, 2, 1, 0) if mutant == "waves_reversed" else (0, 1, 2, 3)
    group = part[:, order[0]].copy()
    for w in order[1:]:
        group = group + part[:, w]
    cnt = np.zeros((grid, 4), np.int64)
    padded = np.zeros((visits * lanes, 4), np.int64)
    padded[:n] = counts
    if visits:
        cnt = padded.reshape(visits, grid, BLOCK, 4).sum(axis=(0, 2))
    n_sums = trr.N_SUMS if photo else tr.N_SUMS
    slab = np.zeros((grid, n_sums), f64)
    slab[:, :28] = group[:, :28]
    slab[:, tr.S_INLIERS], slab[:, tr.S_PIXELS], slab[:, tr.S_ASSOCIATED] = cnt[:, 0], cnt[:, 1], cnt[:, 2]
    if photo:
        slab[:, trr.S_EE], slab[:, trr.S_PHOTO_INLIERS] = group[:, 28], cnt[:, 3]
    # the slabs in memory, stored workgroup after workgroup, and read back at the same stride
    stride = SLAB_STRIDE_RGBD if photo and mutant != "slab32" else SLAB_STRIDE
    mem = np.zeros(MAX_SLABS * SLAB_STRIDE_RGBD + n_sums, f64)
    for b in range(grid):
        mem[b * stride:b * stride + n_sums] = slab[b]
    total = np.zeros(n_sums, f64)
    for b in (range(grid - 1, -1, -1) if mutant == "slabs_reversed" else range(grid)):
        total = total + mem[b * stride:b * stride + n_sums]
    return total


def exact_sums(D, M, depth, normals, intrinsics, Tf, stride, gates, depth_scaling, photo=None, mutant=None):
    """(sums, census codes) of one iteration from the pose Tf (12 float32 values): sums float64 [31], or [33] with photo =
    (P, colour, parameters: a track_rgbd_ref.Params).  codes = {"geo": [n] of tr.EXITS, "clamped": [n], "photo": [n] of
    PHOTO_EXITS or -1 where the term is not reached}."""
    H, W = depth.shape
    n = samples(W, stride) * samples(H, stride)
    Tf = np.asarray(Tf, f32).reshape(3, 4)
    ref_mutant = mutant if mutant in ("distance_lt", "angle_gt", "rint") else None
    with np.errstate(all="ignore"):
        dg = {}
        tr.iteration(D, M, depth, normals, intrinsics, Tf, stride, gates, depth_scaling, f32, f32, dg, ref_mutant)
        assert dg["n"] == n
        geo_rows = _rows(dg["J"], dg["r"], dg["r"])
        counts = np.zeros((n, 4), np.int64)
        code = dg["code"]
        counts[:, 0] = code == tr.EXIT_INLIER
        counts[:, 1] = code != tr.EXIT_NO_DEPTH
        counts[:, 2] = code >= tr.EXIT_DISTANCE
        codes = {"geo": code, "clamped": dg["clamped"], "photo": np.full(n, -1, np.int64), "p": dg["p"]}
        photo_index, photo_rows = np.zeros(0, np.int64), np.zeros((0, 28))
        if photo is not None:
            P, color, params = photo
            dp = {}
            photo_mutant = mutant if mutant in ("distance_lt", "rint", "gradient_gt", "intensity_lt", "no_half") else None
            trr.photometric(D, P, depth, color, intrinsics, Tf, stride, params, depth_scaling, f32, f32, dp, photo_mutant)
            assert np.array_equal(dp["reached"], np.nonzero(code >= tr.EXIT_ANGLE)[0])
            inl = dp["inlier"]
            if mutant == "photo_angle":
                inl = inl & (code[dp["reached"]] == tr.EXIT_INLIER)
                keep = code[dp["index"]] == tr.EXIT_INLIER
                dp["index"], dp["K"], dp["se"], dp["e"] = dp["index"][keep], dp["K"][keep], dp["se"][keep], dp["e"][keep]
            photo_index, photo_rows = dp["index"], _rows(dp["K"], dp["se"], dp["e"])
            counts[dp["index"], 3] = 1
            codes["photo"][dp["reached"]] = np.where(~dp["valid"], 0, np.where(~dp["gradient"], 1, np.where(~dp["intensity"], 2, 3)))
            assert np.array_equal(codes["photo"][dp["reached"]] == 3, inl) or mutant == "photo_angle"
        sums = launch_sum(n, dg["index"], geo_rows, photo_index, photo_rows, counts, photo is not None, mutant)
    return sums, codes


# ---- the solve's surroundings, in the operation order of smx_track.hpp ----
def se3_exp(x):
    """track_ref.se3_exp with the products and sums in the order of the header's loops (sin is the C library's)."""
    wx, wy, wz = (float(v) for v in x[:3])
    th2 = wx * wx + wy * wy + wz * wz
    th = math.sqrt(th2)
    if th < 1e-6:
        A, B, Cc = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        sh = math.sin(0.5 * th)
        A, B, Cc = math.sin(th) / th, 2.0 * sh * sh / th2, (th - math.sin(th)) / (th2 * th)
    K = [0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0]
    K2 = [K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j] for i in range(3) for j in range(3)]
    E = np.zeros((3, 4))
    for i in range(3):
        t = 0.0
        for j in range(3):
            ident = 1.0 if i == j else 0.0
            E[i, j] = ident + A * K[3 * i + j] + B * K2[3 * i + j]
            t += (ident + B * K[3 * i + j] + Cc * K2[3 * i + j]) * float(x[3 + j])
        E[i, 3] = t
    return E


def se3_mul(A, B):
    A, B = np.asarray(A, f64).reshape(12), np.asarray(B, f64).reshape(12)
    out = np.zeros(12)
    for i in range(3):
        for j in range(4):
            v = float(A[4 * i]) * float(B[j]) + float(A[4 * i + 1]) * float(B[4 + j]) + float(A[4 * i + 2]) * float(B[8 + j])
            if j == 3:
                v += float(A[4 * i + 3])
            out[4 * i + j] = v
    return out.reshape(3, 4)


def next_pose(x, Tf):
    """T_rel (float64) after the update x of an iteration that read the 12 floats Tf."""
    return se3_mul(se3_exp(x), np.asarray(Tf, f32).astype(f64))


def exact_call(D, M, depth, normals, intrinsics, pred, params, depth_scaling, photo=None, recorded_x=None, Tf_start=None):
    """The whole call on given model images.  params: track_ref.Params (track_rgbd_ref.Params with photo = (P, colour)).
    recorded_x: the update of every iteration as the implementation under test recorded it (double sin is not specified to
    the bit, so the poses follow the recorded twists; the restatement's own solve, returned as `x_ref`, is compared with a
    tolerance by the caller) -- without, the restatement's own.  Returns a dict: records (level, stride, status, sums, x,
    x_ref, Tf, codes), status, iterations_run, T_rel, global_T_frame float32 [3, 4], inliers, pixels_with_depth, rms_residual,
    last_update_rotation, last_update_translation, information float32 [6, 6], photometric_inliers,
    rms_intensity_residual."""
    with_photo = photo is not None and params.photometric_weight != 0
    ph = (photo[0], photo[1], params) if with_photo else None
    T = tr.IDENTITY.copy() if Tf_start is None else np.asarray(Tf_start, f32).astype(f64).reshape(3, 4)
    T_prev = T.copy()
    status, records, converged_level = tr.OK, [], -1
    for level, (stride, iters) in enumerate(params.levels):
        for _ in range(iters):
            if status >= tr.TOO_FEW_INLIERS or converged_level == level:
                break
            Tf = T.astype(f32)
            sums, codes = exact_sums(D, M, depth, normals, intrinsics, Tf, stride, params.gates(), depth_scaling, ph)
            st, x_ref, _ = (trr.solve if with_photo else tr.solve)(sums, T, params)
            x = x_ref
            if recorded_x is not None and len(records) < len(recorded_x):
                x = np.asarray(recorded_x[len(records)], f64)
            if st < tr.TOO_FEW_INLIERS:
                # (the decision between OK and CONVERGED is taken from the recorded twist as well)
                conv = math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) < params.convergence_rotation and \
                    math.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]) < params.convergence_translation
                st = tr.CONVERGED if conv else tr.OK
                T_prev, T = T, next_pose(x, Tf)
            status = st
            full = np.zeros(trr.N_SUMS)
            full[:len(sums)] = sums
            records.append({"level": level, "stride": stride, "status": st, "sums": full, "x": x, "x_ref": x_ref, "Tf": Tf,
                            "codes": codes})
            if st == tr.CONVERGED:
                converged_level = level
    last = records[-1] if records else None
    if last is not None and status < tr.TOO_FEW_INLIERS and \
            last["sums"][tr.S_INLIERS] < params.min_inlier_fraction * last["sums"][tr.S_PIXELS]:
        status, T = tr.TOO_FEW_INLIERS, T_prev
    pred64 = np.asarray(pred, f32).astype(f64).reshape(3, 4)
    G = pred64 if np.array_equal(T, tr.IDENTITY) else se3_mul(pred64, T)
    s = last["sums"] if last else np.zeros(trr.N_SUMS)
    x = last["x"] if last else np.zeros(6)
    info = np.zeros((6, 6), f32)
    e = 0
    for i in range(6):
        for j in range(i, 6):
            info[i, j] = info[j, i] = f32(s[e])
            e += 1
    return {"records": records, "status": status, "iterations_run": len(records), "T_rel": T, "global_T_frame": G.astype(f32),
            "inliers": int(s[tr.S_INLIERS]), "pixels_with_depth": int(s[tr.S_PIXELS]),
            "rms_residual": f32(math.sqrt(s[tr.S_RR] / s[tr.S_INLIERS])) if s[tr.S_INLIERS] > 0 else f32(0),
            "last_update_rotation": f32(math.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])),
            "last_update_translation": f32(math.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])),
            "information": info, "photometric_inliers": int(s[trr.S_PHOTO_INLIERS]),
            "rms_intensity_residual": f32(math.sqrt(s[trr.S_EE] / s[trr.S_PHOTO_INLIERS])) if s[trr.S_PHOTO_INLIERS] > 0 else f32(0)}
