"""numpy restatement of smx_recon_track_rgbd (point-to-plane ICP plus a photometric term), written from the algorithm as
include/smx.h states it.  Test infrastructure; the geometric part IS tests/track_ref.py (iteration, solve), so that a
weight of 0 gives tests/track_ref.track exactly.

`prepare` is float32 throughout and restates k_track_photo_prepare bit for bit (every operation of it is a single IEEE
float operation; the build has -ffp-contract=off).  The photometric per-pixel part of an iteration is evaluated in `dtype`
like the geometric one, the sums are float64.  Pixels near one of the new decisions are flagged as in track_ref:
  |e| near max_intensity_difference: e = L + gx du + gy dw - I_f; L, gx, gy, I_f are exact inputs, du = uc - (u + 1/2)
    carries uc's error, FLOOR_MARGIN max(|uc|, 1) (track_ref), so |de| <= FLOOR_MARGIN (|gx| max(|uc|, 1) + |gy| max(|wc|,
    1)) + 4 eps: the margin used, per pixel (`e_error` below);
  gradient magnitude near min_gradient: gx^2 + gy^2 of exact inputs, three roundings: GATE_MARGIN relative is generous;
  a depth step near its limit (prepare only, reported for information: prepare is compared bit for bit).
"""
import numpy as np

import track_ref as tr
from track_ref import FLOOR_MARGIN, GATE_MARGIN, f32

N_SUMS = 33
S_EE, S_PHOTO_INLIERS = 31, 32
EPS = float(np.finfo(np.float32).eps)


class Params(tr.Params):
    """Mirror of smx_track_rgbd_params with the defaults of smx_track_rgbd_params_default()."""

    def __init__(self, photometric_weight=0.1, max_intensity_difference=0.2, min_gradient=0.02,
                 gradient_max_relative_depth_step=0.02, **kw):
        tr.Params.__init__(self, **kw)
        self.photometric_weight = float(f32(photometric_weight))
        self.max_intensity_difference = float(f32(max_intensity_difference))
        self.min_gradient = float(f32(min_gradient))
        self.gradient_max_relative_depth_step = float(f32(gradient_max_relative_depth_step))

    def min_gradient_sq(self):
        return float(f32(self.min_gradient) * f32(self.min_gradient))


def luma(r, g, b):
    """((0.299f r + 0.587f g) + 0.114f b) (1.0f / 255.0f) in float32, left to right."""
    r, g, b = (np.asarray(v).astype(f32) for v in (r, g, b))
    return ((f32(0.299) * r + f32(0.587) * g) + f32(0.114) * b) * (f32(1.0) / f32(255.0))


def luma_u32(c):
    c = np.asarray(c, np.uint32)
    return luma(c & 255, (c >> 8) & 255, (c >> 16) & 255)


def model_color(rows, index):
    """The colour render with color_flags = 0 from the index render: the colour row's low 24 bits, alpha 255; 0 = empty."""
    idx = np.asarray(index)
    empty = idx == 0xFFFFFFFF
    col = np.ascontiguousarray(rows[24]).view(np.uint32)[np.where(empty, 0, idx).astype(np.int64)]
    return np.where(empty, 0, (col & 0x00FFFFFF) | 0xFF000000).astype(np.uint32)


def prepare(D, C, max_relative_depth_step, with_flags=False):
    """P [H, W, 4] float32 = (L, gx, gy, valid) from the model depth D [H, W] float32 and colour C [H, W] uint32."""
    D = np.asarray(D, f32)
    H, W = D.shape
    L = luma_u32(C)
    P = np.zeros((H, W, 4), f32)
    P[..., 0] = L
    d = D[1:-1, 1:-1]
    nb = (D[1:-1, :-2], D[1:-1, 2:], D[:-2, 1:-1], D[2:, 1:-1])
    lim = f32(max_relative_depth_step) * d
    ok = d > 0
    near = np.zeros_like(ok)
    for q in nb:
        step = np.abs(q - d)
        ok = ok & (q > 0) & (step <= lim)
        near |= (d > 0) & (q > 0) & (np.abs(step.astype(np.float64) - lim) < GATE_MARGIN * lim)
    gx = f32(0.5) * (L[1:-1, 2:] - L[1:-1, :-2])
    gy = f32(0.5) * (L[2:, 1:-1] - L[:-2, 1:-1])
    P[1:-1, 1:-1, 1] = np.where(ok, gx, f32(0))
    P[1:-1, 1:-1, 2] = np.where(ok, gy, f32(0))
    P[1:-1, 1:-1, 3] = ok.astype(f32)
    if with_flags:
        return P, int(near.sum())
    return P


def photometric(D, P, depth, color, intrinsics, T_rel, stride, params, depth_scaling=5000.0, dtype=np.float64,
                handover=f32, detail=None, mutant=None):
    """The photometric sums of one iteration: dict with `JtJ` [21] (upper triangle, row by row), `Jtr` [6], `ee`,
    `inliers`, `flagged` (pixels near a photometric gate that are not near a floor or the distance gate -- those
    track_ref.iteration counts already), `k_rot` / `k_tra` (largest |K| entry, rotational / translational, over the
    candidate pixels), `e_error` (largest error bound of e over the inliers).
    As in track_ref.iteration, a dict given as `detail` receives the per-sample terms for the exact model: `reached` (the
    samples, in the kernel's index order, that pass the distance gate and so reach the term), per reached sample `valid`
    (P.w != 0), `gradient` and `intensity` (those two gates alone), `inlier`, and per inlier `index`, `K` [k, 6], `se`
    (weight e) and `e` in `dtype`; `mutant` flips one decision (tests/track_exact.py::MUTANTS)."""
    dt = dtype
    fx, fy, cx, cy = (dt(f32(v)) for v in intrinsics)
    H, W = depth.shape
    T = np.asarray(T_rel, np.float64).reshape(3, 4).astype(handover).astype(dt)
    maxd2 = dt(params.gates()[0])
    lam, maxe, ming2 = dt(f32(params.photometric_weight)), dt(f32(params.max_intensity_difference)), dt(params.min_gradient_sq())
    ys, xs = np.mgrid[stride // 2:H:stride, stride // 2:W:stride]
    ys, xs = ys.ravel(), xs.ravel()
    du = depth[ys, xs]
    keep = du != 0
    ys, xs, du = ys[keep], xs[keep], du[keep]
    half = dt(0.5)
    z = du.astype(dt) / dt(f32(depth_scaling))
    vx = z * ((xs.astype(dt) + half - cx) / fx)
    vy = z * ((ys.astype(dt) + half - cy) / fy)
    px = T[0, 0] * vx + T[0, 1] * vy + T[0, 2] * z + T[0, 3]
    py = T[1, 0] * vx + T[1, 1] * vy + T[1, 2] * z + T[1, 3]
    pz = T[2, 0] * vx + T[2, 1] * vy + T[2, 2] * z + T[2, 3]
    alive = pz > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        uu = fx * px / pz + cx
        ww = fy * py / pz + cy
        to_pixel = np.rint if mutant == "rint" else np.floor
        uf, wf = to_pixel(uu), to_pixel(ww)
        alive &= (uf >= 0) & (uf < W) & (wf >= 0) & (wf < H)

        def near_integer(a):
            return np.abs(a - np.rint(a)) < FLOOR_MARGIN * np.maximum(np.abs(a), 1.0)
        counted = (np.abs(pz) < FLOOR_MARGIN * z) | ((pz > 0) & (near_integer(uu) | near_integer(ww)))
    ui = np.where(alive, uf, 0).astype(np.int64)
    wi = np.where(alive, wf, 0).astype(np.int64)
    Dq = np.asarray(D)[wi, ui].astype(dt)
    alive &= Dq > 0
    qx = Dq * ((uf + half - cx) / fx)
    qy = Dq * ((wf + half - cy) / fy)
    with np.errstate(invalid="ignore"):
        dx, dy, dz = px - qx, py - qy, pz - Dq
        d2 = dx * dx + dy * dy + dz * dz
        counted |= alive & (np.abs(d2 - maxd2) < GATE_MARGIN * maxd2)
        alive &= (d2 < maxd2) if mutant == "distance_lt" else (d2 <= maxd2)
    a = np.nonzero(alive)[0]
    px, py, pz, uu, ww, uf, wf, counted = px[a], py[a], pz[a], uu[a], ww[a], uf[a], wf[a], counted[a]
    Pq = np.asarray(P)[wi[a], ui[a]].astype(dt)
    L, gx, gy, valid = Pq[:, 0], Pq[:, 1], Pq[:, 2], Pq[:, 3] != 0
    col = np.asarray(color)[ys[a], xs[a]]
    If = luma(col[:, 0], col[:, 1], col[:, 2]).astype(dt)
    centre = dt(0) if mutant == "no_half" else half
    Lm = (L + gx * (uu - (uf + centre))) + gy * (ww - (wf + centre))
    e = Lm - If
    g2 = gx * gx + gy * gy
    e_err = FLOOR_MARGIN * (np.abs(gx) * np.maximum(np.abs(uu), 1.0) + np.abs(gy) * np.maximum(np.abs(ww), 1.0)) + 4 * EPS
    flagged = valid & (g2 >= ming2 * (1 - GATE_MARGIN)) & (np.abs(np.abs(e) - maxe) < e_err)
    flagged |= valid & (np.abs(e) <= maxe + e_err) & (np.abs(g2 - ming2) < GATE_MARGIN * ming2)
    g_ok = (g2 > ming2) if mutant == "gradient_gt" else (g2 >= ming2)
    e_ok = (np.abs(e) < maxe) if mutant == "intensity_lt" else (np.abs(e) <= maxe)
    inl = valid & g_ok & e_ok
    if detail is not None:
        at = np.nonzero(keep)[0][a]
        detail.update(reached=at, valid=valid, gradient=g_ok, intensity=e_ok, inlier=inl, index=at[inl])
    gfx, gfy = gx * fx, gy * fy
    a0, a1, a2 = gfx / pz, gfy / pz, -((gfx * px + gfy * py) / (pz * pz))
    K = np.stack([lam * (py * a2 - pz * a1), lam * (pz * a0 - px * a2), lam * (px * a1 - py * a0),
                  lam * a0, lam * a1, lam * a2], axis=1)
    cand = valid    # (what a flipped pixel can contribute: any associated pixel with a gradient)
    k_rot = float(np.abs(K[cand, :3]).max()) if cand.any() else 0.0
    k_tra = float(np.abs(K[cand, 3:]).max()) if cand.any() else 0.0
    K, e, se = K[inl], e[inl], (lam * e)[inl]
    if detail is not None:
        detail.update(K=K, se=se, e=e)
    JtJ = np.array([float((K[:, i] * K[:, j]).astype(np.float64).sum()) for i in range(6) for j in range(i, 6)])
    Jtr = np.array([float((K[:, i] * se).astype(np.float64).sum()) for i in range(6)])
    return {"JtJ": JtJ, "Jtr": Jtr, "ee": float((e * e).astype(np.float64).sum()), "inliers": int(inl.sum()),
            "flagged": int((flagged & ~counted).sum()), "k_rot": k_rot, "k_tra": k_tra,
            "e_error": float(e_err[inl].max()) if inl.any() else 0.0}


def iteration(D, M, P, depth, normals, color, intrinsics, T_rel, stride, params, depth_scaling=5000.0, dtype=np.float64,
              handover=f32):
    """One iteration's 33 sums: (sums, margins) with margins = track_ref.iteration's dict (its `flagged` now counts the
    pixels near a photometric gate too) plus `photo` (the dict of `photometric`, None at weight 0)."""
    _, _, _, _, _, mg = tr.iteration(D, M, depth, normals, intrinsics, T_rel, stride, params.gates(), depth_scaling, dtype,
                                     handover)
    sums = np.zeros(N_SUMS)
    sums[:tr.N_SUMS] = mg["sums"]
    mg = dict(mg)
    mg["photo"] = None
    if params.photometric_weight != 0:
        ph = photometric(D, P, depth, color, intrinsics, T_rel, stride, params, depth_scaling, dtype, handover)
        sums[:21] += ph["JtJ"]
        sums[21:27] += ph["Jtr"]
        sums[S_EE], sums[S_PHOTO_INLIERS] = ph["ee"], ph["inliers"]
        mg["photo"] = ph
        mg["flagged"] = mg["flagged"] + ph["flagged"]
    mg["sums"] = sums
    return sums, mg


def solve(sums, T_rel, params, handover=f32):
    """track_ref.solve on the first 31 sums, behind the finiteness of the two others."""
    if not np.all(np.isfinite(sums[tr.N_SUMS:])):
        return tr.NOT_FINITE, np.zeros(6), np.asarray(T_rel, np.float64).reshape(3, 4)
    return tr.solve(sums[:tr.N_SUMS], T_rel, params, handover)


def track(D, M, P, depth, normals, color, intrinsics, params=None, depth_scaling=5000.0, dtype=np.float64, T_start=None,
          handover=f32):
    """The whole call on given model images: the loop of track_ref.track with the 33 sums.  Returns its dict plus
    photometric_inliers and rms_intensity of the last iteration."""
    params = params or Params()
    T = tr.IDENTITY.copy() if T_start is None else np.asarray(T_start, np.float64).reshape(3, 4).copy()
    T_prev = T.copy()
    status, records, converged_level = tr.OK, [], -1
    for level, (stride, iters) in enumerate(params.levels):
        for _ in range(iters):
            if status >= tr.TOO_FEW_INLIERS or converged_level == level:
                break
            sums, mg = iteration(D, M, P, depth, normals, color, intrinsics, T, stride, params, depth_scaling, dtype, handover)
            status, x, Tn = solve(sums, T, params, handover)
            records.append({"level": level, "stride": stride, "status": status, "sums": sums, "x": x,
                            "flagged": mg["flagged"], "flagged_term": mg["flagged_term"]})
            if status < tr.TOO_FEW_INLIERS:
                T_prev, T = T, Tn
            if status == tr.CONVERGED:
                converged_level = level
    last = records[-1] if records else None
    if last is not None and status < tr.TOO_FEW_INLIERS and \
            last["sums"][tr.S_INLIERS] < params.min_inlier_fraction * last["sums"][tr.S_PIXELS]:
        status, T = tr.TOO_FEW_INLIERS, T_prev
    ls = last["sums"] if last else np.zeros(N_SUMS)
    return {"T_rel": T, "status": status, "iterations_run": len(records), "records": records,
            "inliers": int(ls[tr.S_INLIERS]), "pixels": int(ls[tr.S_PIXELS]),
            "rms": float(np.sqrt(ls[tr.S_RR] / ls[tr.S_INLIERS])) if ls[tr.S_INLIERS] > 0 else 0.0,
            "photometric_inliers": int(ls[S_PHOTO_INLIERS]),
            "rms_intensity": float(np.sqrt(ls[S_EE] / ls[S_PHOTO_INLIERS])) if ls[S_PHOTO_INLIERS] > 0 else 0.0,
            "flagged": sum(r["flagged"] for r in records)}


def model_images(rows, n, render, width, height, fx, fy, cx, cy, global_T_pred, params=None):
    """(D, M, C, P): track_ref.model_images plus the colour render and P, as the library hands them out."""
    params = params or Params()
    D, M = tr.model_images(rows, n, render, width, height, fx, fy, cx, cy, global_T_pred, params)
    ref = render(rows, n, width, height, fx, fy, cx, cy, global_T_pred, near_z=params.near_z, far_z=params.far_z, mode=1,
                 disc_factor=params.disc_radius_factor, max_extent=params.max_splat_extent_in_pixels)
    Cm = model_color(rows, ref["index"])
    return D, M, Cm, prepare(D, Cm, params.gradient_max_relative_depth_step)


U = 2.0 ** -24


def photo_sum_bounds(ph, params, B):
    """Bound on |float32 evaluation - restatement| for what the photometric term adds to the 28 float sums and for sum
    e^2, derived.  With A = the largest |lambda a| entry (ph['k_tra']) and R = the largest |lambda p x a| entry (<= B A,
    ph['k_rot']), kc = (R, R, R, A, A, A) bounds |K_a|.  a's entries carry <= 4 roundings on exact gradients and p's 6
    (relative to B, track_ref), the cross product 3 more, the weight 1: |dK_a| <= 16 U max(kc_a, B A) =: kerr_a.  e carries
    ph['e_error'] =: De (see the module docstring).  A product adds one rounding.  Per photometric inlier:
      JtJ[a][b]: kerr_a kc_b + kc_a kerr_b + U kc_a kc_b
      Jtr[a]:    kerr_a lambda Emax + kc_a lambda De + 2 U kc_a lambda Emax       (Emax = max_intensity_difference)
      sum e^2:   2 Emax De + U Emax^2
    plus, for every flagged pixel, the largest term such a pixel can contribute (photo_flag_bounds).  Returns (bounds
    [28], bound of sum e^2, kc); the flagged part is NOT included."""
    R, A = max(ph["k_rot"], B * ph["k_tra"]), ph["k_tra"]
    kc = np.array([R, R, R, A, A, A])
    kerr = 16 * U * np.maximum(kc, B * A)
    lam, emax, de, n = params.photometric_weight, params.max_intensity_difference, ph["e_error"], ph["inliers"]
    out = np.zeros(28)
    e = 0
    for a in range(6):
        for b in range(a, 6):
            out[e] = n * (kerr[a] * kc[b] + kc[a] * kerr[b] + U * kc[a] * kc[b])
            e += 1
    out[21:27] = n * (kerr * lam * emax + kc * lam * de + 2 * U * kc * lam * emax)
    return out, n * (2 * emax * de + U * emax * emax), kc


def photo_flag_bounds(kc, params, flagged):
    """What `flagged` pixels near a decision may move the photometric part of the sums by: per pixel at most
    lambda^2 |J_I|^2 (kc_a kc_b entry by entry), lambda^2 |J_I| Emax (kc_a lambda Emax) and Emax^2.  (The geometric bound
    this is added to, tests/test_gpu_track.py::_sum_bounds, allows a flagged pixel twice its largest geometric term, because
    it may meet the neighbouring model pixel.)  Returns (bounds [28], bound of sum e^2).
    Where pixels are flagged, this term and its geometric counterpart dominate the whole bound -- one flipped pixel outweighs
    the rounding of thousands -- so the comparison of the sums would not show a moderate per-pixel error by itself: the sums
    measured on an MI355X reach 0.4 % of it.  What pins the kernels' arithmetic is P bit for bit, the photometric inlier
    counts (equal in every comparison) and the whole calls on the textured plane, held to a few 1e-6 m against this
    restatement."""
    lam, emax = params.photometric_weight, params.max_intensity_difference
    out = np.zeros(28)
    e = 0
    for a in range(6):
        for b in range(a, 6):
            out[e] = flagged * kc[a] * kc[b]
            e += 1
    out[21:27] = flagged * kc * lam * emax
    return out, flagged * emax * emax


def compare_sums(got, want, mg, params, geometric_bounds):
    """(|got - want| [29], bound [29]) for the 28 float sums and sum e^2 of one iteration: `geometric_bounds(inliers,
    flagged, B, max_distance)` (tests/test_gpu_track.py::_sum_bounds) plus the photometric bounds above."""
    ph, fl = mg["photo"], mg["flagged"]
    B = max(mg["p_max"], 1.0)
    b_photo, b_ee, kc = photo_sum_bounds(ph, params, B)
    f_photo, f_ee = photo_flag_bounds(kc, params, fl)
    bound = np.concatenate([geometric_bounds(want[tr.S_INLIERS], fl, B, params.max_distance) + b_photo + f_photo, [b_ee + f_ee]])
    diff = np.abs(np.concatenate([got[:28], [got[S_EE]]]) - np.concatenate([want[:28], [want[S_EE]]]))
    return diff, bound
