"""numpy restatement of smx_recon_track (frame-to-model point-to-plane ICP), written from the algorithm as include/smx.h
states it.  Test infrastructure.

The per-pixel part (vertex, transform, projection, gates, residual, Jacobian row, products) is evaluated in `dtype`
(float64 by default; float32 is "another legal rounding" of the same algorithm, used to measure how much rounding can
move a whole call); the sums, the solve and the pose update are float64 always.  T_rel is kept in float64 and handed to
an iteration as 12 float32 values, as the library does (`handover`; float64 there gives the algorithm without that
rounding, whose floor is float32 resolution at the scene's distance: a rounded rotation is not exactly rigid).  Like tests/depth_ref.py, an iteration reports how many pixels
sat within the float32 margin of a `floor` or a gate, i.e. whose decision a float32 evaluation may legitimately flip.
"""
import numpy as np

OK, CONVERGED, TOO_FEW_INLIERS, DEGENERATE, NOT_FINITE = range(5)
N_SUMS = 31
S_RR, S_INLIERS, S_PIXELS, S_ASSOCIATED = 27, 28, 29, 30
# Margins inside which a float32 evaluation may decide differently (eps = 2^-23 = 1.2e-7):
#  floor: u = fx p.x / p.z + cx.  p.x and p.z are sums of three products and a translation (6 roundings each, on terms no
#    larger than |p|), the quotient, the product with fx and the sum with cx add three more: |du| <= ~16 eps max(|u|, 1)
#    = 2e-6 relative -- a coordinate closer than that to an integer may land in the neighbouring pixel.
#  distance gate: d = p - q cancels to <= max_distance, its absolute error stays ~8 eps |p|; |d|^2 then moves by
#    2 max_distance 8 eps |p| = 6e-7 m^2 at |p| = 3 m and 10 cm, 6e-5 of max_distance^2: 1e-4 relative.
#  normal gate: a dot product of unit vectors, ~10 roundings on values <= 1: 1e-6 absolute; 1e-4 is generous.
FLOOR_MARGIN = 2e-6   # relative distance of a projected coordinate from an integer
GATE_MARGIN = 1e-4    # relative distance from a gate's threshold

f32 = np.float32
# Where track_pixel leaves a sample (the `code` of iteration's `detail`), in the order of its tests.
(EXIT_NO_DEPTH, EXIT_BEHIND, EXIT_LEFT, EXIT_RIGHT, EXIT_TOP, EXIT_BOTTOM, EXIT_HOLE, EXIT_DISTANCE, EXIT_ANGLE,
 EXIT_INLIER) = range(10)
EXITS = ("depth 0", "pz <= 0", "uf < 0", "uf >= W", "wf < 0", "wf >= H", "hole in D", "distance gate failed",
         "angle gate failed", "inlier")


class Params:
    """Mirror of smx_track_params with the defaults of smx_track_params_default()."""

    def __init__(self, levels=((4, 4), (2, 5), (1, 10)), max_distance=0.10, max_normal_angle_deg=30.0,
                 convergence_rotation=1e-5, convergence_translation=1e-5, min_inliers=50, min_inlier_fraction=0.1,
                 min_pivot_ratio=1e-6, near_z=0.05, far_z=20.0, disc_radius_factor=1.0, max_splat_extent_in_pixels=16.0):
        self.levels = tuple((int(s), int(n)) for s, n in levels)
        self.max_distance = float(f32(max_distance))
        self.max_normal_angle_deg = float(f32(max_normal_angle_deg))
        self.convergence_rotation = float(f32(convergence_rotation))
        self.convergence_translation = float(f32(convergence_translation))
        self.min_inliers = int(min_inliers)
        self.min_inlier_fraction = float(f32(min_inlier_fraction))
        self.min_pivot_ratio = float(f32(min_pivot_ratio))
        self.near_z, self.far_z = float(f32(near_z)), float(f32(far_z))
        self.disc_radius_factor = float(f32(disc_radius_factor))
        self.max_splat_extent_in_pixels = float(f32(max_splat_extent_in_pixels))

    def gates(self):
        """(max_distance^2, cos(max_normal_angle)) as the float32 values the kernel compares against."""
        with np.errstate(over="ignore"):    # (a max_distance whose square is no float any more gives +inf, as in the library)
            d2 = float(f32(self.max_distance) * f32(self.max_distance))
        return (d2, float(f32(np.cos(np.deg2rad(np.float64(self.max_normal_angle_deg))))))


IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(x, switch=1e-6):
    """exp of the twist x = (rotation, translation) as a 3 x 4: R = I + A K + B K^2, t = (I + B K + C K^2) u; the
    coefficients by their series below `switch` radians."""
    x = np.asarray(x, np.float64)
    w, u = x[:3], x[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < switch:
        A, B, Cc = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        sh = np.sin(0.5 * th)
        A, B, Cc = np.sin(th) / th, 2.0 * sh * sh / th2, (th - np.sin(th)) / (th2 * th)
    K = hat(w)
    K2 = K @ K
    R = np.eye(3) + A * K + B * K2
    V = np.eye(3) + B * K + Cc * K2
    return np.concatenate([R, (V @ u)[:, None]], axis=1)


def se3_mul(A, B):
    A, B = np.asarray(A, np.float64).reshape(3, 4), np.asarray(B, np.float64).reshape(3, 4)
    return np.concatenate([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]], axis=1)


def se3_inv(A):
    A = np.asarray(A, np.float64).reshape(3, 4)
    return np.concatenate([A[:, :3].T, (-A[:, :3].T @ A[:, 3])[:, None]], axis=1)


def rotation_vector_norm(R):
    """|log R| without arccos of the trace (which resolves nothing below 1e-8 rad): from the skew part, with the trace
    only deciding the quadrant."""
    R = np.asarray(R, np.float64)
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = 0.5 * (np.trace(R) - 1.0)
    return float(np.arctan2(s, c))


def pose_difference(A, B):
    """(translation distance, rotation angle in radians) between two 3 x 4 poses."""
    E = se3_mul(se3_inv(A), B)
    return float(np.linalg.norm(E[:, 3])), rotation_vector_norm(E[:, :3])


def iteration(D, M, depth, normals, intrinsics, T_rel, stride, gates, depth_scaling=5000.0, dtype=np.float64, handover=f32,
              detail=None, mutant=None):
    """One iteration's sums.  D [H, W] model depth (0 = empty), M [H, W, >=3] model normals, depth [H, W] uint16,
    normals [H, W, 2]; intrinsics (fx, fy, cx, cy); gates (max_distance^2, cos_max_angle).
    Returns (JtJ [6, 6], Jtr [6], sum r^2, inliers, pixels, margins) with margins a dict: `associated`, `flagged` (number
    of pixels with depth within FLOOR_MARGIN / GATE_MARGIN of a floor or a gate), `flagged_term` (the largest |J|^2 + |J r|
    + r^2 scale such a pixel can contribute) and `sums` (the 31 numbers in the library's order).
    For the exact model (tests/track_exact.py, which adds the terms in the launch's order): a dict given as `detail` receives
    the per-sample terms -- `n` samples in the kernel's index order, `code` [n] (EXITS: where track_pixel left), `clamped`
    [n] (the fmaxf of the frame normal's z took the 0), `index` (the samples with a geometric row), their `J` [k, 6] and
    `r` [k] in `dtype`, and `p` [n, 3] (NaN without depth); `mutant` flips one decision (tests/track_exact.py::MUTANTS)."""
    dt = dtype
    fx, fy, cx, cy = (dt(f32(v)) for v in intrinsics)
    H, W = depth.shape
    T = np.asarray(T_rel, np.float64).reshape(3, 4).astype(handover).astype(dt)
    maxd2, cosang = dt(gates[0]), dt(gates[1])
    ys, xs = np.mgrid[stride // 2:H:stride, stride // 2:W:stride]
    ys, xs = ys.ravel(), xs.ravel()
    du = depth[ys, xs]
    keep = du != 0
    ys, xs, du = ys[keep], xs[keep], du[keep]
    pixels = int(keep.sum())
    half = dt(0.5)
    z = du.astype(dt) / dt(f32(depth_scaling))
    vx = z * ((xs.astype(dt) + half - cx) / fx)
    vy = z * ((ys.astype(dt) + half - cy) / fy)
    nx, ny = normals[ys, xs, 0].astype(dt), normals[ys, xs, 1].astype(dt)
    nz = -np.sqrt(np.maximum(dt(0), dt(1) - nx * nx - ny * ny))
    px = T[0, 0] * vx + T[0, 1] * vy + T[0, 2] * z + T[0, 3]
    py = T[1, 0] * vx + T[1, 1] * vy + T[1, 2] * z + T[1, 3]
    pz = T[2, 0] * vx + T[2, 1] * vy + T[2, 2] * z + T[2, 3]
    flagged = np.zeros(len(z), bool)
    alive = pz > 0
    a_pz = alive.copy()
    flagged |= np.abs(pz) < FLOOR_MARGIN * z
    with np.errstate(divide="ignore", invalid="ignore"):
        uu = fx * px / pz + cx
        ww = fy * py / pz + cy
    to_pixel = np.rint if mutant == "rint" else np.floor
    uf, wf = to_pixel(uu), to_pixel(ww)

    def near_integer(a):
        with np.errstate(invalid="ignore"):
            return np.abs(a - np.rint(a)) < FLOOR_MARGIN * np.maximum(np.abs(a), 1.0)
    flagged |= alive & (near_integer(uu) | near_integer(ww))
    with np.errstate(invalid="ignore"):
        alive &= (uf >= 0) & (uf < W) & (wf >= 0) & (wf < H)
    a_in = alive.copy()
    ui = np.where(alive, uf, 0).astype(np.int64)
    wi = np.where(alive, wf, 0).astype(np.int64)
    Dq = np.asarray(D)[wi, ui].astype(dt)
    alive &= Dq > 0
    a_as = alive.copy()
    associated = int(alive.sum())
    Mq = np.asarray(M)[wi, ui, :3].astype(dt)
    qx = Dq * ((uf + half - cx) / fx)
    qy = Dq * ((wf + half - cy) / fy)
    with np.errstate(invalid="ignore"):
        dx, dy, dz = px - qx, py - qy, pz - Dq
        d2 = dx * dx + dy * dy + dz * dz
        flagged |= alive & (np.abs(d2 - maxd2) < GATE_MARGIN * maxd2)
        alive &= (d2 < maxd2) if mutant == "distance_lt" else (d2 <= maxd2)
        a_di = alive.copy()
        mx = T[0, 0] * nx + T[0, 1] * ny + T[0, 2] * nz
        my = T[1, 0] * nx + T[1, 1] * ny + T[1, 2] * nz
        mz = T[2, 0] * nx + T[2, 1] * ny + T[2, 2] * nz
        dot = mx * Mq[:, 0] + my * Mq[:, 1] + mz * Mq[:, 2]
        flagged |= alive & (np.abs(dot - cosang) < GATE_MARGIN)
        alive &= (dot > cosang) if mutant == "angle_gt" else (dot >= cosang)
    a = np.nonzero(alive)[0]
    if detail is not None:
        with np.errstate(invalid="ignore"):
            side = np.where(~(uf >= 0), EXIT_LEFT, np.where(~(uf < W), EXIT_RIGHT, np.where(~(wf >= 0), EXIT_TOP, EXIT_BOTTOM)))
        code = np.where(~a_pz, EXIT_BEHIND, np.where(~a_in, side, np.where(~a_as, EXIT_HOLE, np.where(
            ~a_di, EXIT_DISTANCE, np.where(~alive, EXIT_ANGLE, EXIT_INLIER)))))
        at = np.nonzero(keep)[0]
        detail["n"] = len(keep)
        detail["code"] = np.full(len(keep), EXIT_NO_DEPTH, np.int64)
        detail["code"][at] = code
        detail["clamped"] = np.zeros(len(keep), bool)
        detail["clamped"][at] = (dt(1) - nx * nx - ny * ny) < 0
        detail["index"] = at[a]
        detail["p"] = np.full((len(keep), 3), np.nan)
        detail["p"][at] = np.stack([px, py, pz], axis=1)
    px, py, pz, dx, dy, dz, Mq = px[a], py[a], pz[a], dx[a], dy[a], dz[a], Mq[a]
    r = Mq[:, 0] * dx + Mq[:, 1] * dy + Mq[:, 2] * dz
    J = np.stack([py * Mq[:, 2] - pz * Mq[:, 1], pz * Mq[:, 0] - px * Mq[:, 2], px * Mq[:, 1] - py * Mq[:, 0],
                  Mq[:, 0], Mq[:, 1], Mq[:, 2]], axis=1)
    if detail is not None:
        detail["J"], detail["r"] = J, r
    JtJ = np.zeros((6, 6))
    sums = np.zeros(N_SUMS)
    e = 0
    for i in range(6):
        for j in range(i, 6):
            v = float((J[:, i] * J[:, j]).astype(np.float64).sum())   # products in dtype, sums in float64
            JtJ[i, j] = JtJ[j, i] = v
            sums[e] = v
            e += 1
    Jtr = np.array([float((J[:, i] * r).astype(np.float64).sum()) for i in range(6)])
    rr = float((r * r).astype(np.float64).sum())
    sums[21:27], sums[S_RR], sums[S_INLIERS], sums[S_PIXELS], sums[S_ASSOCIATED] = Jtr, rr, len(a), pixels, associated
    # the most one flipped pixel can add to an entry: |J| <= max(|p|, 1), |r| <= max_distance
    pmax = float(np.sqrt((px.astype(np.float64) ** 2 + py.astype(np.float64) ** 2 + pz.astype(np.float64) ** 2).max())) if len(a) else 0.0
    margins = {"associated": associated, "flagged": int(flagged.sum()), "flagged_term": max(pmax, 1.0) ** 2,
               "sums": sums, "p_max": pmax}
    return JtJ, Jtr, rr, int(len(a)), pixels, margins


def solve(sums, T_rel, params, handover=f32):
    """(status, x [6], new T_rel) from an iteration's 31 sums, by the status rules of smx.h; T_rel unchanged and x zero
    where nothing is solved."""
    x = np.zeros(6)
    T_rel = np.asarray(T_rel, np.float64).reshape(3, 4)
    if not np.all(np.isfinite(sums)):
        return NOT_FINITE, x, T_rel
    if sums[S_PIXELS] > 0 and sums[S_ASSOCIATED] == 0:
        return DEGENERATE, x, T_rel
    if sums[S_INLIERS] < params.min_inliers:
        return TOO_FEW_INLIERS, x, T_rel
    A = np.zeros((6, 6))
    e = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[e]
            e += 1
    b = -np.asarray(sums[21:27], np.float64)
    max_diag = max(A[i, i] for i in range(6))
    L, d = np.zeros((6, 6)), np.zeros(6)
    for j in range(6):
        dj = A[j, j] - sum(L[j, m] * L[j, m] * d[m] for m in range(j))
        if not (dj >= params.min_pivot_ratio * max_diag) or not (dj > 0):
            return DEGENERATE, x, T_rel
        d[j] = dj
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - sum(L[i, m] * L[j, m] * d[m] for m in range(j))) / dj
    y = np.zeros(6)
    for i in range(6):
        y[i] = b[i] - sum(L[i, m] * y[m] for m in range(i))
    sol = np.zeros(6)
    for i in range(5, -1, -1):
        sol[i] = y[i] / d[i] - sum(L[m, i] * sol[m] for m in range(i + 1, 6))
    if not np.all(np.isfinite(sol)):
        return NOT_FINITE, x, T_rel
    # (the twist corrects the pose the iteration linearised at: T_rel as the 12 float32 values it was handed)
    Tn = se3_mul(se3_exp(sol), T_rel.astype(handover).astype(np.float64))
    if not np.all(np.isfinite(Tn)):
        return NOT_FINITE, x, T_rel
    conv = (np.linalg.norm(sol[:3]) < params.convergence_rotation and
            np.linalg.norm(sol[3:]) < params.convergence_translation)
    return (CONVERGED if conv else OK), sol, Tn


def track(D, M, depth, normals, intrinsics, params=None, depth_scaling=5000.0, dtype=np.float64, T_start=None,
          handover=f32):
    """The whole call on given model images.  Returns dict: T_rel (3 x 4 float64), status, iterations_run, records (one
    dict per iteration run: level, stride, status, sums, x, flagged, flagged_term), inliers / pixels of the last iteration,
    flagged (sum over the iterations)."""
    params = params or Params()
    T = IDENTITY.copy() if T_start is None else np.asarray(T_start, np.float64).reshape(3, 4).copy()
    T_prev = T.copy()
    status, records, converged_level = OK, [], -1
    gates = params.gates()
    for level, (stride, iters) in enumerate(params.levels):
        for _ in range(iters):
            if status >= TOO_FEW_INLIERS or converged_level == level:
                break   # (a bad status is sticky; a converged level skips its remaining iterations, the next one runs)
            _, _, _, _, _, mg = iteration(D, M, depth, normals, intrinsics, T, stride, gates, depth_scaling, dtype,
                                          handover)
            status, x, Tn = solve(mg["sums"], T, params, handover)
            records.append({"level": level, "stride": stride, "status": status, "sums": mg["sums"], "x": x,
                            "flagged": mg["flagged"], "flagged_term": mg["flagged_term"]})
            if status < TOO_FEW_INLIERS:
                T_prev, T = T, Tn
            if status == CONVERGED:
                converged_level = level
    last = records[-1] if records else None
    if last is not None and status < TOO_FEW_INLIERS and \
            last["sums"][S_INLIERS] < params.min_inlier_fraction * last["sums"][S_PIXELS]:
        status, T = TOO_FEW_INLIERS, T_prev
    return {"T_rel": T, "status": status, "iterations_run": len(records), "records": records,
            "inliers": int(last["sums"][S_INLIERS]) if last else 0, "pixels": int(last["sums"][S_PIXELS]) if last else 0,
            "rms": float(np.sqrt(last["sums"][S_RR] / last["sums"][S_INLIERS])) if last and last["sums"][S_INLIERS] > 0 else 0.0,
            "flagged": sum(r["flagged"] for r in records)}


def model_images(rows, n, render, width, height, fx, fy, cx, cy, global_T_pred, params=None):
    """(D float32 [H, W], M float32 [H, W, 4]) of a map given as reference-order rows, by the render restatement
    `render` (tests/viz_ref.render), rounded to float as the library hands them out: the normal of the winning slot
    rotated into the prediction's camera frame with float32 products, left-to-right adds."""
    params = params or Params()
    ref = render(rows, n, width, height, fx, fy, cx, cy, global_T_pred, near_z=params.near_z, far_z=params.far_z, mode=1,
                 disc_factor=params.disc_radius_factor, max_extent=params.max_splat_extent_in_pixels)
    D = ref["depth"].astype(f32)
    idx = ref["index"]
    empty = idx == 0xFFFFFFFF
    sl = np.where(empty, 0, idx).astype(np.int64)
    R = np.asarray(global_T_pred, f32).reshape(3, 4)[:, :3]
    nr = rows[8:11][:, sl].astype(f32)          # [3, H, W]
    M = np.zeros((height, width, 4), f32)
    for k in range(3):   # n_c[k] = sum_i R[i, k] n[i]  (R^T n)
        M[..., k] = ((R[0, k] * nr[0]).astype(f32) + (R[1, k] * nr[1]).astype(f32)).astype(f32) + (R[2, k] * nr[2]).astype(f32)
    M[empty] = 0
    return D, M
