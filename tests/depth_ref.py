"""A float64 statement of each per-pixel preprocessing stage (test infrastructure, plain numpy).

Written from the definition of the operation -- weighted mean over the disc; reproject and compare; cross-product
normal and its angle to the viewing ray; largest and smallest neighbour distance -- not from the statement order of the
CPU oracle or of the kernels, and in float64 throughout.  The oracle and the HIP kernels share one author and one
float32 arithmetic contract; this is what can show them wrong together.

Every function returns, beside its result, what a float32 implementation is allowed to get differently: a per-pixel
margin for each threshold decision (the decision is only compared where the float64 quantity is farther than the
margin from its threshold) and a per-pixel error bound for each float result.  u = 2^-24 is the unit roundoff of float32
(relative error of one correctly rounded operation); the derivations stand next to the constants.

Conventions (the reference's): pixel-corner intrinsics, so pixel (x, y) looks along
((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1); u16 depth = depth_scaling x metres; reads outside the image give 0.
"""
import numpy as np

U = 2.0 ** -24


def bilateral_radius(sigma_xy, radius_factor):
    """The disc radius is part of the entry point's definition: (int)(radius_factor * sigma_xy + 0.5) in float32."""
    return int(np.float32(np.float32(radius_factor) * np.float32(sigma_xy)) + np.float32(0.5))


def _shifted(img, dy, dx, fill):
    """out[y, x] = img[y + dy, x + dx], `fill` outside."""
    h, w = img.shape
    out = np.full((h, w), fill, img.dtype)
    ys, yd = slice(max(0, dy), h + min(0, dy)), slice(max(0, -dy), h + min(0, -dy))
    xs, xd = slice(max(0, dx), w + min(0, dx)), slice(max(0, -dx), w + min(0, -dx))
    out[yd, xd] = img[ys, xs]
    return out


def bilateral(depth, sigma_xy, sigma_value_factor, value_to_ignore, radius_factor, max_depth, depth_valid_region_radius):
    """Bilateral filter with depth cutoff.  A pixel is valid if it lies within depth_valid_region_radius of the image
    centre (w // 2, h // 2), is not value_to_ignore and is at most max_depth.  Its result is the mean of the samples s
    of the disc |offset| <= radius that are inside the image and not value_to_ignore, weighted by
        exp(-|offset|^2 / (2 sigma_xy^2) - (s - c)^2 / (2 (sigma_value_factor c)^2)),   c the pixel's own depth,
    rounded to the nearest unit (floor(mean + 0.5)).  For c = 0 (possible when value_to_ignore is not 0) the depth
    sigma is 0: only samples equal to c have weight, the mean is c.

    Returns dict: valid [h,w] bool; value [h,w] float64 = mean + 0.5 before truncation (nan where invalid);
    taps [h,w] int = T, the samples in the disc; ignored_in_disc [h,w] bool; region_margin [h,w] bool (the centre
    distance is within float32 rounding of the region radius: validity is not compared there)."""
    d = np.asarray(depth).astype(np.float64)
    h, w = d.shape
    R = bilateral_radius(sigma_xy, radius_factor)
    sx, sv = float(np.float32(sigma_xy)), float(np.float32(sigma_value_factor))
    ys, xs = np.mgrid[0:h, 0:w]
    r2 = (xs - w // 2) ** 2.0 + (ys - h // 2) ** 2.0
    rr = float(np.float32(depth_valid_region_radius)) ** 2
    region_margin = np.abs(r2 - rr) <= 4 * U * rr + 0.0     # r2 is an exact integer; radius^2 is one float32 product
    ignore = d == float(value_to_ignore)
    valid = (r2 <= rr) & ~ignore & (d <= float(max_depth))
    num, den = np.zeros((h, w)), np.zeros((h, w))
    taps = np.zeros((h, w), np.int64)
    ign_in_disc = np.zeros((h, w), bool)
    sig_v = sv * d
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                g2 = dx * dx + dy * dy
                if g2 > R * R:
                    continue
                s = _shifted(d, dy, dx, -1.0)
                inside = s >= 0
                s_ign = inside & (s == float(value_to_ignore))
                use = inside & ~s_ign
                if g2 > 0:
                    ign_in_disc |= s_ign
                e = -g2 / (2.0 * sx * sx) - (s - d) ** 2 / (2.0 * sig_v * sig_v)
                wgt = np.where(use, np.exp(e), 0.0)
                wgt = np.where(use & (sig_v == 0), (s == d).astype(np.float64) * np.exp(-g2 / (2.0 * sx * sx)), wgt)
                num += wgt * np.where(use, s, 0.0)
                den += wgt
                taps += use
        value = np.where(valid, num / den + 0.5, np.nan)
    return dict(valid=valid, value=value, taps=taps, ignored_in_disc=ign_in_disc & valid, region_margin=region_margin,
                radius=R)


def bilateral_round_margin(ref, depth):
    """How far from an integer `value` may lie for a float32 implementation to truncate it differently:
    v (T + 8) 2^-23, v the centre depth, T the taps -- one rounding per product and per addition of the two sums
    (2 T roundings of relative size u = 2^-24 each, i.e. T 2^-23) plus the exponential's and the division's."""
    return np.asarray(depth).astype(np.float64) * (ref["taps"] + 8) * 2.0 ** -23


def _rays(h, w, fx, fy, cx, cy):
    ys, xs = np.mgrid[0:h, 0:w]
    return (xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy


def _point_error(z, fx, fy, cx, cy):
    """Bound on the float32 error of one unprojected point of depth z (length of the error vector), per pixel [h,w];
    it also covers the pixel's eight neighbours.  x = z (x_pix / fx + c), c = -(cx - 0.5) / fx, t = x_pix / fx + c:
    the roundings that differ from point to point are those of the depth (1 / depth_scaling x the u16: u z |t| in x),
    of the product x_pix (1 / fx) (u z |x_pix / fx|), of the sum (u z |t|) and of the final product (u z |t|); likewise y;
    z takes the first alone.  The three constants 1 / depth_scaling, 1 / fx and c are rounded once for the whole image:
    their errors move all points together and are accounted for where differences of points are formed
    (_COMMON_MODE)."""
    h, w = z.shape
    ys, xs = np.mgrid[0:h, 0:w]
    xf, yf = (xs + 1) / abs(fx), (ys + 1) / abs(fy)
    tx = np.abs((xs + 0.5 - cx) / fx) + 1 / abs(fx)
    ty = np.abs((ys + 0.5 - cy) / fy) + 1 / abs(fy)
    return U * z * np.sqrt((xf + 3 * tx) ** 2 + (yf + 3 * ty) ** 2 + 1.0)


# Error of a difference v of two neighbouring points beyond the two point errors, relative to |v|: the subtraction (1),
# the rounding of 1 / fx (it scales x_pix z / fx of both points: at most (1 + |x_pix / fx|) <= 3 for these cameras), of c
# (two roundings; it multiplies the depth difference: 2 |c| <= 2).  The rounding of 1 / depth_scaling scales every point
# alike: no effect on directions, 2 u on squared distances.
_COMMON_MODE = 6 * U


def outlier_cull(depth, others, T, fx, fy, cx, cy, tolerance, required_count):
    """Multi-frame outlier cull.  A pixel with depth d > 0 is the point X = d (ray); in neighbour k it is T_k X = (ox, oy,
    oz).  Neighbour k AGREES if oz > 0, the projection (fx ox / oz + cx, fy oy / oz + cy) truncates to a pixel of the
    image ((-1, 0) truncates to 0), and that pixel's depth od is not 0 and within (1 +- tolerance) oz.  The pixel is kept
    if all neighbours agree (required_count < 0) or at least required_count do.

    Three-valued: every comparison is made with a margin for float32 rounding (16 u relative to the magnitudes that
    enter it: eight or so operations each side), both candidate pixels are looked up where the projection is within the
    margin of a pixel boundary.  Returns (keep [h,w] bool, certain [h,w] bool)."""
    d = np.asarray(depth).astype(np.float64)
    h, w = d.shape
    tol = float(np.float32(tolerance))
    ys, xs = np.mgrid[0:h, 0:w]
    rxf, ryf = (xs - (cx - 0.5)) / fx, (ys - (cy - 0.5)) / fy
    X = np.stack([d * rxf, d * ryf, d], axis=-1)
    Xabs = np.abs(X)
    n = len(others)
    sure = np.zeros((h, w), np.int64)
    maybe = np.zeros((h, w), np.int64)
    rel = 16 * U
    for k in range(n):
        M = np.asarray(T[k], np.float64).reshape(3, 4)
        o = X @ M[:, :3].T + M[:, 3]
        oscale = Xabs @ np.abs(M[:, :3]).T + np.abs(M[:, 3])         # magnitudes that entered each sum
        oz, ez = o[..., 2], rel * oscale[..., 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = fx * o[..., 0] / oz + cx
            v = fy * o[..., 1] / oz + cy
            eu = rel * (fx * oscale[..., 0] / np.abs(oz) + abs(cx)) + fx * np.abs(o[..., 0]) * ez / (oz * oz)
            ev = rel * (fy * oscale[..., 1] / np.abs(oz) + abs(cy)) + fy * np.abs(o[..., 1]) * ez / (oz * oz)
        front_sure, front_maybe = oz > ez, oz > -ez
        u = np.where(front_maybe & np.isfinite(u), u, -5.0)
        v = np.where(front_maybe & np.isfinite(v), v, -5.0)
        eu = np.where(np.isfinite(eu), np.minimum(eu, 0.5), 0.5)
        ev = np.where(np.isfinite(ev), np.minimum(ev, 0.5), 0.5)
        img = np.asarray(others[k]).astype(np.float64)
        all_good, any_good = np.ones((h, w), bool), np.zeros((h, w), bool)
        for su in (-1, 1):
            for sv_ in (-1, 1):
                uu, vv = u + su * eu, v + sv_ * ev
                inside = (uu > -1) & (vv > -1) & (uu < w) & (vv < h)
                px = np.clip(np.trunc(uu).astype(np.int64), 0, w - 1)
                py = np.clip(np.trunc(vv).astype(np.int64), 0, h - 1)
                od = img[py, px]
                em = rel * od + (1 + tol) * ez
                strict = inside & (od != 0) & (od <= (1 + tol) * oz - em) & (od >= (1 - tol) * oz + em)
                loose = inside & (od != 0) & (od <= (1 + tol) * oz + em) & (od >= (1 - tol) * oz - em)
                all_good &= strict
                any_good |= loose
        sure += front_sure & all_good
        maybe += front_maybe & any_good
    need = n if required_count < 0 else required_count
    keep_lo, keep_hi = sure >= need, maybe >= need
    has = d > 0
    return keep_hi & has, (keep_lo == keep_hi) | ~has


def erode(depth, radius):
    """Erosion: a pixel survives if every pixel of the (2 radius + 1)^2 window is inside the image and not 0.  Radius 0
    is the border copy: the outermost ring of pixels is set to 0."""
    d = np.asarray(depth)
    h, w = d.shape
    r = max(radius, 1) if radius > 0 else 0
    ok = np.ones((h, w), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ok &= _shifted(d, dy, dx, 0) != 0
    if radius == 0:
        ok = np.zeros((h, w), bool)
        ok[1:h - 1, 1:w - 1] = True
    return np.where(ok, d, 0).astype(np.uint16)


def normals(depth, fx, fy, cx, cy, threshold_deg, depth_scaling):
    """Normals and the observation-angle test.  A pixel whose own depth and four direct neighbours are all valid gets
    the unit normal n = (R - L) x (T - B) / |...| of the neighbours' 3-D points (pointing towards the camera for
    fy > 0), and is dropped if the angle between -n and the viewing ray exceeds ... precisely: dropped if
    ray . n >= -cos(threshold).  (A cross product of length <= 1e-6 gives n = (0, 0, -1); the inputs here stay clear
    of that.)

    Returns dict: tested [h,w] bool (reached the angle test), n [h,w,3], dot [h,w], keep [h,w] bool,
    dot_margin [h,w], n_bound [h,w] (bound on |n32 - n64| per component), length [h,w]."""
    d = np.asarray(depth).astype(np.float64)
    h, w = d.shape
    z = d / depth_scaling
    tx, ty = _rays(h, w, fx, fy, cx, cy)
    P = np.stack([z * tx, z * ty, z], axis=-1)
    sh = lambda a, dy, dx: _shifted(a, dy, dx, 0.0)
    tested = (d != 0)
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        tested &= sh(d, dy, dx) != 0
    Pn = lambda dy, dx: np.stack([sh(P[..., c], dy, dx) for c in range(3)], axis=-1)
    a = Pn(0, 1) - Pn(0, -1)
    b = Pn(-1, 0) - Pn(1, 0)
    nn = np.cross(a, b)
    length = np.linalg.norm(nn, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = nn / length[..., None] * (1.0 if fy > 0 else -1.0)
        ray = np.stack([tx, ty, np.ones_like(tx)], axis=-1)
        ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
        dot = (ray * n).sum(-1)
        # error of n: the cross product's components are differences of two products of components of a and b.
        #   a, b: two point errors (_point_error at the deepest neighbour) + _COMMON_MODE;
        #   each product and the difference: 3 u |a| |b|; the vectors' errors enter as |a| e_b + |b| e_a, twice.
        zmax = np.maximum.reduce([sh(z, 0, 1), sh(z, 0, -1), sh(z, 1, 0), sh(z, -1, 0)])
        ep = 2 * _point_error(zmax, fx, fy, cx, cy)
        la, lb = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1)
        ea, eb = ep + _COMMON_MODE * la, ep + _COMMON_MODE * lb
        dn = np.sqrt(3.0) * (3 * U * la * lb + 2 * (la * eb + lb * ea))
        n_bound = dn / length + 3 * U           # + the square root, the reciprocal and the scaling
        # (a worst case: every rounding at its largest and all with one sign.  A correct float32 implementation stays
        # near a hundredth of it at the median; test_depth_ref.py bounds the median as well as the maximum.)
        dot_margin = n_bound + 12 * U           # + the ray's normalisation (5), the dot product (3), -cosf(threshold) (4)
    thr = -np.cos(np.deg2rad(float(np.float32(threshold_deg))))
    keep = tested & ~(dot >= thr)
    return dict(tested=tested, n=n, dot=dot, keep=keep, thr=thr, dot_margin=dot_margin, n_bound=n_bound, length=length)


def radii(depth, fx, fy, cx, cy, extension_factor, clamp_factor, depth_scaling):
    """Point radii and isolated-pixel removal.  For a pixel with valid depth: over its valid 8-neighbours, D = largest
    and m = smallest squared 3-D distance to the pixel's own point; radius^2 = min(extension^2 D, 2 clamp^2 m).  The pixel
    survives if all 8 neighbours are valid.

    Returns dict: has [h,w] bool, keep [h,w] bool, r2 [h,w], clamped [h,w] bool, clamp_margin [h,w] bool (the two
    candidates are within float32 error of each other), r2_bound [h,w] (absolute bound on |r2_32 - r2_64|)."""
    d = np.asarray(depth).astype(np.float64)
    h, w = d.shape
    z = d / depth_scaling
    tx, ty = _rays(h, w, fx, fy, cx, cy)
    P = np.stack([z * tx, z * ty, z], axis=-1)
    has = d != 0
    count = np.zeros((h, w), np.int64)
    D, m = np.zeros((h, w)), np.full((h, w), np.inf)
    eD, em = np.zeros((h, w)), np.zeros((h, w))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            zn = _shifted(z, dy, dx, 0.0)
            ok = zn > 0
            Q = np.stack([_shifted(P[..., c], dy, dx, 0.0) for c in range(3)], axis=-1)
            v = Q - P
            d2 = (v * v).sum(-1)
            # error of d2 = |v|^2: 2 |v| e_v for the vector's error e_v (two point errors + _COMMON_MODE), 5 u d2 for
            # the three squares and two additions, 2 u d2 for the rounding of 1 / depth_scaling
            ev = 2 * _point_error(np.maximum(zn, z), fx, fy, cx, cy) + _COMMON_MODE * np.sqrt(d2)
            e2 = 2 * np.sqrt(d2) * ev + 7 * U * d2
            count += ok
            upd = ok & (d2 > D)
            D, eD = np.where(upd, d2, D), np.where(upd, e2, eD)
            upd = ok & (d2 < m)
            m, em = np.where(upd, d2, m), np.where(upd, e2, em)
    ext2, cl = float(np.float32(extension_factor)) ** 2, 2.0 * float(np.float32(clamp_factor)) ** 2
    with np.errstate(invalid="ignore"):
        big, clamp = ext2 * D, cl * m
        e_big, e_clamp = ext2 * eD + 3 * U * big, np.where(np.isfinite(clamp), cl * em + 4 * U * clamp, 0.0)
        clamped = big > clamp
        clamp_margin = np.abs(big - clamp) <= e_big + e_clamp
        r2 = np.where(clamped, clamp, big)
        r2_bound = np.where(clamp_margin, np.maximum(e_big, e_clamp) + np.abs(big - clamp), np.where(clamped, e_clamp, e_big))
    return dict(has=has, keep=has & (count == 8), r2=r2, clamped=clamped & has, clamp_margin=clamp_margin & has,
                r2_bound=r2_bound, count=count)
