"""The exact model of smx_recon_render: k_render_splat and k_render_resolve (surfelmeshing_amd/csrc/smx_splat.hpp) restated
operation for operation in numpy doubles, so that every byte of the four images can be compared for equality.  Test
infrastructure.

The rule.  Every float field of smx_render_params is widened to double as it is (near_z = 0.05f is not 0.05); L =
mesh_raster_ref.invert_pose(global_T_camera); a row of L times a float vector is summed left to right, `L0 x + L1 y + L2 z
(+ L3)`; f_max = max(fx, fy); u = fx cx / cz + cx0 (the product first); the key is (bits(float32(depth)) << 32) | slot and a
pixel keeps the smallest; the normal image is the float inverse's rotation (a transpose) times the float normal, three
products summed left to right in float32; the colour is viz_ref.vis_color with alpha 255.  numpy's + - * / sqrt floor ceil
fmin fmax on float64 are correctly rounded and never contracted, as the kernel's are with -ffp-contract=off.

Besides the images the model returns the pixel rectangle of every slot that reaches one (the host walk of
tests/test_splat_kernel_host.py compares it too) and a census: for every decision of the kernels, how many slots, (slot,
pixel) pairs or pixels took each side.  `mutant` flips one decision (MUTANTS); tests/test_splat_model.py shows that every
one of them changes what some case of tests/splat_cases.py gives."""
import numpy as np

import viz_ref as vr
from mesh_raster_ref import invert_pose

INVALID = 0xFFFFFFFF
SQUARE, DISC = 0, 1
f32, f64 = np.float32, np.float64

MUTANTS = {
    "near_ge": "cz >= near_z passes the near plane ('<' for '<=' in the rejection)",
    "far_le": "cz <= far_z passes the far plane",
    "rect_floor": "the rectangle starts at floor(u - e - 1/2) instead of ceil",
    "no_half": "the - 1/2 of the rectangle dropped",
    "no_clamp": "the disc's extent is not clamped by max_extent",
    "dz_lt": "dz < near_z instead of dz <= near_z",
    "f_min": "f_max = min(fx, fy)",
    "eps_half": "the edge-on threshold 1e-4 halved",
    "t_ge": "t >= near_z passes",
    "rho_lt": "'<' for '<=' against rho^2",
    "tie_high": "equal depth bits go to the higher slot",
    "key_cz": "the key of a disc's pixel holds cz instead of t",
    "key_double": "keys compare the depth as a double, then the slot",
}


def cam_of(fx, fy, cx, cy, near_z, far_z, half_extent, disc_factor, max_extent, mutant=None):
    """The widened fields of the call, as sp_make_cam sets them."""
    w = lambda v: float(f32(v))
    c = dict(fx=w(fx), fy=w(fy), cx=w(cx), cy=w(cy), near=w(near_z), far=w(far_z), h=w(half_extent), factor=w(disc_factor),
             max_extent=w(max_extent))
    c["f_max"] = min(c["fx"], c["fy"]) if mutant == "f_min" else max(c["fx"], c["fy"])
    return c


def _rot3(L, r, x, y, z):
    return L[4 * r] * x + L[4 * r + 1] * y + L[4 * r + 2] * z


def _count(census, name, **sides):
    for side, v in sides.items():
        census["%s: %s" % (name, side)] = census.get("%s: %s" % (name, side), 0) + int(v)


def _ztest_census(census, pix, bits, slot, npix):
    """What the z-buffer sees when the pairs arrive slot after slot, upwards and downwards: a pair beats the pixel's key by its
    depth, loses by its depth, or carries the same depth bits -- then the slot decides, and the lower slot was stored earlier
    (upwards) or later (downwards)."""
    if pix.size == 0:
        _count(census, "z-test", first=0, win_by_depth=0, loss_by_depth=0, tie_lower_slot_earlier=0, tie_lower_slot_later=0)
        return
    order = np.lexsort((slot, pix))
    p, b = pix[order], bits[order].astype(np.int64)
    start = np.ones(p.size, bool)
    start[1:] = p[1:] != p[:-1]
    first_at = np.maximum.accumulate(np.where(start, np.arange(p.size), 0))
    rank = np.arange(p.size) - first_at
    size = np.bincount(p, minlength=npix)[p]
    tot = dict(first=0, win=0, loss=0, tie_up=0, tie_down=0)
    for down in (False, True):
        rk = size - 1 - rank if down else rank
        run = np.full(npix, -1, np.int64)
        for r in range(int(rk.max()) + 1):
            sel = rk == r
            prev, cur = run[p[sel]], b[sel]
            seen = prev >= 0
            if not down:
                tot["first"] += int((~seen).sum())
                tot["win"] += int((seen & (cur < prev)).sum())
                tot["loss"] += int((seen & (cur > prev)).sum())
            tot["tie_down" if down else "tie_up"] += int((seen & (cur == prev)).sum())
            run[p[sel]] = np.where(seen, np.minimum(prev, cur), cur)
    _count(census, "z-test", first=tot["first"], win_by_depth=tot["win"], loss_by_depth=tot["loss"],
           tie_lower_slot_earlier=tot["tie_up"], tie_lower_slot_later=tot["tie_down"])


def render(rows, n, width, height, fx, fy, cx, cy, global_T_camera, near_z=0.05, far_z=1000.0, mode=SQUARE, half_extent=3.0,
           disc_factor=1.0, max_extent=16.0, color_flags=0, frame_index=0, window=2147483647, mutant=None):
    """Returns {"depth" float32 [H, W], "index" uint32 [H, W], "normal" float32 [H, W, 4], "color" uint8 [H, W, 4],
    "rects" int32 [k, 5] (slot, x0, x1, y0, y1 of every slot that passes the guard, clipped, ascending), "census"}."""
    assert mutant is None or mutant in MUTANTS
    W, H = int(width), int(height)
    c = cam_of(fx, fy, cx, cy, near_z, far_z, half_extent, disc_factor, max_extent, mutant)
    L = invert_pose(global_T_camera)
    census = {}
    err = np.errstate(invalid="ignore", divide="ignore", over="ignore")
    err.__enter__()
    # ---- per slot ----
    r2f = rows[7, :n].astype(f32)
    live = r2f >= f32(0)
    _count(census, "merged", radius_squared_negative=(r2f < 0).sum(), radius_squared_nan=np.isnan(r2f).sum(), live=live.sum())
    sl = np.nonzero(live)[0]
    px, py, pz = (rows[3 + k, sl].astype(f32).astype(f64) for k in range(3))
    cz = L[8] * px + L[9] * py + L[10] * pz + L[11]
    near_ok = cz >= c["near"] if mutant == "near_ge" else cz > c["near"]
    far_ok = cz <= c["far"] if mutant == "far_le" else cz < c["far"]
    _count(census, "near plane", cz_below=(cz < c["near"]).sum(), cz_equal=(cz == c["near"]).sum(), cz_above=(cz > c["near"]).sum(),
           cz_nan=np.isnan(cz).sum())
    _count(census, "far plane", cz_below=(cz < c["far"]).sum(), cz_equal=(cz == c["far"]).sum(), cz_above=(cz > c["far"]).sum())
    keep = near_ok & far_ok
    sl, px, py, pz, cz = sl[keep], px[keep], py[keep], pz[keep], cz[keep]
    ccx = L[0] * px + L[1] * py + L[2] * pz + L[3]
    ccy = L[4] * px + L[5] * py + L[6] * pz + L[7]
    u = c["fx"] * ccx / cz + c["cx"]
    v = c["fy"] * ccy / cz + c["cy"]
    guard = (np.abs(u) < 1e8) & (np.abs(v) < 1e8)
    _count(census, "projection guard", far_outside=(~guard & ~np.isnan(u) & ~np.isnan(v)).sum(), nan=(np.isnan(u) | np.isnan(v)).sum(),
           passes=guard.sum())
    sl, cz, ccx, ccy, u, v = sl[guard], cz[guard], ccx[guard], ccy[guard], u[guard], v[guard]
    r2 = rows[7, sl].astype(f32).astype(f64)
    if mode == DISC:
        rho = c["factor"] * np.sqrt(r2)
        dz = cz - rho
        reaches = dz < c["near"] if mutant == "dz_lt" else dz <= c["near"]
        full = 2.0 * c["f_max"] * rho / dz
        e = np.where(reaches, c["max_extent"], full if mutant == "no_clamp" else np.fmin(c["max_extent"], full))
        _count(census, "disc extent", dz_at_or_below_near=(dz <= c["near"]).sum(), dz_equal_near=(dz == c["near"]).sum(),
               clamped=(~(dz <= c["near"]) & (full > c["max_extent"])).sum(), unclamped=(~(dz <= c["near"]) & (full <= c["max_extent"])).sum())
        _count(census, "disc radius", zero=(rho == 0).sum(), infinite=np.isinf(rho).sum(), finite_positive=((rho > 0) & np.isfinite(rho)).sum())
    else:
        rho = np.zeros_like(cz)
        e = np.full_like(cz, c["h"])
        fu, fv = u - np.floor(u), v - np.floor(v)
        _count(census, "square centre", on_a_pixel_centre=((fu == 0.5) & (fv == 0.5)).sum(), on_a_pixel_edge=((fu == 0) | (fv == 0)).sum(),
               elsewhere=((fu != 0) & (fv != 0) & ~((fu == 0.5) & (fv == 0.5))).sum())
    point = mode == SQUARE and c["h"] == 0.0
    _count(census, "square rule", point=sl.size if point else 0, integer_half_extent=sl.size if mode == SQUARE and not point and c["h"] % 1 == 0 else 0,
           half_integer_half_extent=sl.size if mode == SQUARE and c["h"] % 1 == 0.5 else 0)
    half = 0.0 if mutant == "no_half" else 0.5
    if point:
        x0f, x1f, y0f, y1f = np.floor(u), np.floor(u), np.floor(v), np.floor(v)
    else:
        lo = np.floor if mutant == "rect_floor" else np.ceil
        x0f, x1f, y0f, y1f = lo(u - e - half), np.floor(u + e - half), lo(v - e - half), np.floor(v + e - half)
    x0, x1 = np.fmax(x0f, 0.0).astype(np.int64), np.fmin(x1f, float(W - 1)).astype(np.int64)
    y0, y1 = np.fmax(y0f, 0.0).astype(np.int64), np.fmin(y1f, float(H - 1)).astype(np.int64)
    nonempty = (x0 <= x1) & (y0 <= y1)
    unclipped_nonempty = (x0f <= x1f) & (y0f <= y1f)
    _count(census, "rectangle", clipped_left=(nonempty & (x0f < 0)).sum(), clipped_right=(nonempty & (x1f > W - 1)).sum(),
           clipped_top=(nonempty & (y0f < 0)).sum(), clipped_bottom=(nonempty & (y1f > H - 1)).sum(),
           outside_left=(unclipped_nonempty & (x1f < 0)).sum(), outside_right=(unclipped_nonempty & (x0f > W - 1)).sum(),
           outside_top=(unclipped_nonempty & (y1f < 0)).sum(), outside_bottom=(unclipped_nonempty & (y0f > H - 1)).sum(),
           empty_before_the_clip=(~unclipped_nonempty).sum(), one_pixel=(nonempty & (x0 == x1) & (y0 == y1)).sum(),
           inside_unclipped=(nonempty & (x0f >= 0) & (x1f <= W - 1) & (y0f >= 0) & (y1f <= H - 1)).sum())
    rects = np.stack([sl, x0, x1, y0, y1], axis=1).astype(np.int64)
    # ---- per (slot, pixel) pair ----
    nx_, ny_ = np.where(nonempty, x1 - x0 + 1, 0), np.where(nonempty, y1 - y0 + 1, 0)
    cnt = nx_ * ny_
    k = np.repeat(np.arange(sl.size), cnt)
    off = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    pxl = x0[k] + off % np.maximum(nx_[k], 1)
    pyl = y0[k] + off // np.maximum(nx_[k], 1)
    if mode == SQUARE:
        depth = cz[k]
        hit = np.ones(k.size, bool)
    else:
        nf = [rows[8 + j, sl].astype(f32).astype(f64) for j in range(3)]
        nx, ny, nz = (_rot3(L, r, *nf) for r in range(3))
        n_dot_c = nx * ccx + ny * ccy + nz * cz
        rho2 = rho * rho
        dx = (pxl.astype(f64) + 0.5 - c["cx"]) / c["fx"]
        dy = (pyl.astype(f64) + 0.5 - c["cy"]) / c["fy"]
        n_dot_d = nx[k] * dx + ny[k] * dy + nz[k]
        edge_on = np.abs(n_dot_d) < (5e-5 if mutant == "eps_half" else 1e-4)
        t = n_dot_c[k] / n_dot_d
        front = t >= c["near"] if mutant == "t_ge" else t > c["near"]
        ex, ey, ez = t * dx - ccx[k], t * dy - ccy[k], t - cz[k]
        q = ex * ex + ey * ey + ez * ez
        inside = q < rho2[k] if mutant == "rho_lt" else q <= rho2[k]
        hit = ~edge_on & front & inside
        _count(census, "disc pixel", edge_on=edge_on.sum(), not_edge_on=(~edge_on).sum(),
               t_at_or_below_near=(~edge_on & ~(t > c["near"])).sum(), t_equal_near=(~edge_on & (t == c["near"])).sum(),
               t_above_near=(~edge_on & front).sum(), inside=hit.sum(), on_the_border=(~edge_on & front & (q == rho2[k])).sum(),
               outside=(~edge_on & front & ~inside).sum(), inside_radius_zero=(hit & (rho[k] == 0)).sum(),
               inside_radius_infinite=(hit & np.isinf(rho[k])).sum())
        depth = cz[k] if mutant == "key_cz" else t
    err.__exit__(None, None, None)
    pix, slot, depth = (pyl * W + pxl)[hit], sl[k][hit].astype(np.int64), depth[hit]
    dbits = depth.astype(f32).view(np.uint32)
    _ztest_census(census, pix, dbits, slot, W * H)
    # the smallest key of every pixel
    if mutant == "key_double":
        order = np.lexsort((slot, depth, pix))
    elif mutant == "tie_high":
        order = np.lexsort((-slot, dbits, pix))
    else:
        order = np.lexsort((slot, dbits, pix))
    pix, slot, dbits = pix[order], slot[order], dbits[order]
    first = np.ones(pix.size, bool)
    first[1:] = pix[1:] != pix[:-1]
    out_bits = np.zeros(W * H, np.uint32)
    out_index = np.full(W * H, INVALID, np.uint32)
    out_bits[pix[first]] = dbits[first]
    out_index[pix[first]] = slot[first].astype(np.uint32)
    # ---- resolve ----
    covered = out_index != INVALID
    _count(census, "resolve", empty=(~covered).sum(), covered=covered.sum())
    win = out_index[covered].astype(np.int64)
    m = np.asarray(global_T_camera, f32).reshape(12)
    nrm = rows[8:11, win].astype(f32)
    normal = np.zeros((W * H, 4), f32)
    for r in range(3):      # Lf[4 r + k] = m[4 k + r]
        normal[covered, r] = ((m[r] * nrm[0]).astype(f32) + (m[4 + r] * nrm[1]).astype(f32)).astype(f32) + (m[8 + r] * nrm[2]).astype(f32)
    color = np.zeros(W * H, np.uint32)
    color[covered] = (vr.vis_color(rows, win, color_flags, frame_index, window) & np.uint32(0x00FFFFFF)) | np.uint32(0xFF000000)
    return {"depth": out_bits.view(f32).reshape(H, W), "index": out_index.reshape(H, W), "normal": normal.reshape(H, W, 4),
            "color": color.view(np.uint8).reshape(H, W, 4), "rects": rects, "census": census}


IMAGES = ("depth", "index", "normal", "color")


def same_images(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in IMAGES)
