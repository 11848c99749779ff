"""numpy restatements of the viewer buffers (smx_recon_update_visualization_buffers) and of the headless render
(smx_recon_render), from the reference-order rows of smx_recon_debug_download_surfels / the oracle.  Test
infrastructure.

Part 1 (the viewer buffers) is float32 in the reference's operation order (UpdateSurfelVertexBufferCUDAKernel,
UpdateNeighborIndexBufferCUDAKernel, UpdateNormalVertexBufferCUDAKernel), with np.fmax / np.fmin for the device's
::max / ::min (fmaxf / fminf: a NaN operand yields the other one).  Part 2 (the render) is float64: the contract of
smx.h stated once more, plus, for every pixel, how far the result is from changing -- the relative depth gap between
the best and the second-best key, and the smallest relative margin of any candidate to one of the coverage tests."""
import numpy as np

INVALID = 0xFFFFFFFF
VIS_LAST_UPDATE, VIS_CREATION, VIS_RADII, VIS_NORMALS = 1, 2, 4, 8
SPLAT_SQUARE, SPLAT_DISC = 0, 1
f32 = np.float32


def _u8(v):
    """The float -> u8 conversion of the kernels (truncation in [0, 256), saturating outside, NaN -> 0)."""
    v = np.fmin(np.fmax(np.asarray(v, f32), f32(0)), f32(255))
    return v.astype(np.uint32)


def _rgb(r, g, b):
    return (np.asarray(r, np.uint32) | (np.asarray(g, np.uint32) << 8) | (np.asarray(b, np.uint32) << 16)).astype(np.uint32)


def vis_color(rows, idx, flags, frame_index, window):
    """The 32 colour bits of the vertex buffer for slots idx (kernels.cu:306-349, flags in the template's precedence)."""
    idx = np.asarray(idx, np.int64)
    if flags & (VIS_LAST_UPDATE | VIS_CREATION):
        creation = bool(flags & VIS_CREATION)
        stamp = rows[17 if creation else 18, idx].view(np.uint32)
        age = ((np.uint32(frame_index) - stamp).astype(np.uint32)).view(np.int32).astype(np.int64)
        max_age = 3000 if creation else int(window)
        with np.errstate(invalid="ignore", divide="ignore"):
            blend = (age - 1).astype(f32) * f32(1.0) / f32(max_age - 1)
        blend = np.fmin(f32(1), np.fmax(f32(0), blend)).astype(f32)
        inten = (255 - _u8(f32(255.99) * blend)) & 255
        out = _rgb(inten, inten, inten)
        out = np.where(age < 1, _rgb(255, 80, 80), out)
        out = np.where(age > max_age, _rgb(40, 40, 255), out)
        return out.astype(np.uint32)
    if flags & VIS_RADII:
        with np.errstate(invalid="ignore"):
            radius = np.sqrt(rows[7, idx].astype(f32))
        blend = ((radius - f32(0.0005)) / (f32(0.01) - f32(0.0005))).astype(f32)
        blend = np.fmin(f32(1), np.fmax(f32(0), blend)).astype(f32)
        red = _u8(f32(255.99) * blend)
        return _rgb(red, 255 - red, 80)
    if flags & VIS_NORMALS:
        half = f32(255.99) / f32(2.0)
        return _rgb(*[_u8(half * (rows[8 + k, idx].astype(f32) + f32(1))) for k in range(3)])
    return rows[24, idx].view(np.uint32).copy()


def vertex_buffer(rows, n, frame_index, latest_triangulated, latest_mesh_count, window, flags):
    """[n, 4] uint32 (the bits of x, y, z, colour)."""
    i = np.arange(n)
    out = np.empty((n, 4), np.uint32)
    creation = rows[17, :n].view(np.uint32)
    keep = (creation <= np.uint32(latest_triangulated)) | (i >= latest_mesh_count)
    out[:, 0] = np.where(keep, rows[3, :n], f32(np.nan)).astype(f32).view(np.uint32)
    out[:, 1] = rows[4, :n].view(np.uint32)
    out[:, 2] = rows[5, :n].view(np.uint32)
    out[:, 3] = vis_color(rows, i, flags, frame_index, window)
    return out


def neighbor_buffer(rows, n):
    """[n, 8] uint32: (slot, neighbour or slot) for the four links."""
    i = np.arange(n, dtype=np.uint32)
    out = np.empty((n, 8), np.uint32)
    for k in range(4):
        nb = rows[19 + k, :n].view(np.uint32)
        out[:, 2 * k] = i
        out[:, 2 * k + 1] = np.where(nb == INVALID, i, nb)
    return out


def normal_vertex_buffer(rows, n):
    """[n, 6] uint32 bits: smooth position, smooth position + sqrt(r^2) * normal."""
    s = rows[3:6, :n].astype(f32)
    with np.errstate(invalid="ignore"):
        radius = np.sqrt(rows[7, :n].astype(f32))
    end = (s + (radius[None, :] * rows[8:11, :n].astype(f32)).astype(f32)).astype(f32)
    return np.concatenate([s, end], axis=0).T.copy().view(np.uint32)


def equal_nan_aware(got_bits, want_bits, float_cols=None):
    """Bit equality, except that any NaN equals any NaN (the NaN masks must match)."""
    got_bits, want_bits = np.asarray(got_bits, np.uint32), np.asarray(want_bits, np.uint32)
    if float_cols is None:
        return np.array_equal(got_bits, want_bits)
    g, w = got_bits[:, float_cols].view(f32), want_bits[:, float_cols].view(f32)
    if not np.array_equal(np.isnan(g), np.isnan(w)):
        return False
    m = ~np.isnan(w)
    other = [c for c in range(got_bits.shape[1]) if c not in float_cols]
    return (np.array_equal(g.view(np.uint32)[m], w.view(np.uint32)[m]) and
            np.array_equal(got_bits[:, other], want_bits[:, other]))


def render(rows, n, width, height, fx, fy, cx, cy, global_T_camera, near_z=0.05, far_z=1000.0, mode=SPLAT_SQUARE,
           half_extent=3.0, disc_factor=1.0, max_extent=16.0):
    """float64 restatement of smx_recon_render.  Returns dict: depth [H, W] (0 = empty), index [H, W] uint32,
    gap [H, W] (relative depth gap best -> second best candidate, inf if only one), margin [H, W] (smallest relative
    margin of any candidate pixel / slot pair near a coverage test, inf if none)."""
    T = np.asarray(global_T_camera, np.float64).reshape(3, 4)
    R, t = T[:, :3], T[:, 3]
    slots = np.nonzero(rows[7, :n] >= 0)[0]
    p = rows[3:6, slots].astype(np.float64).T
    nrm = rows[8:11, slots].astype(np.float64).T
    c = (p - t) @ R                      # R^T (p - t)
    nc = nrm @ R
    inside = (c[:, 2] > near_z) & (c[:, 2] < far_z)
    zmargin = np.minimum(np.abs(c[:, 2] - near_z), np.abs(c[:, 2] - far_z)) / np.abs(c[:, 2])
    # (slots just outside the depth range stay in as candidates, flagged through their margin)
    keep = inside | (zmargin < 1e-4)
    slots, c, nc, zmargin, inside = slots[keep], c[keep], nc[keep], zmargin[keep], inside[keep]
    z = c[:, 2]
    u = fx * c[:, 0] / z + cx
    v = fy * c[:, 1] / z + cy
    scale = np.maximum(np.maximum(np.abs(u), np.abs(v)), 1.0)
    if mode == SPLAT_SQUARE:
        e = np.full(len(slots), float(half_extent))
    else:
        rho = disc_factor * np.sqrt(rows[7, slots].astype(np.float64))
        dz = z - rho
        with np.errstate(divide="ignore"):
            e = np.where(dz <= near_z, max_extent, np.minimum(max_extent, 2 * max(fx, fy) * rho / np.where(dz > 0, dz, 1)))
    # candidate rectangles, one pixel wider on each side (pairs near a rectangle's edge are flagged by their margin)
    point = (mode == SPLAT_SQUARE) and half_extent == 0
    if point:
        x0 = np.floor(u) - 1; x1 = np.floor(u) + 1; y0 = np.floor(v) - 1; y1 = np.floor(v) + 1
    else:
        x0 = np.ceil(u - e - 0.5) - 1; x1 = np.floor(u + e - 0.5) + 1
        y0 = np.ceil(v - e - 0.5) - 1; y1 = np.floor(v + e - 0.5) + 1
    x0 = np.clip(x0, 0, width); x1 = np.clip(x1, -1, width - 1)
    y0 = np.clip(y0, 0, height); y1 = np.clip(y1, -1, height - 1)
    nx = np.maximum(x1 - x0 + 1, 0).astype(np.int64)
    ny = np.maximum(y1 - y0 + 1, 0).astype(np.int64)
    cnt = nx * ny
    k = np.repeat(np.arange(len(slots)), cnt)
    off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    px = (x0[k] + off % nx[k]).astype(np.int64)
    py = (y0[k] + off // nx[k]).astype(np.int64)
    xc, yc = px + 0.5, py + 0.5
    ax, ay = np.abs(xc - u[k]), np.abs(yc - v[k])
    if point:
        covered = (px == np.floor(u[k])) & (py == np.floor(v[k]))
        fu, fv = u[k] - np.floor(u[k]), v[k] - np.floor(v[k])
        margin = np.minimum(np.minimum(fu, 1 - fu), np.minimum(fv, 1 - fv)) / scale[k]
        depth = z[k]
    else:
        in_rect = (ax <= e[k]) & (ay <= e[k])
        margin = np.abs(np.minimum(e[k] - ax, e[k] - ay)) / scale[k]
        if mode == SPLAT_SQUARE:
            covered = in_rect
            depth = z[k]
        else:
            d = np.stack([(xc - cx) / fx, (yc - cy) / fy, np.ones_like(xc)], axis=1)
            nd = (nc[k] * d).sum(1)
            ok_nd = np.abs(nd) >= 1e-4
            with np.errstate(divide="ignore", invalid="ignore"):
                tt = (nc[k] * c[k]).sum(1) / np.where(ok_nd, nd, 1.0)
                q = ((tt[:, None] * d - c[k]) ** 2).sum(1)
                r2 = rho[k] ** 2
                cov_margin = np.abs(r2 - q) / (2 * rho[k] * np.linalg.norm(c[k], axis=1))
                t_margin = np.abs(tt - near_z) / np.abs(tt)
            covered = in_rect & ok_nd & (tt > near_z) & (q <= r2)
            margin = np.minimum(margin, np.abs(np.abs(nd) - 1e-4))
            margin = np.where(ok_nd, np.minimum(margin, np.minimum(cov_margin, t_margin)), margin)
            depth = tt
    margin = np.minimum(margin, zmargin[k])
    covered &= inside[k]
    pix = py * width + px
    H, W = height, width
    out_margin = np.full(H * W, np.inf)
    near = margin < 1e-4
    np.minimum.at(out_margin, pix[near], margin[near])
    ci = np.nonzero(covered)[0]
    cp, cd, cs = pix[ci], depth[ci], slots[k[ci]].astype(np.int64)
    # key order: the depth rounded to float (its bit pattern is the key's high word), then the slot
    order = np.lexsort((cs, cd.astype(f32), cp))
    cp, cd, cs = cp[order], cd[order], cs[order]
    first = np.ones(len(cp), bool)
    first[1:] = cp[1:] != cp[:-1]
    fi = np.nonzero(first)[0]
    out_depth = np.zeros(H * W)
    out_index = np.full(H * W, INVALID, np.uint32)
    out_depth[cp[fi]] = cd[fi]
    out_index[cp[fi]] = cs[fi].astype(np.uint32)
    gap = np.full(H * W, np.inf)
    has2 = fi + 1 < len(cp)
    has2[has2] &= cp[fi[has2] + 1] == cp[fi[has2]]
    g = fi[has2]
    gap[cp[g]] = np.abs(cd[g + 1] - cd[g]) / cd[g]
    return {"depth": out_depth.reshape(H, W), "index": out_index.reshape(H, W), "gap": gap.reshape(H, W),
            "margin": out_margin.reshape(H, W)}


def unstable(ref, tol=1e-5):
    """Pixels whose result a float32 evaluation may legitimately change: key gap or coverage margin below tol."""
    return (ref["gap"] < tol) | (ref["margin"] < tol)
