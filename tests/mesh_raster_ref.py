"""numpy model of smx_recon_render_mesh: the contract of include/smx.h stated once more.  Test infrastructure.

Every floating-point quantity is float64 in the contract's operation order (numpy rounds each operation once and never
contracts, and its division and square root are correctly rounded, so the bits are those of the library); edge functions are
np.int64; the z-test is np.minimum on uint64 keys, so the result does not depend on the order of the (triangle, pixel) pairs.
From the reference-order surfel rows of smx_recon_debug_download_surfels."""
import numpy as np

import viz_ref as vr

f32, f64, i64 = np.float32, np.float64, np.int64
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
LARGE_PIXELS = 256
NORMAL_VERTEX, NORMAL_FACE = 0, 1
STAT_KEYS = ("n_in", "n_out_of_range", "n_not_live", "n_clipped", "n_degenerate", "n_culled", "n_drawn", "n_large", "n_covered_pixels")
PAIRS_PER_CHUNK = 1 << 21


def invert_pose(global_T_camera):
    """camera_T_global in double from the float32 [R | t]: R^T, -(R^T t) summed left to right."""
    m = np.asarray(global_T_camera, f32).reshape(12).astype(f64)
    L = np.zeros(12)
    for i in range(3):
        for k in range(3):
            L[4 * i + k] = m[4 * k + i]
        L[4 * i + 3] = -(L[4 * i + 0] * m[3] + L[4 * i + 1] * m[7] + L[4 * i + 2] * m[11])
    return L


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """global_T_camera [3, 4] (float32) of a camera at eye looking at target: x right, y down, z forward."""
    eye, target, up = (np.asarray(v, f64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z) if abs(np.dot(up, z)) < 0.999 else np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], axis=1), eye[:, None]], axis=1).astype(f32)


def _edge(Xp, Yp, Xq, Yq, Px, Py):
    return (Xq - Xp) * (Py - Yp) - (Yq - Yp) * (Px - Xp)


def _owns(Xp, Yp, Xq, Yq, s):
    dx, dy = s * (Xq - Xp), s * (Yq - Yp)
    return (dy < 0) | ((dy == 0) & (dx > 0))


def _weights(X, Y, A, px, py):
    """s E(b, c, P), s E(c, a, P), s E(a, b, P) and the coverage verdict; X, Y: [m, 3] snapped corners, px, py: [m] pixels."""
    s = np.sign(A)
    Px, Py = 256 * px + 128, 256 * py + 128
    ws, cov = [], np.ones(px.shape[0], bool)
    for p, q in ((1, 2), (2, 0), (0, 1)):
        w = s * _edge(X[:, p], Y[:, p], X[:, q], Y[:, q], Px, Py)
        cov &= (w > 0) | ((w == 0) & _owns(X[:, p], Y[:, p], X[:, q], Y[:, q], s))
        ws.append(w)
    return ws, cov


def _persp(ws, A, z):
    """q_k = l_k / z_k and Z; z: [m, 3] the corners' camera depths."""
    area = np.abs(A).astype(f64)
    q = [(ws[k].astype(f64) / area) / z[:, k] for k in range(3)]
    return q, 1.0 / ((q[0] + q[1]) + q[2])


def _normalised(N):
    len2 = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]
    ok = len2 > 0
    length = np.sqrt(np.where(ok, len2, 1.0))
    return np.stack([np.where(ok, N[k] / length, 0.0).astype(f32) for k in range(3)], axis=1)


def render_mesh(rows, n, triangles, width, height, fx, fy, cx, cy, global_T_camera, near_z=0.05, far_z=1000.0,
                cull_back_faces=False, normal_mode=NORMAL_VERTEX, color_flags=0, frame_index=0, window=0):
    """Returns dict: depth [H, W] float32, index [H, W] uint32, normal [H, W, 4] float32, color [H, W, 4] uint8, stats,
    and times_covered [H, W] (how many drawn triangles cover each pixel; not an output of the library)."""
    W, H = int(width), int(height)
    fx, fy, cx, cy, near_z, far_z = (f64(f32(v)) for v in (fx, fy, cx, cy, near_z, far_z))
    L = invert_pose(global_T_camera)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3).astype(i64)
    T = tri.shape[0]
    st = dict.fromkeys(STAT_KEYS, 0)
    st["n_in"] = T
    # ---- vertices
    rows = np.asarray(rows)
    p = rows[3:6, :n].astype(f64)
    with np.errstate(all="ignore"):
        c = [L[4 * k] * p[0] + L[4 * k + 1] * p[1] + L[4 * k + 2] * p[2] + L[4 * k + 3] for k in range(3)]
        u, v = fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy
        inside = (near_z < c[2]) & (c[2] < far_z) & (np.abs(u) < 1048576.0) & (np.abs(v) < 1048576.0)
        X = np.where(inside, np.floor(np.where(inside, u, 0.0) * 256.0 + 0.5), 0.0).astype(i64)
        Y = np.where(inside, np.floor(np.where(inside, v, 0.0) * 256.0 + 0.5), 0.0).astype(i64)
        live = ~(rows[7, :n] < 0) & np.all(np.isfinite(rows[3:6, :n]), axis=0)
    # ---- triangles: steps 1-6
    t_idx = np.arange(T)
    in_range = np.all(tri < n, axis=1)
    st["n_out_of_range"] = int(np.sum(~in_range))
    t_idx = t_idx[in_range]
    ok = np.all(live[tri[t_idx]], axis=1)
    st["n_not_live"] = int(np.sum(~ok))
    t_idx = t_idx[ok]
    ok = np.all(inside[tri[t_idx]], axis=1)
    st["n_clipped"] = int(np.sum(~ok))
    t_idx = t_idx[ok]
    TX, TY = X[tri[t_idx]], Y[tri[t_idx]]
    A = (TX[:, 1] - TX[:, 0]) * (TY[:, 2] - TY[:, 0]) - (TY[:, 1] - TY[:, 0]) * (TX[:, 2] - TX[:, 0])
    st["n_degenerate"] = int(np.sum(A == 0))
    keep = A != 0
    if cull_back_faces:
        st["n_culled"] = int(np.sum(A > 0))
        keep &= A < 0
    t_idx, TX, TY, A = t_idx[keep], TX[keep], TY[keep], A[keep]
    x0 = np.maximum(-((-(TX.min(axis=1) - 128)) // 256), 0)         # ceil
    x1 = np.minimum((TX.max(axis=1) - 128) // 256, W - 1)           # floor
    y0 = np.maximum(-((-(TY.min(axis=1) - 128)) // 256), 0)
    y1 = np.minimum((TY.max(axis=1) - 128) // 256, H - 1)
    keep = (x0 <= x1) & (y0 <= y1)
    t_idx, TX, TY, A, x0, x1, y0, y1 = (a[keep] for a in (t_idx, TX, TY, A, x0, x1, y0, y1))
    nx, ny = x1 - x0 + 1, y1 - y0 + 1
    cnt = nx * ny
    st["n_drawn"] = int(t_idx.size)
    st["n_large"] = int(np.sum(cnt > LARGE_PIXELS))
    TZ = np.stack([c[2][tri[t_idx, k]] for k in range(3)], axis=1) if t_idx.size else np.zeros((0, 3))
    # ---- coverage, depth and z-test over all (triangle, pixel of its box) pairs, a chunk of triangles at a time
    zbuf = np.full(H * W, EMPTY_KEY, np.uint64)
    times = np.zeros(H * W, i64)
    ends = np.cumsum(cnt)
    lo = 0
    while lo < t_idx.size:
        hi = max(lo + 1, int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + PAIRS_PER_CHUNK, side="right")))
        k = np.repeat(np.arange(lo, hi), cnt[lo:hi])
        off = np.arange(k.size) - np.repeat(ends[lo:hi] - cnt[lo:hi] - (ends[lo - 1] if lo else 0), cnt[lo:hi])
        px, py = x0[k] + off % nx[k], y0[k] + off // nx[k]
        ws, cov = _weights(TX[k], TY[k], A[k], px, py)
        k, px, py, ws = k[cov], px[cov], py[cov], [w[cov] for w in ws]
        _, Z = _persp(ws, A[k], TZ[k])
        key = (Z.astype(f32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | t_idx[k].astype(np.uint64)
        np.minimum.at(zbuf, py * W + px, key)
        np.add.at(times, py * W + px, 1)
        lo = hi
    # ---- resolve
    hit = np.nonzero(zbuf != EMPTY_KEY)[0]
    st["n_covered_pixels"] = int(hit.size)
    depth, index = np.zeros(H * W, f32), np.full(H * W, 0xFFFFFFFF, np.uint32)
    normal, color = np.zeros((H * W, 4), f32), np.zeros((H * W, 4), np.uint8)
    if hit.size:
        t = (zbuf[hit] & np.uint64(0xFFFFFFFF)).astype(i64)
        depth[hit] = (zbuf[hit] >> np.uint64(32)).astype(np.uint32).view(f32)
        index[hit] = t.astype(np.uint32)
        corners = tri[t]
        RX, RY = X[corners], Y[corners]
        RA = (RX[:, 1] - RX[:, 0]) * (RY[:, 2] - RY[:, 0]) - (RY[:, 1] - RY[:, 0]) * (RX[:, 2] - RX[:, 0])
        ws, cov = _weights(RX, RY, RA, hit % W, hit // W)
        assert np.all(cov)
        q, Z = _persp(ws, RA, np.stack([c[2][corners[:, k]] for k in range(3)], axis=1))
        m = [q[k] * Z for k in range(3)]
        if normal_mode == NORMAL_FACE:
            a, b, d = ([c[j][corners[:, k]] for j in range(3)] for k in range(3))
            e, f = [b[j] - a[j] for j in range(3)], [d[j] - a[j] for j in range(3)]
            g = [e[1] * f[2] - e[2] * f[1], e[2] * f[0] - e[0] * f[2], e[0] * f[1] - e[1] * f[0]]
            away = (g[0] * a[0] + g[1] * a[1]) + g[2] * a[2] > 0
            N = [np.where(away, -g[j], g[j]) for j in range(3)]
        else:
            nw = rows[8:11, :n].astype(f64)
            nc = [L[4 * j] * nw[0] + L[4 * j + 1] * nw[1] + L[4 * j + 2] * nw[2] for j in range(3)]
            N = [(m[0] * nc[j][corners[:, 0]] + m[1] * nc[j][corners[:, 1]]) + m[2] * nc[j][corners[:, 2]] for j in range(3)]
        normal[hit, :3] = _normalised(N)
        words = [vr.vis_color(rows, corners[:, k], color_flags, frame_index, window) for k in range(3)]
        for ch in range(3):
            C = [((wd >> np.uint32(8 * ch)) & np.uint32(255)).astype(f64) for wd in words]
            val = np.floor(((m[0] * C[0] + m[1] * C[1]) + m[2] * C[2]) + 0.5)
            color[hit, ch] = np.minimum(val, 255.0).astype(np.uint8)
        color[hit, 3] = 255
    return {"depth": depth.reshape(H, W), "index": index.reshape(H, W), "normal": normal.reshape(H, W, 4),
            "color": color.reshape(H, W, 4), "stats": st, "times_covered": times.reshape(H, W)}


# ---- fixtures of the issue ----
def grid_case(reverse=False):
    """A 6 x 6 vertex grid on the plane z = 1 of the camera with fx = fy = 8, cx = cy = 0.5: vertex (i, j) projects to
    (8 i + 0.5, 8 j + 0.5), the centre of pixel (8 i, 8 j), and the axis-aligned and diagonal edges pass through pixel centres.
    Two triangles per cell.  Returns (rows, triangles, camera kwargs)."""
    ii, jj = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    pos = np.stack([ii.ravel().astype(f64), jj.ravel().astype(f64), np.ones(36)], axis=1)
    nrm = np.tile(np.array([0.0, 0.0, -1.0]), (36, 1))
    rows = rows_with_colors(pos, nrm, np.full(36, 0.25))
    tri = []
    for i in range(5):
        for j in range(5):
            a, b, c, d = 6 * i + j, 6 * (i + 1) + j, 6 * (i + 1) + j + 1, 6 * i + j + 1
            tri += [(a, b, c), (a, c, d)]
    tri = np.array(tri, np.uint32)
    if reverse:
        tri = tri[:, ::-1].copy()
    cam = dict(width=48, height=44, fx=8.0, fy=8.0, cx=0.5, cy=0.5, global_T_camera=np.eye(4, dtype=f32)[:3])
    return rows, tri, cam


def rows_with_colors(pos, nrm, r2, seed=5):
    """mesh_ref.rows_of_map plus a colour row and stamps, so that every colour mode has something to show."""
    import mesh_ref as mr
    rows = mr.rows_of_map(np.asarray(pos, f64), np.asarray(nrm, f64), np.asarray(r2, f64))
    n = rows.shape[1]
    rng = np.random.default_rng(seed)
    rows[24] = (rng.integers(0, 1 << 24, n, dtype=np.uint32)).view(f32)
    rows[17] = rng.integers(0, 40, n, dtype=np.uint32).view(f32)
    rows[18] = (rows[17].view(np.uint32) + rng.integers(0, 20, n, dtype=np.uint32)).view(f32)
    return rows
