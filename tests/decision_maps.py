"""A crafted surfel map and call list that reach the per-surfel decisions of Integrate and Regularize whose rare side
no synthetic stream takes (test infrastructure, no GPU needed).

The map is grown by the CPU oracle over frames 4..8 of small_stream(obstacle_until=-1); groups of its slots, chosen by a
seeded permutation so that neighbouring slots belong to different groups, are then edited into states the frame loop
could have produced (unit normals, kept-or-invalid links, finite positions, stamps <= 8, colour flag byte 0), and a
list of calls is run on it.  The decisions (line numbers of oracle/smx_oracle_recon.c):

  1  :224 :286 :497 :568  dot_angle > 0             a surfel seen from behind
  2  :279 :458            z > occlusion_depth       the surfel lies behind the measured surface, outside the noise band
  3  :291                 measurement in front of the surfel and the normals incompatible
  4  :308                 merge candidates agree in radius and position, normals more than 20 degrees apart
  5  :509                 creation_stamp == frame   a surfel created under the current frame index is offered a measurement
  6  :554                 an active surfel is behind the camera
  7  :557 :106            projection into the border columns / rows, quadrant neighbour past the last column
  8  :589                 the candidate neighbour's normal opposes the surfel's
  9  :660                 a supporting surfel next to a new pixel is farther than rf^2 r^2
 10  :670                 two adjacent new pixels differ in depth by more than the neighbour radius
 11  :113                 nx^2 + ny^2 > 1 in the normal image
 12  :775                 the regulariser step is clamped to one surfel radius

build() returns the scenario, run_oracle() the oracle's snapshot after every call, census() counts in float64 how many
cases fall on either side of each decision.
"""
from types import SimpleNamespace

import numpy as np

import oracle as orc
from common import small_pre, small_stream
from oracle_pipeline import OraclePipeline

W, H = 160, 120
CAPACITY = 90000
INVALID = 0xFFFFFFFF
SEED = 20251
BACK_SEGMENTS = (3, 8)             # two whole 1024-slot segments in which every live slot is back-facing
REL = 1e-4                         # census: a case counts only if every comparison on its path is this clear
# pool fractions in 64ths: (name, share)
_SHARES = (("back", 4), ("occluded", 4), ("occluded_control", 2), ("tilted", 6), ("pair25", 4), ("pair5", 2),
           ("pair5_behind", 2), ("pair5_occluded", 2), ("tilted_pair", 3), ("opposed", 16), ("clamp", 4), ("control", 15))
OPPOSED_DEG = 65.0
TILTED_DEG = 45.0
# pairs of an original and a copy in a new slot at the end of the map: (group, turn of both, further turn of the copy,
# original's and copy's distance from the camera centre relative to the grown slot).  The first two meet in front of the
# measured surface, where the merge does not ask for compatible normals (:287); in the last two the copy lies just behind
# it, compatible in one (and merged), 45 degrees off in the other (:291 keeps it, though it equals its original).  In
# pair5_occluded the original lies just inside the 5 % noise band behind the surface and supports the pixel, the copy just
# outside it: occluded (:279), or it would merge.
_PAIRS = (("pair25", 0.0, 25.0, 0.995, 0.995), ("pair5", 0.0, 5.0, 0.995, 0.995),
          ("pair5_behind", 0.0, 5.0, 0.999, 1.002), ("tilted_pair", 45.0, 0.0, 0.999, 1.002),
          ("pair5_occluded", 0.0, 5.0, 1.048, 1.052))
# frame 9's depth: every second row of one block 7 % nearer (a new pixel beside a supported one, :660); in another block
# the even rows 7 % and the odd rows 14 % nearer (new pixels on both sides of every step, :670)
STEP_ROWS, STEP_COLS, STEP_FACTOR = slice(10, 30, 2), slice(10, 60), 0.93
STEP2_ROWS, STEP2_COLS, STEP2_FACTORS = slice(70, 90), slice(100, 140), (0.93, 0.86)
BAD_NORMAL_ROWS, BAD_NORMAL_COLS = slice(40, 44), slice(70, 90)


def _turned(T, yaw_deg, pitch_deg):
    """The pose T with the camera turned about its own y axis, then its own x axis."""
    th, ph = np.radians(yaw_deg), np.radians(pitch_deg)
    Ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ph), -np.sin(ph)], [0, np.sin(ph), np.cos(ph)]])
    T2 = np.asarray(T, np.float64).copy()
    T2[:, :3] = T2[:, :3] @ Ry @ Rx
    return T2.astype(np.float32)


def build():
    """The scenario: .rows [25, count] float32, .count, .merge_count, .groups (name -> slot indices), .calls, .camera,
    .pre, .capacity.  A call is a namespace with .kind 'regularize' (frame, weight, radius_factor, window) or 'integrate'
    (frame, pose, depth, normals, radius, color, params); the images of a call are never written to."""
    s = small_stream(W, H, obstacle_until=-1)
    pre = small_pre(W)
    params = orc.IntegrateParams.defaults()
    po = OraclePipeline(W, H, s.fx, s.fy, s.cx, s.cy, CAPACITY, pre, params)
    for f in range(0, 16):
        d, c = s.frame(f)
        po.upload(f, d, c)
    for f in range(4, 9):
        po.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    n0, merge_count = po.recon.surfels_size, po.recon.merge_count
    grown = po.recon.surfels()[:, :n0].copy()

    T = np.asarray(s.pose(9), np.float64)
    R, centre = T[:, :3], T[:, 3]
    rng = np.random.default_rng(SEED)
    live = grown[7] > 0
    in_back_segment = np.zeros(n0, bool)
    for seg in BACK_SEGMENTS:
        assert (seg + 1) * 1024 <= n0
        in_back_segment[seg * 1024:(seg + 1) * 1024] = True
    pool = rng.permutation(np.flatnonzero(live & ~in_back_segment))
    groups, at = {}, 0
    for name, share in _SHARES:
        k = len(pool) * share // 64
        groups[name] = np.sort(pool[at:at + k])
        at += k
    groups["back_segments"] = np.flatnonzero(live & in_back_segment)

    n_pairs = sum(len(groups[name]) for name, _, _, _, _ in _PAIRS)
    if (n0 + n_pairs) % 1024 == 0:                 # the appended copies leave the count off a segment boundary
        groups["pair5"] = groups["pair5"][:-1]
        n_pairs -= 1
    rows = np.zeros((25, n0 + n_pairs), np.float32)
    rows[:, :n0] = grown
    u32 = rows.view(np.uint32)

    def about_camera_x(idx, deg):
        th = np.radians(np.broadcast_to(np.asarray(deg, np.float64), (len(idx),)))
        nl = R.T @ rows[8:11, idx].astype(np.float64)
        out = np.stack([nl[0], np.cos(th) * nl[1] - np.sin(th) * nl[2], np.sin(th) * nl[1] + np.cos(th) * nl[2]])
        rows[8:11, idx] = (R @ out).astype(np.float32)

    def along_ray(idx, factor):
        p = rows[0:3, idx].astype(np.float64)
        q = centre[:, None] + factor * (p - centre[:, None])
        rows[3:6, idx] = (rows[3:6, idx].astype(np.float64) + (q - p)).astype(np.float32)
        rows[0:3, idx] = q.astype(np.float32)

    for name in ("back", "back_segments"):
        rows[8:11, groups[name]] *= -1.0
    along_ray(groups["occluded"], 1.08)
    along_ray(groups["occluded_control"], 1.02)
    about_camera_x(groups["tilted"], TILTED_DEG)
    along_ray(groups["tilted"], 1.01)              # just behind the measured surface: the compatibility test runs
    at = n0
    for name, both_deg, deg, factor, copy_factor in _PAIRS:
        src = groups[name]
        new = np.arange(at, at + len(src))
        at += len(src)
        about_camera_x(src, both_deg)
        rows[:, new] = rows[:, src]
        along_ray(src, factor)
        along_ray(new, copy_factor)
        about_camera_x(new, deg)
        u32[19:23, new] = INVALID
        groups[name + "_copy"] = new
    opp = groups["opposed"]
    sign = np.where(rng.random(len(opp)) < 0.5, OPPOSED_DEG, -OPPOSED_DEG)
    about_camera_x(opp, sign)
    along_ray(opp, 0.99)
    cl = groups["clamp"]
    rows[3:6, cl] = rows[0:3, cl] + 3.0 * np.sqrt(rows[7, cl]) * rows[8:11, cl]

    # images: frame 9 (edited) and frame 10
    def images(f, edit):
        po.preprocess(f, s.outlier_frames(f), s.others_TR_reference(f))
        depth, normals, radius = po.depth_final.copy(), po.normals.copy().reshape(H, W, 2), po.radius.copy()
        if edit:
            depth[STEP_ROWS, STEP_COLS] = (depth[STEP_ROWS, STEP_COLS].astype(np.float32) * STEP_FACTOR).astype(np.uint16)
            for j, factor in enumerate(STEP2_FACTORS):
                rws = slice(STEP2_ROWS.start + j, STEP2_ROWS.stop, 2)
                depth[rws, STEP2_COLS] = (depth[rws, STEP2_COLS].astype(np.float32) * factor).astype(np.uint16)
            normals[BAD_NORMAL_ROWS, BAD_NORMAL_COLS] = 0.9
        return depth, normals, radius, po.color[f].copy()

    def to_the_edge(img):
        """Preprocessing leaves a border without depth, behind which :557 cannot be seen (:562 drops what projects onto
        a pixel without depth): every row, then every column, carries its outermost valid pixel on to the image edge."""
        depth, normals, radius, color = (a.copy() for a in img)
        for transposed in (False, True):
            d, nrm, rad = (depth.T, normals.transpose(1, 0, 2), radius.T) if transposed else (depth, normals, radius)
            for y in range(d.shape[0]):
                x = np.flatnonzero(d[y] > 0)
                if len(x):
                    for a in (d, nrm, rad):
                        a[y, :x[0]], a[y, x[-1] + 1:] = a[y, x[0]], a[y, x[-1]]
        return depth, normals, radius, color

    img9, img10 = images(9, True), images(10, False)
    img10b = to_the_edge(img10)

    def integrate(frame, pose, img, tag):
        return SimpleNamespace(kind="integrate", tag=tag, frame=frame, pose=np.asarray(pose, np.float32), depth=img[0],
                               normals=img[1], radius=img[2], color=img[3], params=params, depth_scaling=pre.depth_scaling)

    T32 = s.pose(9)
    calls = [
        SimpleNamespace(kind="regularize", tag="regularize", frame=8, weight=10.0, radius_factor=2.0, window=30),
        integrate(9, T32, img9, "frame 9, edited images"),
        integrate(10, _turned(T32, 6.0, 0.0), img10b, "yaw +6"),
        integrate(10, _turned(T32, 6.0, 0.0), img10b, "yaw +6 again, same frame index"),
        integrate(11, _turned(T32, -6.0, 0.0), img10b, "yaw -6"),
        integrate(12, _turned(T32, -9.0, 0.0), img10b, "yaw -9"),
        integrate(13, _turned(T32, -12.0, 0.0), img10b, "yaw -12"),
        integrate(14, _turned(T32, -15.0, 0.0), img10b, "yaw -15"),
        integrate(15, _turned(T32, 0.0, 5.0), img10b, "pitch +5"),
        integrate(16, _turned(T32, 0.0, -5.0), img10b, "pitch -5"),
        integrate(17, _turned(T32, 120.0, 0.0), img10, "yaw 120"),
        # the map behind the camera (:554) while the surfels of the first of these two calls support the second
        integrate(18, _turned(T32, 180.0, 0.0), img10, "yaw 180"),
        integrate(19, _turned(T32, 180.0, 0.0), img10, "yaw 180 again"),
    ]
    for c in calls[1:]:
        for a in (c.depth, c.normals, c.radius, c.color):
            a.setflags(write=False)
    rows.setflags(write=False)
    return SimpleNamespace(rows=rows, count=rows.shape[1], merge_count=merge_count, grown_count=n0, groups=groups,
                           calls=calls, camera=(s.fx, s.fy, s.cx, s.cy), pre=pre, capacity=CAPACITY, pose9=T32)


def run_oracle(sc, on_call=None):
    """Runs the oracle through the scenario; returns one snapshot per call: rows_before / rows (after), count,
    merge_count, surfel_count, scratch (copies of the oracle's images), depth (the blended depth), stats, camera."""
    fx, fy, cx, cy = sc.camera
    rec = orc.Recon(sc.capacity, W, H, fx, fy, cx, cy)
    rec.surfels()[:, :sc.count] = sc.rows
    rec.set_counts(sc.count, sc.merge_count)
    snaps = []
    for c in sc.calls:
        before = rec.surfels()[:, :rec.surfels_size].copy()
        depth = None
        if c.kind == "regularize":
            rec.regularize(c.frame, c.weight, c.radius_factor, c.window)
        else:
            depth = c.depth.copy()
            rec.integrate(c.frame, c.depth_scaling, depth, c.normals, c.radius, c.color, c.pose, c.params)
        n = rec.surfels_size
        scratch = {k: v.copy() for k, v in rec.scratch().items()}
        snap = SimpleNamespace(rows_before=before, rows=rec.surfels()[:, :n].copy(), count=n,
                               merge_count=rec.merge_count, surfel_count=rec.surfel_count, scratch=scratch,
                               depth=depth, stats=rec.stats(), camera=sc.camera)
        snaps.append(snap)
        if on_call:
            on_call(c, snap)
    rec.close()
    return snaps


# ---- census ---------------------------------------------------------------------------------------------------------
class _Path:
    """The cases that are still on a code path (.on) and whose every comparison so far was clear of its threshold."""

    def __init__(self, size):
        self.on, self.clear = np.ones(size, bool), np.ones(size, bool)

    def gt(self, q, thr, scale):
        with np.errstate(invalid="ignore"):
            self.clear &= ~self.on | (np.abs(q - thr) > REL * np.abs(scale))
            return q > thr

    def keep(self, cond):
        self.on &= cond

    def count(self, rare):
        m = self.on & self.clear
        return int(np.count_nonzero(m & rare)), int(np.count_nonzero(m & ~rare))


def _add(out, decision, site, pair):
    a = out.setdefault(decision, {}).setdefault(site, (0, 0))
    out[decision][site] = (a[0] + pair[0], a[1] + pair[1])


def _projection(rows, pose, camera):
    """float64 projection of every slot: local point, u, v, pixel, validity, clearness."""
    fx, fy, cx, cy = camera
    G = np.asarray(pose, np.float64).reshape(3, 4)
    g = rows[0:3].astype(np.float64)
    loc = G[:, :3].T @ (g - G[:, 3:4])
    z = loc[2]
    dist = np.sqrt((loc * loc).sum(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * (loc[0] / z) + cx, fy * (loc[1] / z) + cy
    return SimpleNamespace(G=G, g=g, loc=loc, z=z, dist=dist, u=u, v=v)


def _second_pixel(u, v, px, py):
    """The quadrant neighbour: (has one, x, y, clear, in the branch of :106)."""
    xf, yf = u - px, v - py
    a, b = xf < yf, xf < 1 - yf
    clear = (np.abs(xf - yf) > REL) & (np.abs(xf - (1 - yf)) > REL)
    ox = np.where(a & b, px - 1, np.where(~a & ~b, px + 1, px))
    oy = np.where(a & ~b, py + 1, np.where(~a & b, py - 1, py))
    has = np.where(a & b, px > 1, np.where(a & ~b, py < H - 1, np.where(~a & b, py > 0, px < W - 1)))
    return has, ox, oy, clear, ~a & ~b


def _is_active(stamps_u32, frame, window):
    bound = np.int64(np.int32(np.uint32((int(frame) - int(window)) & 0xFFFFFFFF)))
    return stamps_u32.view(np.int32).astype(np.int64) > bound


def census(state_before, call, after):
    """float64 restatement of the PREDICATES (not of the updates) of the twelve decisions for one call.

    state_before: rows [25, n] before the call; call: an entry of build().calls; after: the oracle's snapshot after the
    call (run_oracle): its scratch images `supporting`, `first_depth`, `new_flags`, the blended depth and the rows (the
    neighbour update reads positions and normals as the integration left them).  Returns {decision: {site: (rare,
    common)}}; a case is counted only if every comparison on its path is farther than 1e-4 relative from its threshold."""
    out = {}
    if call.kind == "regularize":
        _census_regularize(state_before, call, after, out)
        return out
    camera = after.camera
    fx, fy, cx, cy = camera
    p = call.params
    snf, window, frame = float(np.float32(p.sensor_noise_factor)), p.surfel_integration_active_window_size, call.frame
    cos_compat = np.cos(np.radians(float(p.normal_compatibility_threshold_deg)))
    rf2 = float(p.radius_factor_for_regularization_neighbors) ** 2
    inv_scaling = 1.0 / call.depth_scaling
    n = state_before.shape[1]
    B, A = state_before, after.rows[:, :n]
    sup, first = after.scratch["supporting"].ravel(), after.scratch["first_depth"].ravel().astype(np.float64)
    nimg = call.normals.reshape(-1, 2).astype(np.float64)
    nz_arg = 1 - nimg[:, 0] ** 2 - nimg[:, 1] ** 2
    nz_clear = np.abs(nz_arg) > REL
    mn = np.stack([nimg[:, 0], nimg[:, 1], -np.sqrt(np.maximum(nz_arg, 0))])
    md_in = inv_scaling * call.depth.ravel().astype(np.float64)
    md_bl = inv_scaling * after.depth.ravel().astype(np.float64)

    pr = _projection(B, call.pose, camera)
    nB = B[8:11].astype(np.float64)
    ln = pr.G[:, :3].T @ nB
    with np.errstate(invalid="ignore", divide="ignore"):
        dot_view = (pr.loc * ln).sum(0) / pr.dist
    idx = np.arange(n)

    def visible(path, q):
        path.keep(path.gt(q.z, 0, q.dist))
        for val, hi in ((q.u, W), (q.v, H)):
            path.keep(~path.gt(-val, 0, hi) & ~path.gt(val, hi, hi) & (val != hi))
        px, py = np.floor(np.where(path.on, q.u, 0)).astype(np.int64), np.floor(np.where(path.on, q.v, 0)).astype(np.int64)
        for val, pix in ((q.u, px), (q.v, py)):   # a float32 u next to an integer may fall into the other pixel
            path.clear &= ~path.on | (np.minimum(val - pix, pix + 1 - val) > REL * np.maximum(np.abs(val), 1))
        return np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)

    active_b = _is_active(B[18].view(np.uint32), frame, window)

    # quadrant :106, where the min-depth stage calls it
    path = _Path(n)
    path.keep(active_b)
    px, py = visible(path, pr)
    has2, ox, oy, qclear, right = _second_pixel(pr.u, pr.v, px, py)
    path.clear &= qclear
    path.keep(right)
    _add(out, 7, ":106", path.count(px == W - 1))

    def pairs(path):
        """(surfel, pixel) cases of a per-surfel path: the pixel itself and the quadrant neighbour."""
        k1, k2 = py * W + px, np.clip(oy, 0, H - 1) * W + np.clip(ox, 0, W - 1)
        two = _Path(2 * n)
        two.on = np.concatenate([path.on, path.on & has2])
        two.clear = np.concatenate([path.clear, path.clear & qclear])
        return two, np.concatenate([idx, idx]), np.concatenate([k1, k2])

    def gates(path, i, k, md):
        """measurement > 0, not in front of the first surface, then the occlusion test: returns `occluded`"""
        path.keep(md[k] > 0)
        path.keep(~path.gt((1 - snf) * md[k], first[k], md[k]))
        return path.gt(pr.z[i], (1 + snf) * md[k], md[k])

    # associate
    path = _Path(n)
    path.keep(active_b)
    px, py = visible(path, pr)
    two, i, k = pairs(path)
    two.keep(~gates(two, i, k, md_in))
    _add(out, 1, ":224", two.count(two.gt(dot_view[i], 0, 1)))

    # merge (the surfel's own pixel only)
    path = _Path(n)
    path.keep(B[7] >= 0)
    px, py = visible(path, pr)
    k = py * W + px
    occluded = gates(path, idx, k, md_in)
    _add(out, 2, ":279", path.count(occluded))
    path.keep(~occluded)
    back = path.gt(dot_view, 0, 1)
    _add(out, 1, ":286", path.count(back))
    path.keep(~back)
    in_front = path.gt(pr.z, md_in[k], md_in[k])
    d = (ln * mn[:, k]).sum(0)
    sub = _Path(n)
    sub.on, sub.clear = path.on & in_front, path.clear & nz_clear[k]
    incompatible = sub.gt(cos_compat, d, 1)
    _add(out, 3, ":291", sub.count(incompatible))
    path.clear &= ~in_front | sub.clear
    path.keep(~(in_front & incompatible))
    s_ = sup[k]
    path.keep((s_ != idx) & (s_ != INVALID))
    s_ = np.where(s_ == INVALID, 0, s_).astype(np.int64)
    r2, or2 = B[7].astype(np.float64), B[7, s_].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = r2 / or2
    path.keep(~path.gt(ratio, 1.44, 1.44) & path.gt(ratio, 1 / 1.44, 1))
    d2 = ((pr.g - pr.g[:, s_]) ** 2).sum(0)
    lim = 0.5 * 0.0625 * (r2 + or2)
    path.keep(~path.gt(d2, lim, lim))
    nd = (nB * nB[:, s_]).sum(0)
    _add(out, 4, ":308", path.count(path.gt(0.93969, nd, 1)))

    # integrate
    merged_now = A[7] < 0
    path = _Path(n)
    path.keep(active_b & ~merged_now)
    px, py = visible(path, pr)
    two, i, k = pairs(path)
    occluded = gates(two, i, k, md_bl)
    _add(out, 2, ":458", two.count(occluded))
    two.keep(~occluded)
    sub = _Path(2 * n)
    sub.on, sub.clear = two.on.copy(), two.clear & nz_clear[k]
    _add(out, 11, ":113 integrate", sub.count(nz_arg[k] <= 0))
    back = two.gt(dot_view[i], 0, 1)
    _add(out, 1, ":497", two.count(back))
    two.keep(~back)
    Gn = pr.G[:, :3] @ mn[:, k]
    in_front = two.gt(pr.z[i], md_bl[k], md_bl[k])
    two.clear &= ~in_front | nz_clear[k]
    two.keep(~(in_front & two.gt(cos_compat, (nB[:, i] * Gn).sum(0), 1)))
    _add(out, 5, ":509", two.count(B[17].view(np.uint32)[i] >= frame))

    # neighbour update, on the rows the integration left behind
    qa = _projection(A, call.pose, camera)
    nA = A[8:11].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dot_a = (qa.loc * (qa.G[:, :3].T @ nA)).sum(0) / qa.dist
    path = _Path(n)
    path.keep(_is_active(A[18].view(np.uint32), frame, window))
    in_front_of_camera = path.gt(qa.z, 0, qa.dist)
    _add(out, 6, ":554", path.count(~in_front_of_camera))
    path.keep(in_front_of_camera)
    sides = {"u<1": path.gt(1, qa.u, W), "u>=W-1": ~path.gt(W - 1, qa.u, W), "v<1": path.gt(1, qa.v, H),
             "v>=H-1": ~path.gt(H - 1, qa.v, H)}
    inside = ~(sides["u<1"] | sides["u>=W-1"] | sides["v<1"] | sides["v>=H-1"])
    for name, cond in sides.items():
        m = path.on & path.clear
        _add(out, 7, ":557 " + name, (int(np.count_nonzero(m & cond)), int(np.count_nonzero(m & inside))))
    path.keep(inside)
    x, y = np.floor(np.where(path.on, qa.u, 1)).astype(np.int64), np.floor(np.where(path.on, qa.v, 1)).astype(np.int64)
    for val, pix in ((qa.u, x), (qa.v, y)):
        path.clear &= ~path.on | (np.minimum(val - pix, pix + 1 - val) > REL * np.maximum(np.abs(val), 1))
    k = y * W + x
    path.keep(~path.gt(qa.z, (1 + snf) * md_bl[k], md_bl[k]))
    back = path.gt(dot_a, 0, 1)
    _add(out, 1, ":568", path.count(back))
    path.keep(~back)
    r2 = A[7].astype(np.float64)
    path.keep(r2 >= 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        path.keep(~path.gt(call.radius.ravel().astype(np.float64)[k] / r2, 2.25, 2.25))
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        nb = sup[np.clip(y + dy, 0, H - 1) * W + np.clip(x + dx, 0, W - 1)]
        q = _Path(n)
        q.on, q.clear = path.on & (nb != INVALID) & (nb != idx), path.clear.copy()
        nb = np.where(nb == INVALID, 0, nb).astype(np.int64)
        d2 = ((qa.g[:, nb] - qa.g) ** 2).sum(0)
        q.keep(~q.gt(d2, rf2 * r2, rf2 * r2))
        _add(out, 8, ":589", q.count(~q.gt((nA * nA[:, nb]).sum(0), 0, 1)))

    # create: per new pixel and direction
    new = after.scratch["new_flags"].ravel() == 1
    ky, kx = np.divmod(np.flatnonzero(new), W)
    k = ky * W + kx
    depth = md_bl[k]
    lp = np.stack([depth * ((kx + 0.5 - cx) / fx), depth * ((ky + 0.5 - cy) / fy), depth])
    gp = pr.G[:, :3] @ lp + pr.G[:, 3:4]
    r2 = call.radius.ravel().astype(np.float64)[k]
    one = _Path(len(k))
    one.clear &= nz_clear[k]
    _add(out, 11, ":113 create", one.count(nz_arg[k] <= 0))
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        kk = (ky + dy) * W + (kx + dx)           # new pixels are never on the image border
        nb = sup[kk]
        q = _Path(len(k))
        q.keep(nb != INVALID)
        nbi = np.where(nb == INVALID, 0, nb).astype(np.int64)
        ga = after.rows[0:3].astype(np.float64)[:, np.minimum(nbi, n - 1)]
        d2 = ((ga - gp) ** 2).sum(0)
        _add(out, 9, ":660", q.count(q.gt(d2, rf2 * r2, rf2 * r2)))
        q = _Path(len(k))
        q.keep((nb == INVALID) & new[kk])
        ad2 = (depth - md_bl[kk]) ** 2
        _add(out, 10, ":670", q.count(q.gt(ad2, rf2 * r2, rf2 * r2)))
    return out


def _census_regularize(B, call, after, out):
    """Decision 12 for a standalone Regularize: the accumulate and step sums in float64."""
    n = B.shape[1]
    A = after.rows[:, :n]
    stamps = B[18].view(np.uint32).view(np.int32).astype(np.int64)
    bound = np.int64(np.int32(np.uint32((int(call.frame) - int(call.window)) & 0xFFFFFFFF)))
    recent = ~(stamps < bound)
    sp, mp, nrm = B[3:6].astype(np.float64), B[0:3].astype(np.float64), B[8:11].astype(np.float64)
    links_b, links_a = B[19:23].view(np.uint32), A[19:23].view(np.uint32)
    w = float(call.weight)
    valid = links_b != INVALID
    nb = np.where(valid, links_b, 0).astype(np.int64)
    used = valid & recent[nb]
    cnt = used.sum(0)
    acc, accw = np.zeros((3, n)), np.zeros(n)
    for j in range(4):
        m = used[j]
        t = sp[:, nb[j]] - sp
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 2 * w / cnt * (nrm * t).sum(0)
        for c in range(3):
            np.add.at(acc[c], nb[j][m], (f * nrm[c])[m])
        np.add.at(accw, nb[j][m], (w / np.maximum(cnt, 1))[m])
    grad = 2 * (sp - mp) + acc
    valid_a = links_a != INVALID
    nba = np.where(valid_a, links_a, 0).astype(np.int64)
    rg = np.zeros((3, n))
    for j in range(4):
        t = sp[:, nba[j]] - sp
        rg -= np.where(valid_a[j], (nrm * t).sum(0), 0) * nrm
    cnt_a = valid_a.sum(0)
    grad = grad + np.where(cnt_a > 0, 2 * w / np.maximum(cnt_a, 1), 0) * rg
    step_len = 0.5 / (1 + w + accw) * np.sqrt((grad * grad).sum(0))
    with np.errstate(invalid="ignore"):
        max_step = np.sqrt(B[7].astype(np.float64))
    path = _Path(n)
    path.keep(recent & (B[7] > 0))
    clamped = path.gt(step_len, max_step, max_step)
    _add(out, 12, ":775", path.count(clamped))
    out["clamped"] = path.on & path.clear & clamped
    out["free"] = path.on & path.clear & ~clamped


def total(censuses):
    """Sums the per-call results of census(): {decision: {site: (rare, common)}}."""
    out = {}
    for c in censuses:
        for dec, sites in c.items():
            if isinstance(dec, int):
                for site, pair in sites.items():
                    _add(out, dec, site, pair)
    return out
