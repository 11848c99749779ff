"""Hand-built maps that take smx_recon_render through every decision of its two kernels, the views they are rendered from and
the parameter sets.  Test infrastructure: tests/test_splat_model.py asserts through the census of tests/splat_ref.py that both
sides of every decision are taken, tests/test_splat_kernel_host.py and tests/test_gpu_splat.py compare the kernels with the model.

A slot that has to sit ON a boundary is placed with coordinates that are exact in float32 (`exact=True` asserts it): depths
that are powers of two, pixel offsets from the principal point that are multiples of 1/4 horizontally (fx = 64) and of 3/4
vertically (fy = 24), so that every intermediate of the kernel's double arithmetic is exact as well.  Every other slot keeps
well away from any boundary.  Offsets are relative to the principal point, so one map serves both views."""
import numpy as np

import splat_ref as sp

f32 = np.float32
FX, FY = 64.0, 24.0
# (width, height, cx, cy): one over and one under 64 wide, neither width a multiple of 64 nor height one of 4
VIEWS = {"70x37": (70, 37, 35.25, 18.75), "33x17": (33, 17, 16.25, 8.75)}
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(f32)
INF, NAN = float("inf"), float("nan")

# name -> keyword arguments of splat_ref.render / fields of smx_render_params
PARAMS = {
    "square h=0": dict(mode=sp.SQUARE, half_extent=0.0, near_z=0.05, far_z=1000.0, color_flags=0),
    "square h=2": dict(mode=sp.SQUARE, half_extent=2.0, near_z=0.05, far_z=1000.0, color_flags=4),
    "square h=2.5": dict(mode=sp.SQUARE, half_extent=2.5, near_z=0.05, far_z=20.0, color_flags=8),
    "disc library": dict(mode=sp.DISC, near_z=0.05, far_z=1000.0, disc_factor=1.0, max_extent=16.0, color_flags=0),
    "disc tracker": dict(mode=sp.DISC, near_z=0.05, far_z=20.0, disc_factor=1.0, max_extent=16.0, color_flags=0),
    "disc factor 2 extent 4": dict(mode=sp.DISC, near_z=0.25, far_z=8.0, disc_factor=2.0, max_extent=4.0, color_flags=1,
                                   frame_index=7, window=5),
}


class Map:
    def __init__(self, view):
        self.W, self.H, self.cx, self.cy = view
        self.slots, self.notes, self.pose = [], [], IDENT

    def at(self, du, dv, z, exact=False):
        """The camera-space point that projects du, dv pixels from the principal point at depth z."""
        p = np.array([du / FX * z, dv / FY * z, z], np.float64)
        if exact:
            assert np.array_equal(p.astype(f32).astype(np.float64), p), p
        return p

    def px(self, u, v, z):
        """... that projects to the image point (u, v)."""
        return self.at(u - self.cx, v - self.cy, z)

    def add(self, p, r2, why, n=(0.0, 0.0, -1.0)):
        self.slots.append((np.asarray(p, np.float64), float(r2), np.asarray(n, np.float64)))
        self.notes.append(why)
        return len(self.slots) - 1

    def rows(self):
        k = len(self.slots)
        rows = np.zeros((25, k), f32)
        for i, (p, r2, n) in enumerate(self.slots):
            # (smooth positions in the global frame: the pose's translation added, exact for the poses used here)
            rows[3:6, i] = (p + self.pose[:, 3].astype(np.float64)).astype(f32)
            rows[7, i] = r2
            rows[8:11, i] = n
        rows[0:3] = rows[3:6]
        rows[17] = (np.arange(k) % 9).astype(np.uint32).view(f32)            # creation stamp
        rows[18] = (np.arange(k) % 11).astype(np.uint32).view(f32)           # last update stamp
        rows[19:23] = np.full((4, k), sp.INVALID, np.uint32).view(f32)
        rows[24] = ((np.arange(k, dtype=np.uint32) * np.uint32(2654435761)) & np.uint32(0x00FFFFFF)).view(f32)
        return rows


def _px_radius(pixels, z):
    """RadiusSquared of a disc facing the camera at depth z that is `pixels` wide horizontally (factor 1)."""
    return (pixels * z / FX) ** 2


def planes(view):
    """The merged test and both depth planes at every near_z / far_z of PARAMS, below, on and above."""
    m = Map(view)
    m.add(m.at(-8, -3, 1.0), -1.0, "merged: RadiusSquared < 0")
    m.add(m.at(-6, -3, 1.0), NAN, "merged: RadiusSquared NaN")
    m.add(m.at(-4, -3, 1.0), _px_radius(1.5, 1.0), "live, inside both planes")
    m.add([NAN, 0.0, 1.0], 1e-4, "NaN position: cz is NaN, rejected by the depth test")
    m.add([0.0, NAN, 1.0], 1e-4, "NaN position in y only (L[9] = 0 times NaN is NaN)")
    m.add([1e7, 0.0, 1.0], 1e-4, "projection guard: u = 6.4e8")
    m.add([0.0, -1e8, 4.0], 1e-4, "projection guard: v = -6e8")
    i = 0
    for name, z in (("near_z 0.05f", f32(0.05)), ("near_z 0.25", f32(0.25)), ("far_z 8", f32(8.0)), ("far_z 20", f32(20.0)),
                    ("far_z 1000", f32(1000.0))):
        for side, zz in (("one float below", np.nextafter(z, f32(0))), ("exactly on", z), ("one float above", np.nextafter(z, f32(np.inf)))):
            # (the pose is the identity: cz is the float itself wherever the slot is; every slot has pixels of its own)
            m.add(m.at(-30.0 + 4.0 * i, 3.0 if i % 2 else -6.0, float(zz)), _px_radius(1.5, float(zz)), "cz %s %s" % (side, name))
            i += 1
    return m


def squares(view):
    """Square mode: where the centre falls in its pixel, the four borders, a single pixel, the z-test."""
    m = Map(view)
    m.add(m.at(0.25, 0.75, 2.0, exact=True), 1e-4, "centre exactly on a pixel centre (u = cx + 1/4, v = cy + 3/4)")
    m.add(m.at(5.75, 2.25, 2.0, exact=True), 1e-4, "centre exactly on a pixel corner: u and v integers")
    m.add(m.at(-5.25, 0.4, 2.0), 1e-4, "centre on a vertical pixel edge only")
    m.add(m.at(-10.6, -3.3, 2.0), 1e-4, "centre at a generic place")
    W, H = m.W, m.H
    m.add(m.px(1.3, 0.5 * H + 0.2, 3.0), 1e-4, "clipped at the left border")
    m.add(m.px(W - 1.3, 0.5 * H - 3.2, 3.0), 1e-4, "clipped at the right border")
    m.add(m.px(0.5 * W + 6.3, 1.2, 3.0), 1e-4, "clipped at the top border")
    m.add(m.px(0.5 * W - 6.3, H - 0.8, 3.0), 1e-4, "clipped at the bottom border")
    m.add(m.px(-9.3, 0.5 * H, 3.0), 1e-4, "wholly outside on the left")
    m.add(m.px(W + 9.3, 0.5 * H, 3.0), 1e-4, "wholly outside on the right")
    m.add(m.px(0.5 * W, -9.3, 3.0), 1e-4, "wholly outside above")
    m.add(m.px(0.5 * W, H + 9.3, 3.0), 1e-4, "wholly outside below")
    m.add(m.px(-1.4, -1.4, 3.0), 1e-4, "one pixel left after the clip (the corner pixel, at h = 2 and 2.5)")
    # the z-test: pairs at one place
    a = m.at(12.3, -6.4, 2.0)
    m.add(a, 1e-4, "tie: same position as the next slot, the lower slot has to win")
    m.add(a, 1e-4, "tie: same position as the previous slot")
    b = m.at(-15.6, 5.3, 2.0)
    m.add(b * 1.25, 1e-4, "hidden behind the next slot (stored earlier when slots are walked upwards)")
    m.add(b, 1e-4, "in front of the previous slot: wins by depth")
    m.add(b * 0.75, 1e-4, "in front of both")
    m.add(b * 1.5, 1e-4, "behind all three: loses by depth")
    return m


def disc_extent(view):
    """Disc mode: the extent's three branches, dz exactly on near_z, discs at the borders."""
    m = Map(view)
    m.add(m.at(-12.3, 0.4, 1.0), 0.25, "clamped by max_extent: 2 f rho / dz = 128, and the disc is 32 pixels wide")
    m.add(m.at(14.4, -2.3, 1.0), 1.0 / 256, "unclamped at factor 1 (e = 8.5): 4 pixels wide, 1.5 high, so min(fx, fy) would cut it")
    m.add(m.at(0.25, 0.75, 1.0, exact=True), 2.0 ** -16, "unclamped at factor 2 and max_extent 4 (e = 1): on a pixel centre")
    m.add(m.at(3.4, 5.2, 0.3), 0.28 ** 2, "dz <= near_z: the disc reaches the near plane, e = max_extent")
    m.add([0.0, 0.0, float(f32(f32(0.05) + f32(2.0 ** -8)))], 2.0 ** -16, "dz exactly near_z = 0.05f at factor 1 (rho = 2^-8)")
    m.add([0.0, 0.0, 0.25 + 2.0 ** -8], 2.0 ** -18, "dz exactly near_z = 0.25 at factor 2 (rho = 2^-8)")
    W, H = m.W, m.H
    m.add(m.px(2.2, 0.5 * H + 1.3, 2.0), _px_radius(6.0, 2.0), "disc clipped at the left border")
    m.add(m.px(W - 2.2, 0.5 * H - 1.3, 2.0), _px_radius(6.0, 2.0), "disc clipped at the right border")
    m.add(m.px(0.5 * W + 3.1, 0.9, 2.0), _px_radius(6.0, 2.0), "disc clipped at the top border")
    m.add(m.px(0.5 * W - 3.1, H - 0.9, 2.0), _px_radius(6.0, 2.0), "disc clipped at the bottom border")
    m.add(m.px(-30.0, 0.5 * H, 2.0), _px_radius(3.0, 2.0), "disc wholly outside on the left")
    m.add(m.px(W + 30.0, 0.5 * H, 2.0), _px_radius(3.0, 2.0), "disc wholly outside on the right")
    m.add(m.px(0.5 * W, -30.0, 2.0), _px_radius(3.0, 2.0), "disc wholly outside above")
    m.add(m.px(0.5 * W, H + 30.0, 2.0), _px_radius(3.0, 2.0), "disc wholly outside below")
    return m


def disc_border(view):
    """A pixel whose ray meets the disc's plane exactly rho from the centre (a 3-4-5 triangle in units of 1/128)."""
    m = Map(view)
    # pixel du = 1.25, dv = 0.75: dx = 5/256, dy = 1/32; t = 2: the point (5/128, 1/16, 2); centre (2/128, 1/32, 2)
    m.add([2.0 / 128, 1.0 / 32, 2.0], 25.0 / 16384, "a pixel centre exactly on the disc's border at factor 1: <= rho^2 keeps it")
    m.add(m.at(-9.2, -2.1, 2.0), _px_radius(3.0, 2.0), "pixels well inside and well outside the disc", n=(0.3, -0.2, -0.9))
    return m


def disc_point(view):
    """Radius 0 and +inf, and the edge-on test."""
    m = Map(view)
    m.add(m.at(0.25, 0.75, 2.0, exact=True), 0.0, "radius 0 exactly on a pixel centre: one pixel, distance 0 <= 0")
    m.add(m.at(7.4, 2.9, 2.0), 0.0, "radius 0 elsewhere: an empty rectangle")
    # pixel du = 1.25 (dx = 5/256): n . d = 7.5e-5 there, below 1e-4 and above the half of it; the radius is infinite, so
    # that only the edge-on test keeps that pixel out
    m.add([5.0 / 256 * 4.0 + 0.001, 1.0 / 32 * 4.0, 4.0], INF, "edge-on for one pixel column (|n . d| = 7.5e-5); radius +inf",
          n=(1.0, 0.0, -5.0 / 256 + 7.5e-5))
    return m


def disc_near(view):
    """Tilted discs whose centre is visible and whose plane crosses the near plane inside the rectangle."""
    m = Map(view)
    # near_z = 0.25: the plane x - z = -251/1024 meets the ray of pixel du = 1.25 (dx = 5/256) at t = 1/4 exactly
    m.add([21.0 / 1024, 0.0, 17.0 / 64], 2.0 ** -10, "t exactly near_z = 0.25 at one pixel column, below it to the left", n=(1.0, 0.0, -1.0))
    # near_z = 0.05f: the plane x - z / 4 = -0.0175 has t <= 0.05 for dx <= -0.1
    m.add([0.0, 0.02, 0.07], 0.05 ** 2, "t <= near_z = 0.05f on the left of a disc whose centre is at 0.07", n=(1.0, 0.0, -0.25))
    return m


def ties(view):
    """The z-test in disc mode: coplanar overlapping discs (equal depth bits), and discs in front of each other."""
    m = Map(view)
    r2 = _px_radius(5.0, 2.0)
    m.add(m.at(-8.3, 1.2, 2.0), r2, "coplanar with the next two, overlapping: the lower slot wins the overlap")
    m.add(m.at(-4.1, 2.3, 2.0), r2, "coplanar, overlaps both neighbours")
    m.add(m.at(-0.2, 0.4, 2.0), r2, "coplanar, overlaps the previous")
    m.add(m.at(10.3, -1.2, 3.0), _px_radius(6.0, 3.0), "behind the next slot: hidden where they overlap (stored earlier, upwards)")
    m.add(m.at(12.4, -0.3, 2.0), _px_radius(4.0, 2.0), "in front of the previous slot: wins by depth", n=(0.2, 0.1, -0.95))
    m.add(m.at(14.1, 0.8, 4.0), _px_radius(6.0, 4.0), "behind both: loses by depth")
    return m


def deep(view):
    """Depths that differ as doubles and are one float: the key holds the float, so the slot decides."""
    m = Map(view)
    m.pose = IDENT.copy()
    m.pose[2, 3] = -512.0
    lo = m.add(np.array([0.5, 0.25, 513.0]) + np.array([0, 0, 2.0 ** -23]), 100.0, "cz = 513 + 2^-23: the same float as 513, lower slot")
    m.add([0.5, 0.25, 513.0], 100.0, "cz = 513: nearer as a double, the same float, higher slot: loses the tie")
    assert lo == 0
    return m


def cloud(view):
    """A few hundred random discs seen from a rotated camera: every row of L takes part, depths overlap."""
    m = Map(view)
    rng = np.random.default_rng(20240611)
    k = 300
    p = rng.uniform([-1.2, -0.6, 1.0], [1.2, 0.6, 3.5], (k, 3))
    n = rng.normal(size=(k, 3)) * [0.4, 0.4, 0.2] + [0, 0, -1.0]
    n /= np.linalg.norm(n, axis=1)[:, None]
    r2 = rng.uniform(0.02, 0.12, k) ** 2
    # look from the side: global_T_camera = [R | t], points given in the camera frame and moved to the global one
    a, b = np.deg2rad(17.0), np.deg2rad(-9.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R, t = Ry @ Rx, np.array([0.3, -0.2, 0.1])
    for i in range(k):
        m.slots.append((R @ p[i] + t, r2[i] if i % 17 else -r2[i], R @ n[i]))
        m.notes.append("random disc" if i % 17 else "random merged slot")
    m.pose = np.concatenate([R, np.zeros((3, 1))], axis=1).astype(f32)
    # (rows() adds the pose's translation: leave it zero there, the points already hold it)
    rows = m.rows()
    m.pose = np.concatenate([R, t[:, None]], axis=1).astype(f32)
    m.rows = lambda: rows
    return m


BUILDERS = {"planes": planes, "squares": squares, "disc_extent": disc_extent, "disc_border": disc_border, "disc_point": disc_point,
            "disc_near": disc_near, "ties": ties, "deep": deep, "cloud": cloud}


def cases():
    """[(name, rows, n, view keywords of splat_ref.render)] for every map in every view."""
    out = []
    for vname, view in VIEWS.items():
        for name, build in BUILDERS.items():
            m = build(view)
            rows = m.rows()
            out.append(("%s %s" % (name, vname), rows, rows.shape[1],
                        dict(width=m.W, height=m.H, fx=FX, fy=FY, cx=m.cx, cy=m.cy, global_T_camera=m.pose), m.notes))
    return out


def runs():
    """Every case with every parameter set: (case name, parameter set name, rows, n, keywords)."""
    for name, rows, n, view, _ in cases():
        for pname, p in PARAMS.items():
            yield name, pname, rows, n, dict(view, **p)


def oracle_map():
    """The oracle-built map of tests/test_render_api.py (8 frames of small_stream with the obstacle) and its capture view:
    (rows, n, view keywords).  The caller has built the oracle (the `orc` fixture)."""
    from common import small_pre, small_stream
    from oracle_pipeline import OraclePipeline
    s = small_stream(obstacle_until=8)
    po = OraclePipeline(s.width, s.height, s.fx, s.fy, s.cx, s.cy, 60000, small_pre(s.width))
    for f in range(0, 16):
        po.upload(f, *s.frame(f))
    for f in range(4, 12):
        po.process(f, s.outlier_frames(f), s.others_TR_reference(f), s.pose(f))
    n = po.recon.surfels_size
    rows = np.array(po.recon.surfels(), np.float32, copy=True)   # (the oracle's buffer goes with the pipeline)
    return rows, n, dict(width=s.width, height=s.height, fx=s.fx, fy=s.fy, cx=s.cx, cy=s.cy, global_T_camera=s.pose(11))


# the three modes of tests/test_gpu_render.py::test_render_matches_the_reference
GROWN_MODES = {"square h=0": dict(mode=sp.SQUARE, half_extent=0.0), "square h=3": dict(mode=sp.SQUARE, half_extent=3.0),
               "disc": dict(mode=sp.DISC, half_extent=3.0)}


def api_params(kw):
    """The keywords of splat_ref.render as those of api.make_render_params (positional view first)."""
    names = dict(mode="splat_mode", half_extent="splat_half_extent_in_pixels", disc_factor="disc_radius_factor",
                 max_extent="max_splat_extent_in_pixels", window="surfel_integration_active_window_size")
    view = [kw[k] for k in ("width", "height", "fx", "fy", "cx", "cy", "global_T_camera")]
    return view, {names.get(k, k): v for k, v in kw.items() if k not in ("width", "height", "fx", "fy", "cx", "cy", "global_T_camera")}
