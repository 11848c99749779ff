"""Hand-built maps and frames that take smx_recon_track / smx_recon_track_rgbd through the structure of their reduction and
through both sides of every decision of track_pixel and track_photo_pixel.  Test infrastructure: tests/test_track_cases.py
asserts on the CPU, through the exit codes of the exact model (tests/track_exact.py), that every listed side is taken;
tests/test_gpu_track_cases.py uploads the same maps with debug_upload_surfels and the same frames directly.

The map is a room corner of three disc grids (a back wall, a left wall, a floor) with a raised block in front of the back wall
(depth steps on all four sides) and a patch of discs cut out (a hole in D); the frame is the uncut corner rendered by the exact
splat model (tests/splat_ref.py) from a camera moved by `motion`, with a patch of depth 0, a patch of normals tilted past the
angle gate and a few normals with nx^2 + ny^2 > 1.  fx != fy and the principal points are not integers.  The model images on
the CPU come from the same exact splat model, so everything here is deterministic and needs no GPU.

Shapes (samples per stride 1 / 2 / 4 / 8):
  70x37      2590 (two workgroups, the second part-filled) / 665 / 162 / 45 (less than one wavefront)
  64x32      2048: one workgroup, every lane 8 samples
  683x3      2049: two workgroups, the second holds one sample
  1026x512   525312: ceil(n / 2048) = 257 workgroups clamped to 256, lanes with a ninth sample; 65 workgroups at stride 2
  4x37       no sample at stride 8 (the image is narrower than half the stride)"""
import functools

import numpy as np

import splat_ref as sp
import track_exact as tx
import track_ref as tr
import track_rgbd_ref as trr

f32 = np.float32
DEPTH_SCALING = 5000.0
STRIDES = (1, 2, 4, 8)


def _grid(lo0, hi0, lo1, hi1, s):
    a, b = np.arange(lo0, hi0 + 1e-9, s), np.arange(lo1, hi1 + 1e-9, s)
    A, B = np.meshgrid(a, b)
    return A.ravel(), B.ravel()


def corner(spacing, cut=True, back_z=2.5):
    """The room corner in the prediction's camera frame: (points [k, 3], normals [k, 3], colours [k] uint32)."""
    pts, nrm = [], []
    x, y = _grid(-1.0, 1.8, -2.2, 0.6, spacing)                      # back wall
    keep = ~((x > -0.5) & (x < -0.05) & (y > -1.3) & (y < -0.7)) if cut else np.ones(x.size, bool)
    pts.append(np.stack([x, y, np.full(x.size, back_z)], 1)[keep]); nrm.append(np.tile([0.0, 0.0, -1.0], (int(keep.sum()), 1)))
    z, y = _grid(0.6, back_z - spacing, -2.2, 0.6, spacing)          # left wall
    pts.append(np.stack([np.full(z.size, -1.0), y, z], 1)); nrm.append(np.tile([1.0, 0.0, 0.0], (z.size, 1)))
    x, z = _grid(-1.0 + spacing, 1.8, 0.6, back_z - spacing, spacing)  # floor
    pts.append(np.stack([x, np.full(x.size, 0.6), z], 1)); nrm.append(np.tile([0.0, -1.0, 0.0], (x.size, 1)))
    x, y = _grid(0.4, 1.0, -0.6, 0.0, spacing)                       # the raised block: 15 cm in front of the back wall
    pts.append(np.stack([x, y, np.full(x.size, back_z - 0.15)], 1)); nrm.append(np.tile([0.0, 0.0, -1.0], (x.size, 1)))
    p, n = np.concatenate(pts), np.concatenate(nrm)
    # a smooth colour field with gradients in every direction
    r = 128 + 100 * np.sin(3.1 * p[:, 0] + 1.3 * p[:, 1])
    g = 128 + 100 * np.sin(2.3 * p[:, 1] - 1.7 * p[:, 2])
    b = 128 + 100 * np.cos(2.9 * p[:, 2] + 0.7 * p[:, 0])
    col = (r.astype(np.uint32) | (g.astype(np.uint32) << 8) | (b.astype(np.uint32) << 16))
    return p, n, col


def rows_of(p, n, col, radius, pose):
    """Reference-order rows [25, k] of discs given in the camera frame of `pose` (3 x 4)."""
    pose = np.asarray(pose, np.float64).reshape(3, 4)
    k = p.shape[0]
    rows = np.zeros((25, k), f32)
    rows[3:6] = (p @ pose[:, :3].T + pose[:, 3]).T.astype(f32)
    rows[0:3] = rows[3:6]
    rows[7] = radius * radius
    rows[8:11] = (n @ pose[:, :3].T).T.astype(f32)
    rows[19:23] = np.full((4, k), sp.INVALID, np.uint32).view(f32)
    rows[24] = col.astype(np.uint32).view(f32)
    return rows


class Case:
    """name; width, height, fx, fy, cx, cy; rows (the map), pred (3 x 4 float32); depth uint16, normals float32 [H, W, 2],
    color uint8 [H, W, 3]; kw: keywords of track_rgbd_ref.Params off their defaults (levels are set by the tests)."""

    def __init__(self, name, view, rows, pred, frame, kw, note):
        self.name, self.note = name, note
        self.width, self.height, self.fx, self.fy, self.cx, self.cy = view
        self.rows, self.pred = rows, np.asarray(pred, f32).reshape(3, 4)
        self.depth, self.normals, self.color = frame
        self.kw = dict(kw)
        self.depth_scaling = DEPTH_SCALING

    @property
    def intrinsics(self):
        return (self.fx, self.fy, self.cx, self.cy)

    def params(self, levels, **more):
        kw = dict(self.kw, **more)
        return trr.Params(levels=levels, **kw)

    def render_kw(self, p):
        return dict(width=self.width, height=self.height, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy, near_z=p.near_z,
                    far_z=p.far_z, mode=sp.DISC, disc_factor=p.disc_radius_factor, max_extent=p.max_splat_extent_in_pixels,
                    color_flags=0)

    def model(self):
        """(D, M, Cm, P) of the exact splat model and the restatement of the prepare kernel, as float32 / uint32 images."""
        return _model(self)


@functools.lru_cache(maxsize=None)
def _model_of(name):
    c = by_name(name)
    p = c.params([(1, 1)])
    out = sp.render(c.rows, c.rows.shape[1], global_T_camera=c.pred, **c.render_kw(p))
    D = np.ascontiguousarray(out["depth"], f32)
    M = np.ascontiguousarray(out["normal"], f32)
    Cm = np.ascontiguousarray(out["color"]).view(np.uint32)[..., 0].copy()
    return D, M, Cm, trr.prepare(D, Cm, p.gradient_max_relative_depth_step)


def _model(c):
    return _model_of(c.name)


def frame_from_render(out, H, W):
    D = out["depth"]
    depth = np.where(D > 0, np.rint(D.astype(np.float64) * DEPTH_SCALING), 0).astype(np.uint16)
    normals = np.ascontiguousarray(out["normal"][..., :2], f32)
    color = np.ascontiguousarray(out["color"][..., :3], np.uint8)
    return depth, normals, color


VIEW_70 = (70, 37, 64.0, 24.0, 35.25, 18.75)
PRED = tr.se3_exp([0.02, -0.03, 0.01, 0.25, -0.5, 0.125]).astype(f32)
MOTION_RIGHT = [0.004, -0.006, 0.003, 0.07, 0.13, 0.02]     # after the update samples leave on the right and at the bottom
MOTION_LEFT = [-0.004, 0.006, -0.003, -0.07, -0.13, -0.02]  # ... on the left and at the top
KW = dict(max_distance=0.25, min_inliers=10)


def _corner_case(name, view, spacing, motion, note, edits=True, same_pose_offset=None, kw=None):
    W, H = view[0], view[1]
    kw = dict(KW, **(kw or {}))
    radius = 0.8 * spacing
    p_cut, n_cut, c_cut = corner(spacing, cut=True)
    rows = rows_of(p_cut, n_cut, c_cut, radius, PRED)
    prm = trr.Params(**kw)
    rk = dict(width=W, height=H, fx=view[2], fy=view[3], cx=view[4], cy=view[5], near_z=prm.near_z, far_z=prm.far_z, mode=sp.DISC,
              disc_factor=prm.disc_radius_factor, max_extent=prm.max_splat_extent_in_pixels, color_flags=0)
    if same_pose_offset is None:
        p_all, n_all, c_all = corner(spacing, cut=False)
        full = rows_of(p_all, n_all, c_all, radius, PRED)
        true_pose = tr.se3_mul(PRED, tr.se3_exp(motion)).astype(f32)
        depth, normals, color = frame_from_render(sp.render(full, full.shape[1], global_T_camera=true_pose, **rk), H, W)
    else:   # (a large image: the frame is the model's own render, pushed back by a few raw depth units)
        depth, normals, color = frame_from_render(sp.render(rows, rows.shape[1], global_T_camera=PRED, **rk), H, W)
        depth = np.where(depth > 0, depth + same_pose_offset, 0).astype(np.uint16)
        color = np.clip(color.astype(np.int32) + 9, 0, 255).astype(np.uint8)
    if edits and W >= 40 and H >= 20:
        depth[H // 2 + 3:H // 2 + 7, 8:16] = 0                            # a patch without depth
        normals[H // 2 - 9:H // 2 - 5, W // 2 + 6:W // 2 + 16] = (0.7, 0.1)    # past the angle gate, the photometric term goes on
        normals[2:5, W // 2:W // 2 + 3] = (0.9, 0.8)                        # nx^2 + ny^2 > 1: nz = -sqrt(max(0, .)) = -0
    return Case(name, view, rows, PRED, (depth, normals, color), kw, note)


def _gates_case():
    """Samples that sit exactly ON the four gates (the pose is the identity, the principal point half-integral so that one
    pixel's ray is the optical axis, every coordinate involved exact in float32):
      distance: pixel (35, 18) sees the axis; a facing disc at z = 2 and a frame depth of 2.125 m (10625 / 5000, exact):
        dx = dy = 0, dz = 1/8, d^2 = 1/64 = max_distance^2 with max_distance = 1/8;
      angle: the discs left of it have the normal (sqrt(3)/2, 0, -1/2) against a frame normal (0, 0, -1): the dot product is
        exactly 1/2 = (float)cos(60 degrees);
      gradient, intensity: min_gradient is set to |gx| of a model pixel with gy = 0, max_intensity_difference to |e| of a
        sample, both taken from the exact model below -- the comparison is then between equal floats."""
    W, H, fx, fy, cx, cy = view = (70, 37, 64.0, 24.0, 35.5, 18.5)
    ident = tr.IDENTITY.astype(f32)
    x, y = _grid(-1.3, 1.3, -1.8, 1.8, 0.2)
    p = np.stack([x, y, np.full(x.size, 2.0)], 1)
    n = np.tile([0.0, 0.0, -1.0], (x.size, 1))
    tilted = x < -0.35
    n[tilted] = (np.sqrt(0.75), 0.0, -0.5)
    colc = (128 + 100 * np.sin(2.7 * x)).astype(np.uint32)         # colour by column: no vertical gradient inside the wall
    col = colc | (colc << 8) | (colc << 16)
    rows = rows_of(p, n, col, 0.16, ident)
    rows[8:11, tilted] = np.array([[f32(np.sqrt(0.75))], [f32(0)], [f32(-0.5)]], f32)
    kw = dict(max_distance=0.125, max_normal_angle_deg=60.0, min_inliers=10)
    prm = trr.Params(**kw)
    rk = dict(width=W, height=H, fx=fx, fy=fy, cx=cx, cy=cy, near_z=prm.near_z, far_z=prm.far_z, mode=sp.DISC,
              disc_factor=prm.disc_radius_factor, max_extent=prm.max_splat_extent_in_pixels, color_flags=0)
    out = sp.render(rows, rows.shape[1], global_T_camera=ident, **rk)
    depth, normals, color = frame_from_render(out, H, W)
    normals[:] = 0                                   # every frame normal is (0, 0, -1)
    depth[depth > 0] += 60                           # 12 mm behind the model: a residual everywhere
    assert out["depth"][18, 35] == f32(2.0)
    depth[18, 35] = 10625
    color = np.clip(color.astype(np.int32) + 14, 0, 255).astype(np.uint8)
    # the two photometric gates from the exact model at the identity
    D = np.ascontiguousarray(out["depth"], f32)
    Cm = np.ascontiguousarray(out["color"]).view(np.uint32)[..., 0].copy()
    P = trr.prepare(D, Cm, prm.gradient_max_relative_depth_step)
    cand = np.argwhere((P[..., 3] != 0) & (P[..., 2] == 0) & (np.abs(P[..., 1]) > 0.004) & (depth > 0))
    assert len(cand) > 4
    gy_, gx_ = cand[len(cand) // 2]
    kw["min_gradient"] = float(abs(P[gy_, gx_, 1]))
    dp = {}
    with np.errstate(all="ignore"):
        trr.photometric(D, P, depth, color, (fx, fy, cx, cy), ident, 1, trr.Params(**kw), DEPTH_SCALING, f32, f32, dp)
    e = np.sort(np.abs(dp["e"]))
    kw["max_intensity_difference"] = float(e[(3 * len(e)) // 4])
    c = Case("gates 70x37", view, rows, ident, (depth, normals, color), kw,
             "samples exactly on the distance, angle, gradient and intensity gates")
    c.on_gradient_pixel = (int(gx_), int(gy_))
    return c


def _build():
    out = [
        _corner_case("corner right 70x37", VIEW_70, 0.2, MOTION_RIGHT, "the camera moved right and down: exits at uf >= W and wf >= H"),
        _corner_case("corner left 70x37", VIEW_70, 0.2, MOTION_LEFT, "the opposite motion: exits at uf < 0 and wf < 0"),
        _gates_case(),
        _corner_case("one workgroup 64x32", (64, 32, 58.0, 22.0, 32.25, 15.75), 0.2, MOTION_RIGHT, "2048 samples at stride 1"),
        _corner_case("two workgroups 683x3", (683, 3, 420.0, 24.0, 341.25, 1.75), 0.1, MOTION_RIGHT,
                     "2049 samples at stride 1: the second workgroup holds one"),
        _corner_case("narrow 4x37", (4, 37, 64.0, 24.0, 2.25, 18.75), 0.2, MOTION_RIGHT, "no sample at stride 8", kw=dict(min_inliers=3)),
    ]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_build())


@functools.lru_cache(maxsize=None)
def clamp_case():
    """1026 x 512 over a corner of about 20 000 discs, generated: 525 312 samples at stride 1."""
    return _corner_case("clamp 1026x512", (1026, 512, 600.0, 280.0, 513.25, 255.75), 0.03, None,
                        "257 workgroups clamped to 256, a ninth visit", edits=True, same_pose_offset=25,
                        kw=dict(max_splat_extent_in_pixels=6.0))


def by_name(name):
    if name.startswith("clamp"):
        return clamp_case()
    return {c.name: c for c in cases()}[name]


NAMES = ("corner right 70x37", "corner left 70x37", "gates 70x37", "one workgroup 64x32", "two workgroups 683x3", "narrow 4x37")


def prepare_census(D, step):
    """Which side of every decision of track_photo_pixel the pixels of D take: counts by name."""
    D = np.asarray(D, f32)
    H, W = D.shape
    y, x = np.mgrid[0:H, 0:W]
    out = {"column 0": int((x == 0).sum()), "column W-1": int((x == W - 1).sum()), "row 0": int((y == 0).sum()),
           "row H-1": int((y == H - 1).sum())}
    if H < 3 or W < 3:
        out.update({"interior": 0})
        return out
    d = D[1:-1, 1:-1]
    nb = {"left": D[1:-1, :-2], "right": D[1:-1, 2:], "up": D[:-2, 1:-1], "down": D[2:, 1:-1]}
    out["interior"] = int(d.size)
    out["centre empty"] = int((d == 0).sum())
    full = (d > 0)
    for q in nb.values():
        full = full & (q > 0)
    lim = f32(step) * d
    over = {k: np.abs(q - d) > lim for k, q in nb.items()}
    for k, q in nb.items():
        others = (d > 0)
        for k2, q2 in nb.items():
            if k2 != k:
                others = others & (q2 > 0)
        out["%s neighbour empty alone" % k] = int((others & (q == 0)).sum())
        alone = full & over[k]
        for k2 in nb:
            if k2 != k:
                alone = alone & ~over[k2]
        out["%s depth step over the limit alone" % k] = int(alone.sum())
    out["valid"] = int((full & ~over["left"] & ~over["right"] & ~over["up"] & ~over["down"]).sum())
    return out


def end_of_call_variants(c, photo):
    """The decisions at the end of a call, on case c: [(name, keywords of c.params, depth_scaling, exact, expect)].  `exact`:
    records and result are held to exact_call bit for bit (not where the sums are NaNs, whose payload nothing specifies);
    expect(records, result, want) asserts what the variant is about (want: exact_call's dict, None without `exact`)."""
    D, M, Cm, P = c.model()
    ph = (P, c.color) if photo else None
    levels = [(2, 2), (1, 2)]
    r = tx.exact_call(D, M, c.depth, c.normals, c.intrinsics, c.pred, c.params(levels, min_inlier_fraction=0.0), c.depth_scaling, ph)
    last = r["records"][-1]["sums"]
    ratio = last[tr.S_INLIERS] / last[tr.S_PIXELS]
    assert len(r["records"]) == 4 and r["status"] < tr.TOO_FEW_INLIERS and 0.3 < ratio < 1
    near = f32(ratio)
    above = near if float(near) > ratio else np.nextafter(near, f32(2))
    below = near if float(near) < ratio else np.nextafter(near, f32(0))
    untouched = r["global_T_frame"]

    def bits(a):
        return np.ascontiguousarray(a, f32).view(np.uint32)

    def expect_above(records, result, want):
        s = records[-1]["sums"]
        assert s[tr.S_INLIERS] < float(above) * s[tr.S_PIXELS] and records[-1]["status"] < tr.TOO_FEW_INLIERS
        assert result["status"] == tr.TOO_FEW_INLIERS and len(records) == 4
        # the pose before the last update: the prediction times the pose the last iteration read
        T = records and tx.next_pose(records[-2]["x"], want["records"][-2]["Tf"])
        assert np.array_equal(bits(result["global_T_frame"]), bits(tx.se3_mul(np.asarray(c.pred, f32).astype(np.float64), T).astype(f32)))
        assert not np.array_equal(bits(result["global_T_frame"]), bits(untouched))

    def expect_below(records, result, want):
        s = records[-1]["sums"]
        assert not s[tr.S_INLIERS] < float(below) * s[tr.S_PIXELS]
        assert result["status"] == records[-1]["status"] < tr.TOO_FEW_INLIERS and len(records) == 4
        T = tx.next_pose(records[-1]["x"], want["records"][-1]["Tf"])
        assert np.array_equal(bits(result["global_T_frame"]), bits(tx.se3_mul(np.asarray(c.pred, f32).astype(np.float64), T).astype(f32)))

    def expect_skip(records, result, want):
        lv, st = [q["level"] for q in records], [q["status"] for q in records]
        first = st.index(tr.CONVERGED)
        assert lv[first] == 0 and 1 <= first < 5, (lv, st)                    # level 0 converged before its six iterations ...
        assert lv.count(0) == first + 1 and lv[first + 1:] == [1] * (len(lv) - first - 1) and lv.count(1) >= 1, (lv, st)
        assert result["status"] == st[-1] == tr.OK and result["iterations_run"] == len(records)   # (a later OK overwrites it)

    def expect_not_finite(records, result, want):
        assert len(records) == 1 and records[0]["status"] == tr.NOT_FINITE == result["status"]
        assert not np.all(np.isfinite(records[0]["sums"])) and np.all(records[0]["x"] == 0)
        assert np.array_equal(bits(result["global_T_frame"]), bits(c.pred)) and result["iterations_run"] == 1

    def expect_full_ring(records, result, want):
        assert len(records) == 96 == result["iterations_run"] and [q["level"] for q in records] == [0] * 32 + [1] * 32 + [2] * 32
        assert all(q["status"] == tr.OK for q in records)

    ds = c.depth_scaling
    return [
        ("min_inlier_fraction just above the ratio", dict(levels=levels, min_inlier_fraction=float(above)), ds, True, expect_above),
        ("min_inlier_fraction just below the ratio", dict(levels=levels, min_inlier_fraction=float(below)), ds, True, expect_below),
        ("level 0 converges early", dict(levels=[(1, 6), (8, 1)], convergence_rotation=1e-4, convergence_translation=1e-4), ds, True,
         expect_skip),
        ("a float product overflows", dict(levels=levels, max_distance=1e30), 1e-30, False, expect_not_finite),
        ("a full ring", dict(levels=[(4, 32), (2, 32), (1, 32)], convergence_rotation=0.0, convergence_translation=0.0), ds, True,
         expect_full_ring),
    ]
