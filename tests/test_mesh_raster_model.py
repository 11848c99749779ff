"""The numpy model of smx_recon_render_mesh (tests/mesh_raster_ref.py) pinned on hand-made cases, so that what the kernels
are compared against for equality is itself checked against something written down by hand."""
import numpy as np
import pytest

import mesh_raster_ref as rr
import mesh_ref as mr

EYE = np.eye(4, dtype=np.float32)[:3]
EMPTY = 0xFFFFFFFF


def _flat(points_px, z=1.0):
    """Rows of vertices given in pixel coordinates, on the plane z of a camera with fx = fy = 1, cx = cy = 0."""
    p = np.asarray(points_px, np.float64)
    pos = np.concatenate([p * z, np.full((p.shape[0], 1), z)], axis=1)
    return rr.rows_with_colors(pos, np.tile([0.0, 0.0, -1.0], (p.shape[0], 1)), np.full(p.shape[0], 0.01))


def _unit_cam(w, h, **kw):
    return dict(width=w, height=h, fx=1.0, fy=1.0, cx=0.0, cy=0.0, global_T_camera=EYE, **kw)


def _picture(index):
    return ["".join("." if v == EMPTY else "X" for v in row) for row in index]


def test_one_triangle_by_hand():
    # a = (0.5, 0.5), b = (4.5, 0.5), c = (0.5, 4.5): corners and both legs pass through pixel centres.  A > 0 (s = +1):
    # edge a -> b runs right (d.y == 0, d.x > 0: owns its centres), c -> a runs up (d.y < 0: owns), b -> c runs down (not).
    rows = _flat([(0.5, 0.5), (4.5, 0.5), (0.5, 4.5)])
    tri = np.array([[0, 1, 2]], np.uint32)
    want = ["XXXX..",
            "XXX...",
            "XX....",
            "X.....",
            "......"]
    out = rr.render_mesh(rows, 3, tri, **_unit_cam(6, 5))
    assert _picture(out["index"]) == want
    assert out["stats"] == dict(n_in=1, n_out_of_range=0, n_not_live=0, n_clipped=0, n_degenerate=0, n_culled=0, n_drawn=1,
                                n_large=0, n_covered_pixels=10)
    assert np.all(out["depth"][out["index"] == 0] == 1.0) and np.all(out["depth"][out["index"] == EMPTY] == 0.0)
    assert np.all(out["color"][out["index"] == EMPTY] == 0) and np.all(out["color"][out["index"] == 0][:, 3] == 255)
    # at corner a's pixel the weights are (1, 0, 0): its own colour and normal come out
    assert out["color"][0, 0, :3].tolist() == [int(rows[24].view(np.uint32)[0] >> s) & 255 for s in (0, 8, 16)]
    assert out["normal"][0, 0].tolist() == [0.0, 0.0, -1.0, 0.0]
    # the other winding: s = -1, the same ownership by direction of travel, so the same picture; it is the front face
    back = rr.render_mesh(rows, 3, tri[:, ::-1], **_unit_cam(6, 5))
    assert _picture(back["index"]) == want
    assert rr.render_mesh(rows, 3, tri, **_unit_cam(6, 5, cull_back_faces=True))["stats"]["n_culled"] == 1
    assert rr.render_mesh(rows, 3, tri[:, ::-1], **_unit_cam(6, 5, cull_back_faces=True))["stats"]["n_covered_pixels"] == 10


@pytest.mark.parametrize("reverse", [False, True])
def test_every_pixel_inside_the_grid_is_covered_exactly_once(reverse):
    rows, tri, cam = rr.grid_case(reverse)
    out = rr.render_mesh(rows, 36, tri, **cam)
    times = out["times_covered"]
    assert np.all(times[1:40, 1:40] == 1)            # strictly inside the outline (0.5 .. 40.5)^2
    assert np.all(times <= 1) and np.all(times[41:] == 0) and np.all(times[:, 41:] == 0)
    # the outline itself: the top and the left side are owned, the bottom and the right side are not
    assert np.all(times[0, 0:40] == 1) and np.all(times[0:40, 0] == 1) and np.all(times[40, :] == 0) and np.all(times[:, 40] == 0)
    assert np.all(out["depth"][times == 1] == 1.0)
    assert out["stats"]["n_drawn"] == 50 and out["stats"]["n_covered_pixels"] == 1600


def test_fronto_parallel_plane_has_the_planes_depth_exactly():
    rng = np.random.default_rng(2)
    z = 2.5
    px = rng.uniform(-5, 45, (60, 2))
    pos = np.concatenate([(px - [20.0, 15.0]) * z / 30.0, np.full((60, 1), z)], axis=1)
    rows = rr.rows_with_colors(pos, np.tile([0.0, 0.0, -1.0], (60, 1)), np.full(60, 0.01))
    tri = rng.integers(0, 60, (80, 3)).astype(np.uint32)
    out = rr.render_mesh(rows, 60, tri, 40, 30, 30.0, 30.0, 20.0, 15.0, EYE)
    hit = out["index"] != EMPTY
    assert hit.sum() > 600 and np.all(out["depth"][hit] == np.float32(z))
    assert np.all(out["normal"][hit] == np.array([0.0, 0.0, -1.0, 0.0], np.float32))
    face = rr.render_mesh(rows, 60, tri, 40, 30, 30.0, 30.0, 20.0, 15.0, EYE, normal_mode=rr.NORMAL_FACE)
    assert np.all(face["normal"][hit] == np.array([0.0, 0.0, -1.0, 0.0], np.float32))


@pytest.fixture(scope="module")
def sphere():
    """The sphere fixture under its convex hull, wound counter-clockwise seen from outside: a closed surface (the mesher's
    own output has holes, through which the far side's back faces show)."""
    from scipy.spatial import ConvexHull
    m = mr.sphere_map()
    tri = ConvexHull(m[0]).simplices.copy()
    P = m[0][tri]
    inwards = np.sum(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) * P[:, 0], axis=1) < 0
    tri[inwards] = tri[inwards][:, ::-1]
    return rr.rows_with_colors(*m), tri.astype(np.uint32)


OUTSIDE = dict(width=160, height=120, fx=131.25, fy=131.25, cx=80.0, cy=60.0,
               global_T_camera=np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -3]], np.float32))


def test_sphere_from_outside_culling_changes_nothing(sphere):
    rows, tri = sphere
    n = rows.shape[1]
    both = rr.render_mesh(rows, n, tri, **OUTSIDE)
    front = rr.render_mesh(rows, n, tri, cull_back_faces=True, **OUTSIDE)
    for k in ("depth", "index", "normal", "color"):
        assert both[k].tobytes() == front[k].tobytes()
    st = front["stats"]
    assert st["n_culled"] > 0.6 * st["n_in"] and both["stats"]["n_culled"] == 0
    assert np.all(both["times_covered"][both["index"] != EMPTY] == 2) and np.all(front["times_covered"] <= 1)
    cover = st["n_covered_pixels"] / (160 * 120)
    print("the hull mesh covers %.1f %% of the image" % (100 * cover))
    assert 0.34 < cover < 0.36            # a unit sphere from 3 away: pi (131.25 / sqrt(8))^2 pixels = 35.2 %
    hit = both["index"] != EMPTY
    assert 1.9 < both["depth"][hit].min() < 2.1 and both["depth"][hit].max() < 3.0
    # vertex normals point back at the camera in the middle of the disc, and have unit length wherever something is drawn
    assert both["normal"][60, 80, 2] < -0.9
    assert np.allclose(np.linalg.norm(both["normal"][hit][:, :3], axis=1), 1.0, atol=1e-6)
    # the radii colour mode is another picture
    radii = rr.render_mesh(rows, n, tri, color_flags=4, **OUTSIDE)
    assert radii["depth"].tobytes() == both["depth"].tobytes() and radii["color"].tobytes() != both["color"].tobytes()
    assert np.all(radii["color"][hit][:, 2] == 80)


def test_coplanar_duplicates_resolve_to_the_earlier_index():
    rows = _flat([(0.5, 0.5), (8.5, 0.5), (0.5, 8.5), (8.5, 8.5)])
    tri = np.array([[3, 2, 1], [0, 1, 2], [0, 1, 2], [2, 0, 1]], np.uint32)
    out = rr.render_mesh(rows, 4, tri, **_unit_cam(10, 10))
    assert set(np.unique(out["index"])) == {0, 1, EMPTY}
    assert np.all(out["times_covered"][out["index"] == 1] == 3)


def test_every_counter_counts():
    rows = _flat([(0.5, 0.5), (40.5, 0.5), (0.5, 40.5), (3.2, 3.3), (3.4, 3.3), (3.3, 3.4), (10.0, 10.0), (20.0, 20.0), (30.0, 30.0),
                  (1.0, 1.0), (2.0, 2.0)])
    rows[5, 9] = 0.01          # slot 9 lies in front of near_z
    rows[7, 10] = -1.0         # slot 10 is merged
    tri = np.array([[0, 2, 1],       # front-facing, a box of 40 x 40 pixels: large
                    [0, 1, 2],       # the same, back-facing: culled
                    [3, 5, 4],       # front-facing, between pixel centres: an empty box, counted nowhere
                    [6, 7, 8],       # collinear
                    [0, 1, 11],      # an index out of range
                    [0, 1, 10],      # a merged corner
                    [0, 1, 9]],      # a corner in front of the near plane
                   np.uint32)
    st = rr.render_mesh(rows, 11, tri, **_unit_cam(48, 48, cull_back_faces=True))["stats"]
    assert st["n_in"] == 7 and st["n_out_of_range"] == 1 and st["n_not_live"] == 1 and st["n_clipped"] == 1
    assert st["n_degenerate"] == 1 and st["n_culled"] == 1 and st["n_drawn"] == 1 and st["n_large"] == 1
    assert st["n_covered_pixels"] == 40 * 41 // 2
    assert all(st[k] > 0 for k in rr.STAT_KEYS)
