"""The model of smx_recon_import_points (tests/import_ref.py) on the cases of tests/import_cases.py: every case reaches the
decision it is named for, every mutant of the definition fails a named case, the Jacobi iteration agrees with numpy.linalg.eigh,
and on the sphere of mesh_ref.sphere_map() the imported surfels triangulate at least as well as the fixture's own.  CPU only."""
import numpy as np
import pytest

import import_cases as ic
import import_ref as ir
import mesh_ref

# mutant -> the case that must notice it.  (There is no mutant for the order of the nine double sums: on exactly collinear clouds
# with 24-bit coordinates, where the sums do round, the reversed order still gave the same float32 normals and classes; the
# order is stated so that the host walk and the device have one answer, not because an output here depends on it.)
MUTANT_CASES = {
    "ball_lt": "on_the_ball_and_one_ulp_outside",
    "tie_high_index": "k4_tie_by_index",
    "sparse_le": "m_equal_min_and_one_below",
    "rough_ge": "planar_grid",
    "radius_last": "planar_grid",
    "orient_le": "dot_zero_view_point",
    "tie_high_column": "collinear_on_x",
    "skip_none": "planar_grid",
    "sums_float32": "n_1025",
    "bad_origin_ignored": "nan_inf_coordinates_and_origins",
}
# Measured with this iteration (the explicit two-row formulas) on the 4 000 covariances of the sphere, k = 16, search radius 0.2:
# largest off-diagonal 3.5e-8 after 3 sweeps, 4.7e-25 after 4, 1.6e-96 after 5, exactly 0 after 6; the normals after 4 and
# more sweeps lie within 1.21e-15 rad of float64 eigh's.
MEASURED_MAX_ANGLE = 1.21e-15


@pytest.fixture(scope="module")
def modelled():
    return {c.name: (c, c.model()) for c in ic.cases()}


@pytest.fixture(scope="module")
def sphere():
    pos, nrm, r2 = mesh_ref.sphere_map()
    P = pos.astype(np.float32)
    p = ir.params(k=16, search_radius=0.2, radius_rank=8, radius_scale_squared=2.0, orient=ir.ORIENT_ORIGINS)
    return P, (pos, nrm, r2), p, ir.import_model(P, None, 2.0 * P, p)


def same(a, b):
    if a[3]["failed"] != b[3]["failed"] or a[2] != b[2]:
        return False
    if not np.array_equal(ir.comparable(a[0]), ir.comparable(b[0])):
        return False
    return a[3]["failed"] or np.array_equal(a[1], b[1])


def test_every_case_reaches_its_decision(modelled):
    print()
    for name, (c, _) in modelled.items():
        print("%-44s %s" % (name, c.decision))
    cls = lambda name: modelled[name][1][3]["cls"]
    m = lambda name: modelled[name][1][3]["lists"][2]
    assert cls("m_equal_min_and_one_below").tolist() == [ir.OK] * 6 + [ir.SPARSE] * 5
    assert m("m_equal_min_and_one_below").tolist() == [6] * 6 + [5] * 5
    assert m("on_the_ball_and_one_ulp_outside")[0] == 4 and 1 in modelled["on_the_ball_and_one_ulp_outside"][1][3]["lists"][0][0, :4]
    assert 2 not in modelled["on_the_ball_and_one_ulp_outside"][1][3]["lists"][0][0, :4]
    assert (cls("exact_duplicates") == ir.DEGENERATE).all()
    assert np.array_equal(modelled["collinear_on_x"][1][3]["normals"], np.tile(np.array([0, 1, 0], np.float32), (12, 1)))
    grid = modelled["planar_grid"][1]
    assert np.array_equal(grid[3]["normals"], np.tile(np.array([0, 0, 1], np.float32), (81, 1))) and (grid[3]["lam"][:, 0] == 0).all()
    for name in ("dot_zero_view_point", "dot_zero_origins"):
        assert np.array_equal(modelled[name][1][3]["normals"][:, 2], np.ones(36, np.float32)), name
    assert np.array_equal(modelled["orient_view_point_flips"][1][3]["normals"][:, 2], -np.ones(36, np.float32))
    bad = cls("nan_inf_coordinates_and_origins")
    assert [int(bad[i]) for i in (7, 19, 33, 40, 41)] == [ir.BAD] * 5 and modelled["nan_inf_coordinates_and_origins"][1][2]["n_bad"] == 5
    lists = modelled["nan_inf_coordinates_and_origins"][1][3]["lists"]
    assert not np.isin(lists[0][np.arange(lists[0].shape[1])[None, :] < lists[2][:, None]], (7, 19, 33, 40, 41)).any()
    assert modelled["nan_origins_ignored_without_origins_mode"][1][2]["n_bad"] == 3
    assert cls("variation_at_the_threshold")[0] == ir.OK and cls("variation_one_ulp_above")[0] == ir.ROUGH
    assert modelled["k4_tie_by_index"][1][3]["lists"][0][0].tolist() == [0, 1, 2, 3] and modelled["k4_tie_by_index"][1][2]["n_saturated"] == 5
    assert modelled["k64_dense_patch"][1][2]["n_saturated"] == 300
    assert not modelled["capacity_exact"][1][3]["failed"] and modelled["capacity_exact"][1][2]["new_size"] == 43
    short = modelled["capacity_one_short"][1]
    assert short[3]["failed"] and short[2]["n_imported"] == 40 and short[2]["new_size"] == 3 and short[0].shape[1] == 3
    nem = modelled["non_empty_map"]
    assert np.array_equal(ir.comparable(nem[1][0][:, :17]), ir.comparable(nem[0].old_rows)) and nem[1][1].min() == 17
    assert (ir.u32(modelled["default_color"][1][0])[24] == 0x00ABCDEF).all()
    assert modelled["n_0"][1][2]["new_size"] == 0 and modelled["n_1"][1][2]["n_sparse"] == 1
    for n in (63, 64, 65, 1023, 1024, 1025):
        st = modelled["n_%d" % n][1][2]
        assert st["n_points"] == n == st["n_bad"] + st["n_sparse"] + st["n_degenerate"] + st["n_rough"] + st["n_imported"]
        assert st["n_imported"] > 0.9 * n


def test_rows_of_an_appended_slot(modelled):
    c, (rows, p2s, st, ex) = modelled["non_empty_map"]
    u = ir.u32(rows)
    new = p2s[p2s != ir.INVALID]
    assert np.array_equal(new, 17 + np.arange(st["n_imported"]))
    pts = c.points[p2s != ir.INVALID]
    assert np.array_equal(rows[0:3, new].T, pts) and np.array_equal(rows[3:6, new].T, pts)
    assert (rows[6, new] == 2.5).all() and (rows[7, new] > 0).all() and not rows[11:17, new].any() and not rows[23, new].any()
    assert (u[17:19, new] == 9).all() and (u[19:23, new] == 0xFFFFFFFF).all()
    assert np.array_equal(u[24, new], c.colors[p2s != ir.INVALID])
    assert np.allclose(np.linalg.norm(rows[8:11, new], axis=0), 1.0, atol=2e-7)


def test_every_mutant_fails_its_case(modelled):
    assert set(MUTANT_CASES) == set(ir.MUTANTS)
    print()
    for mutant, name in MUTANT_CASES.items():
        c, good = modelled[name]
        print("%-20s -> %s" % (mutant, name))
        assert not same(c.model(mutant=mutant), good), (mutant, name)


def test_model_is_reproducible_and_takes_given_lists(modelled):
    for name in ("nan_inf_coordinates_and_origins", "n_65", "k64_dense_patch"):
        c, good = modelled[name]
        assert same(c.model(), good) and same(c.model(lists=good[3]["lists"]), good)


def test_jacobi_on_the_matrices_no_cloud_reaches():
    lam, nrm, diag, off, V = ir.jacobi(ic.MATRICES["theta_infinite"])
    assert lam.tolist() == [[1.0, 3.0, 2.0]] and nrm.tolist() == [[1.0, 0.0, 0.0]] and not off.any()      # t = 0: only a_pq is cleared
    assert np.array_equal(V[0], np.eye(3))
    lam, nrm, _, off, V = ir.jacobi(ic.MATRICES["theta_squared_infinite"])
    assert lam.tolist() == [[1.0, 3.0, 2.0]] and np.array_equal(V[0], np.eye(3)) and not off.any()
    lam, nrm, _, off, _ = ir.jacobi(ic.MATRICES["theta_zero"], sweeps=1)
    assert lam[0, 0] == 1.0 and nrm.tolist() == [[0.0, 0.0, 1.0]] and not off.any()                       # t = 1, c = sn = 1 / sqrt(2)
    lam, nrm, _, _, _ = ir.jacobi(ic.MATRICES["all_pairs_zero"])
    assert lam.tolist() == [[1.0, 3.0, 1.0]] and nrm.tolist() == [[0.0, 1.0, 0.0]]                       # columns 1 and 2 tie: the lower


def test_jacobi_against_eigh_on_the_sphere(sphere):
    P, _, p, (_, _, _, ex) = sphere
    idx, d2, m = ex["lists"]
    C = ir.covariance(P, idx, m, np.ones(P.shape[0], bool))
    M = np.zeros((P.shape[0], 3, 3))
    for (a, b), v in C.items():
        M[:, a, b] = M[:, b, a] = v
    w, V = np.linalg.eigh(M)
    print()
    for sweeps in (3, 4, 5, ir.SWEEPS):
        lam, n, _, off, _ = ir.jacobi(C, sweeps)
        angle = np.arcsin(np.minimum(np.linalg.norm(np.cross(n, V[:, :, 0]), axis=1), 1.0)).max()
        print("%d sweeps: largest off-diagonal %.3g, largest angle to eigh %.3g rad, largest |lam0 - eigh| %.3g" % (
            sweeps, np.abs(off).max(), angle, np.abs(lam[:, 0] - w[:, 0]).max()))
    assert np.abs(off).max() < 1e-39
    assert angle <= 4 * MEASURED_MAX_ANGLE
    assert np.abs(lam[:, 0] - w[:, 0]).max() < 1e-15 * np.abs(w).max()


def test_sphere_end_to_end(sphere):
    P, (pos, nrm, r2), p, (rows, p2s, st, ex) = sphere
    assert st["n_imported"] == 4000 and st["n_saturated"] == 4000
    radial = P / np.linalg.norm(P, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip((ex["normals"] * radial).sum(1), -1.0, 1.0)))
    print("\nfitted normals against the radial direction: mean %.2f, max %.2f degrees" % (angle.mean(), angle.max()))
    assert angle.max() < 10.0
    tri, ts, _ = mesh_ref.triangulate(*mesh_ref.map_of_rows(rows))
    _, fixture, _ = mesh_ref.triangulate(pos, nrm, r2)
    print("triangles: imported %d, the fixture's own radii and normals %d" % (ts["n_triangles"], fixture["n_triangles"]))
    assert ts["n_triangles"] >= fixture["n_triangles"] and ts["truncated_lists"] == 0 and ts["star_overflow"] == 0
    t = np.sort(tri.astype(np.int64), axis=1)
    edges = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]])
    assert np.unique(edges, axis=0, return_counts=True)[1].max() <= 2      # no non-manifold edge
