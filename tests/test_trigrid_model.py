"""The cases of tests/trigrid_cases.py on the CPU: the brute-force models and the numpy grids express every one of them, and
each case is what its name says (so the GPU test of the shared build compares against something that can fail)."""
import numpy as np
import pytest

import distance_ref as dr
import raycast_ref as rr
import rayscene_ref as sr
import trigrid_cases as tc


@pytest.mark.parametrize("name", list(tc.cases()))
def test_the_models_handle_the_case(name):
    pos, nrm, r2, _ = tc.world()
    pts, rays = tc.queries()
    case = tc.cases()[name]
    tri, md = case["tri"], case["max_distance"]
    R, t_of, counts = dr.classify(pos, r2, tri)
    nearest, distance, closest, dst = dr.answer(dr.brute(pos, r2, tri, pts), md, True)
    hit, t, uv, rst = rr.answer(rr.brute(pos, r2, tri, rays, *tc.T_RANGE), 0)
    assert nearest.shape == (64,) and hit.shape == (64,) and dst["n_bad_points"] == 1 and rst["n_bad_rays"] == 1
    assert counts["n_in"] == tri.shape[0] == R.shape[0] + counts["n_not_live"] + counts["n_repeated"] + counts["n_out_of_range"]
    for cs in case["cells"]:
        cd, cr = tc.distance_cell(pos, r2, tri, cs, md), tc.raycast_cell(pos, r2, tri, cs)
        sd, srr = dr.structure(pos, r2, tri, cd, md), rr.structure(pos, r2, tri, cr)
        g = sr.grid(pos, r2, tri, cr)
        assert g["cells"].shape[0] == srr["n_cells"] and (g["lo"] is None) == (srr["n_entries"] == 0)
        if name == "every triangle wide":
            assert sd == srr == dict(n_wide=tri.shape[0], n_entries=0, n_cells=0) and R.shape[0] == tri.shape[0]
        elif name == "no triangle in R":
            assert R.shape[0] == 0 and sd == srr == dict(n_wide=0, n_entries=0, n_cells=0)
            assert min(counts["n_not_live"], counts["n_repeated"], counts["n_out_of_range"]) > 0
            if cs == 0:
                assert cd == float(dr.MARGIN * dr.F(md)) and cr == float(rr.MIN_CELL)
        elif name.startswith("wide list"):
            assert sd["n_wide"] == srr["n_wide"] == 2 and sd["n_entries"] > 0 and srr["n_entries"] > sd["n_entries"]
            assert not np.isin([63, 64, 127], t_of).any() and np.isin([10, 62, 65, 128], t_of).all()
        elif R.shape[0] > 0:
            assert sd["n_wide"] == srr["n_wide"] == 0 and srr["n_entries"] >= sd["n_entries"] >= R.shape[0]
    if R.shape[0] > 0:                      # something is found, and not everything
        assert 0 < dst["n_matched"] < 63 and 0 < rst["n_hit"] < 63
    else:
        assert dst["n_matched"] == rst["n_hit"] == 0 and np.all(nearest == dr.INVALID) and np.all(np.isinf(t))
