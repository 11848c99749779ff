"""The rule of smx_recon_triangulate_update (include/smx.h) on the CPU, with the float64 / Qhull model of tests/mesh_ref.py:
after a perturbation no star differs outside D, no slot outside A differs in the triangles it owns or in its star-triangle
count, and the old result patched on A is exactly the triangulation of the new map.  And the point of it: changes that
are confined to a part of the map leave most of the map outside D."""
import numpy as np
import pytest

import mesh_ref as mr
import mesh_update_ref as mu

FIXTURES = {
    "sphere": (lambda: mr.sphere_map(1500), mr.Params()),
    "sphere_truncated": (lambda: mr.sphere_map(1500), mr.Params(search_radius_factor=1.5, max_neighbors=16)),
    "plane": (lambda: mr.plane_map(40), mr.Params()),
}


def _check_rule(old, new, prm):
    n_prev, n = old[0].shape[0], new[0].shape[0]
    old_stars, _, _, _ = mr.stars(*old, prm)
    new_stars, _, _, _ = mr.stars(*new, prm)
    old_tri, old_st, _ = mr.triangulate(*old, prm)
    new_tri, new_st, _ = mr.triangulate(*new, prm)
    changed = mu.changed_mask(old, new)
    dirty = mu.dirty_mask(old, new, prm, changed)
    reagree = mu.reagree_mask(dirty, old_stars, new_stars, n)
    assert np.all(dirty[changed]) and np.all(reagree[dirty])
    # stars outside D are equal
    differing = [p for p in range(n) if not dirty[p] and old_stars.get(p, set()) != new_stars.get(p, set())]
    assert differing == []
    # owned triangles and distinct counts outside A are equal
    _, old_counted = mu.agree(old_stars, old, prm)
    _, new_counted = mu.agree(new_stars, new, prm)
    assert sum(new_counted.values()) == new_st["n_star_triangles"]
    outside = np.nonzero(~reagree)[0]
    assert [p for p in outside if old_counted.get(int(p), 0) != new_counted.get(int(p), 0)] == []
    keep_old = old_tri[~reagree[old_tri[:, 0].astype(np.int64)]]
    keep_new = new_tri[~reagree[new_tri[:, 0].astype(np.int64)]]
    assert keep_old.tobytes() == keep_new.tobytes()
    # the old result patched on A is the new result
    patched, n_kept = mu.patch(old_tri, old_stars, new_stars, dirty, reagree, new, prm)
    assert patched.tobytes() == new_tri.tobytes()
    print("%d -> %d slots, %d changed, |D| = %d, |A| = %d, triangles %d -> %d (%d kept)" % (
        n_prev, n, changed.sum(), dirty.sum(), reagree.sum(), old_tri.shape[0], new_tri.shape[0], n_kept))
    return changed, dirty, reagree, n_kept


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_rule_on_the_fixtures(name):
    make, prm = FIXTURES[name]
    old = make()
    new, picked = mu.perturb(old, np.arange(old[0].shape[0]), np.random.default_rng(7))
    changed, dirty, reagree, n_kept = _check_rule(old, new, prm)
    assert changed.sum() == picked.size + 20
    assert n_kept > 0 and dirty.sum() < old[0].shape[0]


def test_changes_confined_to_a_cap_leave_most_of_the_map_alone():
    old = mr.sphere_map(4000)
    cap = np.nonzero(old[0][:, 2] > 0.9)[0]
    new, _ = mu.perturb(old, cap, np.random.default_rng(11), n_append=100)
    changed, dirty, reagree, _ = _check_rule(old, new, mr.Params())
    assert dirty.sum() < new[0].shape[0] / 4


def test_changed_mask_is_bitwise():
    pos, nrm, r2 = mr.plane_map(4)
    pos[3, 0] = np.nan
    r2[5] = np.nan
    old = (pos, nrm, r2)
    assert not mu.changed_mask(old, tuple(a.copy() for a in old)).any()          # NaN equals itself
    p2 = pos.copy()
    p2[2, 2] = -0.0                                                            # -0 differs from +0
    assert mu.changed_mask(old, (p2, nrm, r2)).tolist() == [i == 2 for i in range(16)]
