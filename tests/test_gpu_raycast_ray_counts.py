"""The ray counts at which the cast changes shape, through smx_recon_raycast_mesh and through a scene without and with a bit
grid: k_ray_cast takes 4 rays per workgroup and k_ray_stats is grid-stride over at most 256 workgroups of 256 lanes, so 1, 3, 4, 5,
63, 64, 65 and 257 rays sit on both sides of a workgroup of the cast, a wavefront and a workgroup of the stats, and 65 537 is the
first count at which a lane of the stats kernel sums two rays.  Everything is compared for equality with the brute-force model
of tests/raycast_ref.py, which runs once on the 1 000 unique rays."""
import numpy as np
import pytest

import mesh_ref as mr
import raycast_ref as rr
from test_gpu_raycast import _rec_of

pytestmark = pytest.mark.gpu

COUNTS = (1, 3, 4, 5, 63, 64, 65, 257)
UNIQUE = 1000
TILED = 256 * 256 + 1
T_MAX = 10.0
WORK = ("n_layers", "n_lookups", "n_pair_tests")
CAST = ("n_rays", "n_bad_rays", "n_hit", "n_front_hits", "max_t_bits")


def _take(model, idx):
    """The model of the rays idx of the model's (brute() keeps everything of a ray at the ray's position)."""
    part = dict(model)
    for k in ("key1", "key2", "uv1", "uv2", "bad"):
        part[k] = model[k][idx]
    return part


def test_ray_counts_around_every_workgroup_size_and_two_rays_per_stats_lane(smx):
    m = mr.sphere_map(n=1500)
    rec = _rec_of(smx, m)
    tri, _ = rec.Triangulate(None)
    unique = np.ascontiguousarray(rr.ray_sets()["inside-out"][0][:UNIQUE])
    assert unique.shape[0] == UNIQUE
    model = rr.brute(m[0], m[2], tri, unique, 0.0, T_MAX)
    scenes = {occ: rec.BuildRayScene(None, tri, 0.0, occ) for occ in (-1, 0)}
    assert scenes[-1].stats["occupancy_log2"] == -1 and scenes[0].stats["occupancy_log2"] >= 0
    work = {}
    for n in COUNTS + (UNIQUE, TILED):
        idx = np.arange(n) % UNIQUE
        rays = np.ascontiguousarray(unique[idx])
        wh, wt, wuv, wst = rr.answer(_take(model, idx), 0)
        bh, bt, buv, bst = rec.RaycastMesh(None, tri, rays, 0.0, T_MAX, 0.0, 0, return_uv=True)
        assert {k: bst[k] for k in rr.STAT_NAMES} == wst, (n, bst, wst)
        for got, want, name in ((bh, wh, "hit"), (bt, wt, "t"), (buv, wuv, "uv")):
            assert got.tobytes() == want.tobytes(), (n, name)
        work[n] = {k: bst[k] for k in WORK}
        for occ, sc in scenes.items():
            hit, t, uv, st = sc.Cast(None, rays, 0.0, T_MAX, 0, return_uv=True)
            for got, want, name in ((hit, wh, "hit"), (t, wt, "t"), (uv, wuv, "uv")):
                assert got.tobytes() == want.tobytes(), (n, occ, name)
            assert {k: st[k] for k in CAST} == {k: wst[k] for k in CAST}, (n, occ, st, wst)
            assert st["n_layers"] == bst["n_layers"] and st["n_pair_tests"] == bst["n_pair_tests"], (n, occ, st, bst)
            if occ == -1:      # no grid: the call's work, counter for counter
                assert st["n_lookups"] == bst["n_lookups"] and st["n_bit_tests"] == 0 and st["n_lookup_misses"] <= st["n_lookups"], (n, st, bst)
            else:
                assert st["n_bit_tests"] == bst["n_lookups"] and st["n_lookups"] <= bst["n_lookups"], (n, st, bst)
    # a ray's work does not depend on its neighbours: the tiled set's counters are the sums over the tiling
    rest = TILED % UNIQUE
    bst_rest = rec.RaycastMesh(None, tri, np.ascontiguousarray(unique[:rest]), 0.0, T_MAX, 0.0, 0)[-1]
    for k in WORK:
        assert work[TILED][k] == (TILED // UNIQUE) * work[UNIQUE][k] + bst_rest[k] > 0, (k, work[TILED], work[UNIQUE], bst_rest)
    print("%d rays: %d hit, %d layers, %d look-ups, %d pair tests" % (TILED, wst["n_hit"], *(work[TILED][k] for k in WORK)))
    assert wst["n_hit"] > TILED // 2
    for sc in scenes.values():
        sc.close()
    rec.close()
