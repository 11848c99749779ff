"""The arithmetic, the index and the traversal of smx_raycast.hip without a GPU: smx_raycast.hpp holds the BAD test of a ray, the
candidate test of step 3 with its key, the inflated box of a triangle, the dominant axis and its layers, the t interval and the
cell rectangle of a layer, the exit test and the walk of one ray as inline functions (the classes, the cell table and its
operations come from smx_trigrid.hpp).  This test compiles them for the host with the project's -ffp-contract=off into a
stand-alone program (its own main: it reads a case file and writes a result file; tests/ray_host.py holds it, and
tests/test_rayscene_kernel_host.py runs it with the occupancy grids) and walks mark, index, cast and stats one "lane" after the
other -- forwards and in a seeded shuffled order -- with plain words behind the table operations and no grid in front of the
table, which is the index smx_recon_raycast_mesh casts.  Every output byte and every statistic has to equal the brute-force
model of tests/raycast_ref.py, as on the device, for every ray set and every cell size.  With the early exit off the program
also checks, for EVERY candidate (ray, triangle) pair of the model and not only the winners, that the triangle is on the wide
list or entered in a cell the walk looked up.  For every hit the key recomputed from the map positions of the winning triangle
has to equal the walk's key, and the recomputed u, v and sign of det what the walk kept, bit for bit: the kernel writes the kept
values and reads no map.  smx_raycast.hpp is also compiled by itself for the host.  The same program is also built with -fsanitize=address,undefined and run directly."""
import numpy as np
import pytest

import distance_ref as dr
import ray_host
import raycast_ref as rr
from ray_host import ORDERS


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("raycast_host")


@pytest.fixture(scope="module")
def program(work):
    ray_host.build(work, ray_host.ALONE, [], "raycast_alone")
    return ray_host.build(work, ray_host.RAY_PROGRAM, [], "raycast_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return ray_host.build(work, ray_host.RAY_PROGRAM, ray_host.SANITIZE, "raycast_host_san")


def host_raycast(exe, work, pos, r2, tri, rays, t_min, t_max, cell_size=0.0, cull=0, pairs=None):
    """[(rc, hit, t, uv, stats, extra)] for every order: the program without a grid."""
    runs = ray_host.host_scene(exe, work, pos, r2, tri, rays, t_min, t_max, cell_size, cull, pairs, (-1,))
    assert [(order, occ) for order, occ, *_ in runs] == [(order, -1) for order in ORDERS]
    for _, _, rc, *_, extra in runs:          # no grid: no bit is tested, and the walk is the walk beside it
        assert rc != 0 or extra["k"] == -1 and extra["bit_tests"] == 0 and extra["lookups"] == extra["base_lookups"] and extra["relations_wrong"] == 0
    return [run[2:] for run in runs]


def _pairs_for(model, cull):
    """The candidate pairs of the model under `cull`, ascending by ray.  (The side of a pair is not kept, so cull 1 / 2 check the
    pairs of cull 0: a superset, which the walk with the exit off has to cover just the same.)"""
    p = model["pairs"]
    return p[np.argsort(p[:, 0], kind="stable")]


def _compare(exe, work, world, model, rays, t0, t1, what, cell_size, cull):
    pos, nrm, r2, tri, _ = world
    wh, wt, wuv, wst = rr.answer(model, cull)
    if cell_size > 0:
        wst.update(rr.structure(pos, r2, tri, cell_size))
    pairs = _pairs_for(model, cull)
    differing = 0
    for order, (rc, hit, tt, uv, st, extra) in zip(ORDERS, host_raycast(exe, work, pos, r2, tri, rays, t0, t1, cell_size, cull, pairs)):
        assert rc == 0
        used = st.pop("cell_size_used")
        if cell_size > 0:
            assert used == float(rr.cell_used(cell_size))
        else:
            assert used >= float(rr.MIN_CELL)
            for k in ("n_wide", "n_entries", "n_cells"):
                st.pop(k)
        assert st == wst, (what, order, st, wst)
        assert extra["pairs_missed"] == 0 and extra["exit_differs"] == 0 and extra["kept_differs"] == 0, (what, order, extra)
        differing += sum(int(a.tobytes() != b.tobytes()) for a, b in ((hit, wh), (tt, wt), (uv, wuv)))
    print("%s cell %g cull %d: %d hit, %d candidate pairs all met, %.2f cells per layer (%d layers, %d with the exit off), %d differing arrays"
          % (what, cell_size, cull, wst["n_hit"], pairs.shape[0], extra["lookups_full"] / max(1, extra["layers_full"]), extra["layers"],
             extra["layers_full"], differing))
    assert differing == 0, what


def test_every_ray_set_on_the_host(program, work):
    world = dr.world()
    for k, (name, (rays, t0, t1)) in enumerate(rr.ray_sets().items()):
        m = rr.model_of(name)
        for j, cs in enumerate(rr.CELL_SIZES):
            _compare(program, work, world, m, rays, t0, t1, name, cs, (k + j) % 3)


def test_every_cull_mode_on_the_host(program, work):
    world = dr.world()
    for name in ("around the hand-made triangles", "inside-out"):
        rays, t0, t1 = rr.ray_sets()[name]
        for cull in (0, 1, 2):
            _compare(program, work, world, rr.model_of(name), rays, t0, t1, name, 0.0225, cull)


def test_an_index_out_of_range_and_empty_inputs_on_the_host(program, work):
    pos, nrm, r2, tri, _ = dr.world()
    rays, t0, t1 = rr.ray_sets()["BAD and limits"]
    bad = tri.copy()
    bad[77, 2] = pos.shape[0]
    assert [r[0] for r in host_raycast(program, work, pos, r2, bad, rays, t0, t1)] == [-1, -1]
    none = np.zeros((0, 3), np.uint32)
    n_bad = int(rr.bad_rays(rays).sum())
    for rc, hit, tt, uv, st, extra in host_raycast(program, work, pos, r2, none, rays, t0, t1):
        assert rc == 0 and np.all(hit == rr.INVALID) and np.all(np.isinf(tt)) and np.all(np.isnan(uv))
        assert st["n_hit"] == 0 and st["n_bad_rays"] == n_bad and st["n_entries"] == 0
    for rc, hit, tt, uv, st, extra in host_raycast(program, work, pos, r2, tri, np.zeros((0, 6), np.float32), 0.0, 1.0, 0.2):
        assert rc == 0 and hit.size == 0 and st["n_rays"] == 0 and st["n_entries"] == rr.structure(pos, r2, tri, 0.2)["n_entries"]


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code."""
    world = dr.world()
    for name, cs, cull in (("around the hand-made triangles", 0.0, 0), ("BAD and limits", 2.0 ** -9, 0), ("BAD and limits", 0.2, 1),
                           ("axis rays", 0.0225, 2), ("t_min = t_max", 0.2, 0)):
        rays, t0, t1 = rr.ray_sets()[name]
        _compare(sanitized, work, world, rr.model_of(name), rays, t0, t1, name + ", sanitized", cs, cull)
