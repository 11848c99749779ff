"""The occupancy bit grid and the filtered walk of the ray cast without a GPU: smx_rayscene.hpp holds what a kept scene needs of
the grid (which block sizes fit, the bit an entry sets), smx_raycast.hpp the grid's index function, the look-up with the bit
test in front of it, the walk that keeps the winner's (u, v, det) and one ray's view of the cast, ray_cast_one, as inline
functions.  This test compiles them for the host with the project's -ffp-contract=off into a stand-alone program (its own
main: it reads a case file and writes a result file; tests/ray_host.py holds it, and tests/test_raycast_kernel_host.py runs it
without a grid).  The program builds the index and the bit grid one "lane" after the other -- forwards and in a seeded shuffled
order -- and walks every ray with ray_cast_one, for the occupancy settings none, the smallest block that fits, k = 0 and k = 3.
Every output byte and statistic has to equal the brute-force model of tests/raycast_ref.py; the work counters have to stand in
the contract's relations to a walk of the same function with a k = -1 grid in the same program; every cell with entries has its
block's bit set, at k = 0 no other bit is set, and the set bits number the distinct blocks; with the early exit off every
candidate pair of the model is wide or lies in a cell whose table entry was looked up.  The same program is also built with
-fsanitize=address,undefined and run directly."""
import numpy as np
import pytest

import distance_ref as dr
import ray_host
import raycast_ref as rr
import rayscene_ref as sr
from ray_host import ORDERS


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("rayscene_host")


@pytest.fixture(scope="module")
def program(work):
    return ray_host.build(work, ray_host.RAY_PROGRAM, [], "rayscene_host")


@pytest.fixture(scope="module")
def sanitized(work):
    return ray_host.build(work, ray_host.RAY_PROGRAM, ray_host.SANITIZE, "rayscene_host_san")


def host_scene(exe, work, pos, r2, tri, rays, t_min, t_max, cell_size=0.0, cull=0, pairs=None, settings=sr.SETTINGS):
    """[(order, occupancy, rc, hit, t, uv, stats, extra)] for every order and setting."""
    return ray_host.host_scene(exe, work, pos, r2, tri, rays, t_min, t_max, cell_size, cull, pairs, settings)


def _compare(exe, work, world, model, rays, t0, t1, what, cell_size, cull, seen_k=None):
    pos, nrm, r2, tri, _ = world
    wh, wt, wuv, wst = rr.answer(model, cull)
    if cell_size > 0:
        wst.update(rr.structure(pos, r2, tri, cell_size))
    p = model["pairs"]
    pairs = p[np.argsort(p[:, 0], kind="stable")]
    found = set()
    for order, occ, rc, hit, tt, uv, st, extra in host_scene(exe, work, pos, r2, tri, rays, t0, t1, cell_size, cull, pairs):
        tag = (what, cell_size, cull, order, occ)
        assert rc == 0, tag
        used = st.pop("cell_size_used")
        g = sr.grid(pos, r2, tri, used)
        if cell_size > 0:
            assert used == float(rr.cell_used(cell_size))
        else:
            assert used >= float(rr.MIN_CELL)
            for k in ("n_wide", "n_entries", "n_cells"):
                st.pop(k)
        assert st == wst, (tag, st, wst)
        k = extra["k"]
        assert k == (-1 if occ == -1 else sr.smallest(g) if occ == 0 else occ - 1), tag
        if k >= 0:
            assert extra["n_blocks_set"] == sr.blocks_set(g, k) and extra["grid_bits"] == sr.bits(g, k), (tag, extra)
        for name in ("bits_wrong", "relations_wrong", "pairs_missed", "exit_differs", "kept_differs"):
            assert extra[name] == 0, (tag, extra)
        assert extra["bit_tests"] == (extra["base_lookups"] if k >= 0 else 0) and extra["found"] == extra["lookups"] - extra["misses"], (tag, extra)
        found.add(extra["found"])
        for got, want in ((hit, wh), (tt, wt), (uv, wuv)):
            assert got.tobytes() == want.tobytes(), tag
        if order == ORDERS[0]:
            if seen_k is not None:
                seen_k.add(k)
            print("%s cell %g cull %d occupancy %d: k = %d, %d blocks set; %d bit tests, %d look-ups (%d without a grid), %d misses" % (
                what, cell_size, cull, occ, k, extra["n_blocks_set"], extra["bit_tests"], extra["lookups"], extra["base_lookups"], extra["misses"]))
    assert len(found) == 1, (what, cell_size, cull, found)       # look-ups that found a run: the same for every setting


def test_every_ray_set_on_the_host(program, work):
    world = dr.world()
    seen_k = set()
    for k, (name, (rays, t0, t1)) in enumerate(rr.ray_sets().items()):
        m = rr.model_of(name)
        for j, cs in enumerate(rr.CELL_SIZES):
            _compare(program, work, world, m, rays, t0, t1, name, cs, (k + j) % 3, seen_k)
    assert 0 in seen_k and any(k > 0 for k in seen_k) and -1 in seen_k, seen_k


def test_every_cull_mode_on_the_host(program, work):
    world = dr.world()
    for name in ("around the hand-made triangles", "inside-out"):
        rays, t0, t1 = rr.ray_sets()[name]
        for cull in (0, 1, 2):
            _compare(program, work, world, rr.model_of(name), rays, t0, t1, name, 0.0225, cull)


def test_a_block_size_that_does_not_fit_an_index_out_of_range_and_empty_inputs(program, work):
    pos, nrm, r2, tri, _ = dr.world()
    rays, t0, t1 = rr.ray_sets()["BAD and limits"]
    bad = tri.copy()
    bad[77, 2] = pos.shape[0]
    assert [r[2] for r in host_scene(program, work, pos, r2, bad, rays, t0, t1)] == [-1] * (len(ORDERS) * len(sr.SETTINGS))
    none = np.zeros((0, 3), np.uint32)
    n_bad = int(rr.bad_rays(rays).sum())
    for order, occ, rc, hit, tt, uv, st, extra in host_scene(program, work, pos, r2, none, rays, t0, t1):
        assert rc == 0 and np.all(hit == rr.INVALID) and np.all(np.isinf(tt)) and np.all(np.isnan(uv))
        assert st["n_hit"] == 0 and st["n_bad_rays"] == n_bad and st["n_entries"] == 0 and extra["n_blocks_set"] == 0 and extra["bit_tests"] == 0
        assert extra["k"] == (occ - 1 if occ > 0 else -1)
    for order, occ, rc, hit, tt, uv, st, extra in host_scene(program, work, pos, r2, tri, np.zeros((0, 6), np.float32), 0.0, 1.0, 0.2):
        assert rc == 0 and hit.size == 0 and st["n_rays"] == 0 and st["n_entries"] == rr.structure(pos, r2, tri, 0.2)["n_entries"]
    # two small triangles 120 m apart at the smallest cell: 2^33 bits at k = 5 (refused), below 2^31 at k = 6, which is the smallest that fits
    f = np.float32
    corner = np.array([[0, 0, 0], [0.001, 0, 0], [0, 0.001, 0]], f)
    far = np.concatenate([corner - f(59.99), corner + f(59.99)])
    far_r2, far_tri = np.full(6, 1e-4, f), np.array([[0, 1, 2], [3, 4, 5]], np.uint32)
    far_rays = np.array([[-59.9897, -59.9897, -50.0, 0, 0, -1], [59.9903, 59.9903, 50.0, 0, 0, 1], [0, 0, 0, 1, -1, 0.5]], f)
    want = rr.answer(rr.brute(far, far_r2, far_tri, far_rays, 0.0, 100.0), 0)
    assert want[3]["n_hit"] == 2
    g = sr.grid(far, far_r2, far_tri, 2.0 ** -9)
    assert not sr.fits(g, 5) and sr.fits(g, 6)
    for order, occ, rc, hit, tt, uv, st, extra in host_scene(program, work, far, far_r2, far_tri, far_rays, 0.0, 100.0, 2.0 ** -9, 0, None, (1, 6, 7, 0, -1)):
        assert rc == (-3 if occ in (1, 6) else 0), (occ, rc)
        if rc == 0:
            assert extra["k"] == (6 if occ in (7, 0) else -1) and extra["bits_wrong"] == 0 and extra["relations_wrong"] == 0
            assert hit.tobytes() == want[0].tobytes() and tt.tobytes() == want[1].tobytes() and uv.tobytes() == want[2].tobytes()
            if extra["k"] == 6:
                assert extra["n_blocks_set"] == sr.blocks_set(g, 6) == 2 and extra["grid_bits"] == sr.bits(g, 6)


def test_the_program_under_the_sanitizers(sanitized, work):
    """Run directly, as a program of its own: address and undefined-behaviour sanitizers on the header's host code."""
    world = dr.world()
    for name, cs, cull in (("around the hand-made triangles", 0.0, 0), ("BAD and limits", 2.0 ** -9, 0), ("BAD and limits", 0.2, 1),
                           ("axis rays", 0.0225, 2), ("t_min = t_max", 0.2, 0)):
        rays, t0, t1 = rr.ray_sets()[name]
        _compare(sanitized, work, world, rr.model_of(name), rays, t0, t1, name + ", sanitized", cs, cull)
