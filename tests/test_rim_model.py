"""The model of smx_recon_mesh_rim against itself: rim() (np.unique over the sorted index pairs of R) equals rim_slow() (a
dictionary of pairs, one triangle at a time) on every case; the hand cases give the bytes written down beside them; the rim
edges are the boundary edges of smx_recon_fill_holes' model where the two calls keep the same triangles; and a census shows
that the cases reach every bit set and clear and every region of the distance call on a rim and on an interior feature."""
import numpy as np
import pytest

import distance_ref as dr
import fill_cases as fc
import fill_ref as fr
import mesh_ref as mr
import rim_ref as rf


def test_the_two_statements_agree_and_the_hand_cases_give_their_bytes():
    for name, pos, r2, tri, want, expect in rf.cases():
        got, st = rf.rim(pos, r2, tri)
        slow, sst = rf.rim_slow(pos, r2, tri)
        assert got.dtype == np.uint8 and got.shape == (tri.shape[0],) and got.tobytes() == slow.tobytes() and st == sst, name
        assert tuple(st) == rf.STAT_NAMES and int(got.max(initial=0)) < 64
        if want is not None:
            assert got.tolist() == want, (name, [hex(v) for v in got])
        for k, v in expect.items():
            assert st[k] == v, (name, k, st[k], v)
    pos, _, r2, tri, _ = dr.world()
    got, st = rf.rim(pos, r2, tri)
    slow, sst = rf.rim_slow(pos, r2, tri)
    assert got.tobytes() == slow.tobytes() and st == sst


def test_an_index_out_of_range_raises():
    for pos, r2, tri in rf.refused():
        with pytest.raises(ValueError):
            rf.rim(pos, r2, tri)


def test_the_input_order_and_the_winding_do_not_matter():
    pos, _, r2, tri, _ = dr.world()
    got, st = rf.rim(pos, r2, tri)
    perm = np.random.default_rng(2).permutation(tri.shape[0])
    again, ast = rf.rim(pos, r2, tri[perm])
    assert again.tobytes() == got[perm].tobytes() and ast == st
    # the other winding swaps B and C: bits 1 <-> 3 and 2 <-> 4
    flipped, fst = rf.rim(pos, r2, tri[:, [0, 2, 1]])
    g = got.astype(np.uint32)
    swapped = (g & 0x21) | ((g & 0x02) << 2) | ((g & 0x08) >> 2) | ((g & 0x04) << 2) | ((g & 0x10) >> 2)
    assert flipped.tolist() == swapped.tolist() and fst == st


def test_rim_edges_are_the_boundary_edges_of_the_fill_model():
    """Where no triangle is repeated or out of range both calls keep the triangles with live corners."""
    done = 0
    for name, pos, nrm, r2, tri, _ in fc.cases():
        _, st = rf.rim(pos, r2, tri)
        if st["n_repeated"] or st["n_out_of_range"]:
            continue
        wst = fr.fill(pos, nrm, r2, tri)[3]
        assert st["n_rim_edges"] == wst["n_boundary_edges"] and st["n_edges"] == wst["n_edges"] and st["n_not_live"] == wst["n_not_live"], name
        done += 1
    assert done >= 15
    pos, nrm, r2 = mr.sphere_map(n=1500)
    tri = mr.triangulate(pos, nrm, r2)[0]
    assert rf.rim(pos, r2, tri)[1]["n_rim_edges"] == fr.fill(pos, nrm, r2, tri)[3]["n_boundary_edges"] > 0


def test_census_every_bit_and_every_region_on_and_off_the_rim():
    bits_set, bits_clear = np.zeros(6, int), np.zeros(6, int)
    for name, pos, r2, tri, _, _ in rf.cases():
        got, _ = rf.rim(pos, r2, tri)
        R, t, _ = dr.classify(pos, r2, tri)
        for k in range(6):
            bits_set[k] += int(np.sum((got[t] >> k) & 1))
            bits_clear[k] += int(np.sum(1 - ((got[t] >> k) & 1)))
    print("bits set %s, clear %s" % (bits_set.tolist(), bits_clear.tolist()))
    assert np.all(bits_set > 50) and np.all(bits_clear > 50)
    # the regions the distance model reports for the points of its world, against the bytes of the world's triangles
    pos, _, r2, tri, _ = dr.world()
    got, _ = rf.rim(pos, r2, tri)
    on, off = np.zeros(7, int), np.zeros(7, int)
    for name in dr.point_sets():
        m = dr.model_of(name)
        ok = m["t"] != dr.INVALID
        byte, region = got[m["t"][ok].astype(np.int64)], m["region"][ok]
        h = np.array([rf.hit(b, r) for b, r in zip(byte, region)], bool)
        on += np.bincount(region[h], minlength=7)
        off += np.bincount(region[~h], minlength=7)
    print("regions hit on the rim %s, off it %s" % (on.tolist(), off.tolist()))
    assert np.all(on[:6] > 0) and on[6] == 0 and np.all(off > 0)
