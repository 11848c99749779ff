"""The scenario of tests/update_gather_cases.py reaches every kind of candidate the neighbour update can meet -- shown
with the oracle alone (no GPU); tests/test_gpu_update_gathers.py runs the same call through the HIP path."""
import numpy as np
import pytest

import update_gather_cases as ugc


@pytest.fixture(scope="module")
def scenario():
    return ugc.build()


def test_the_call_holds_slots_for_every_case(scenario):
    c = ugc.census(scenario)
    for name in ugc.CASES:
        assert c[name] >= 100, (name, c)
    # a share of the lanes that reach the gathers has nothing to evaluate, most have
    assert 0.1 * c["lanes"] < c["lanes_without_new_candidate"] < 0.5 * c["lanes"], c
    # (see the module's docstring: the supporting image cannot offer one slot the same surfel twice)
    assert c["twice"] == 0, c


def test_the_rewritten_links_are_what_the_groups_say(scenario):
    us = scenario
    links = us.rows.view(np.uint32)[19:23]
    after = us.snap.rows[19:23, :us.count].view(np.uint32)
    assert (links[:, us.groups["empty"]] == ugc.INVALID).all()
    assert (links[2:, us.groups["half_empty"]] == ugc.INVALID).all()
    g = us.groups["all_linked"]
    assert (links[:, g] != ugc.INVALID).all()
    # slots all of whose candidates are links get no new link (the call may still drop some: a replaced surfel loses its
    # links, and the regulariser that ends the call detaches merged surfels from their neighbours)
    assert ((after[:, g] == links[:, g]) | (after[:, g] == ugc.INVALID)).all()
    assert (after[:, g] == links[:, g]).all(0).mean() > 0.5
    # empty link slots were filled, far links replaced by nearer candidates
    assert (after[:, us.groups["empty"]] != ugc.INVALID).any(0).mean() > 0.8
    g = us.groups["far_links"]
    assert (after[:, g] != links[:, g]).any(0).mean() > 0.8
