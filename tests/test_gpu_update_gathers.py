"""The neighbour update gathers records only for candidates that can change a link (relink, smx_recon.hip).  The call of
tests/update_gather_cases.py -- one Integrate call on a crafted map with slots for every kind of candidate, shown by
tests/test_update_gather_cases.py on the CPU -- through the HIP path: the map is injected with debug_upload_surfels, and
after the call EVERY row (the link rows 19..22 among them), the association images, the blended depth and the counters
must equal the oracle's bit for bit.  Routes: the visible list (default), the all-slot scan (scan mode 1), and the
gathers without range-checked buffers that capacities from 2^28 slots take (scan mode 1024), alone and with the scan."""
from types import SimpleNamespace

import numpy as np
import pytest

import decision_maps as dm
import update_gather_cases as ugc
from test_gpu_parity import _compare_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenario():
    return ugc.build()


@pytest.mark.parametrize("scan_mode", [0, 1, 1024, 1025])
def test_links_match_the_oracle_after_the_call(smx, scenario, scan_mode):
    from surfelmeshing_amd._lib import IntegrateParams
    from surfelmeshing_amd.pipeline import FramePipeline
    us = scenario
    call, snap = us.call, us.snap
    pg = FramePipeline(dm.W, dm.H, *us.camera, us.capacity, us.pre, IntegrateParams.defaults())
    pg.reconstruction.set_scan_mode(scan_mode)
    pg.reconstruction.debug_upload_surfels(us.rows, us.merge_count)
    assert pg.reconstruction.surfels_size() == us.count
    pg.color[0] = smx.CUDABuffer(dm.H, dm.W, np.uint8, 3)
    pg.filtered_A.Upload(call.depth)
    pg.normals.Upload(call.normals)
    pg.radius.Upload(call.radius)
    pg.color[0].Upload(call.color)
    pg.depth_final = pg.filtered_A
    pg.integrate_as(call.frame, 0, call.pose)
    got = pg.reconstruction.debug_download_surfels(snap.count)
    assert np.array_equal(got[19:23, :snap.count].view(np.uint32), snap.rows[19:23].view(np.uint32)), "link rows"
    oracle_side = SimpleNamespace(depth_final=snap.depth,
                                  recon=SimpleNamespace(surfels_size=snap.count, surfel_count=snap.surfel_count, surfels=lambda: snap.rows,
                                                        scratch=lambda: dict(snap.scratch), stats=lambda: snap.stats))
    _compare_state(oracle_side, pg, check_scratch=True)
