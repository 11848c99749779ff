"""The crafted map of tests/decision_maps.py through the HIP path: the state is injected with debug_upload_surfels, the
edited images are written into the pipeline's buffers, and after EVERY call the rows, the association images, the
blended depth and the counters must equal the oracle's bit for bit.  tests/test_decision_maps.py shows on the CPU that
these calls take both sides of the twelve decisions no stream reaches."""
from types import SimpleNamespace

import numpy as np
import pytest

import decision_maps as dm
from test_gpu_parity import _compare_state

pytestmark = pytest.mark.gpu


class _OracleSide:
    """What _compare_state reads of an OraclePipeline, served from a snapshot of decision_maps.run_oracle."""

    def __init__(self, snap):
        s = snap
        self.depth_final = s.depth
        self.recon = SimpleNamespace(surfels_size=s.count, surfel_count=s.surfel_count, surfels=lambda: s.rows,
                                     scratch=lambda: {k: v for k, v in s.scratch.items()}, stats=lambda: s.stats)


@pytest.fixture(scope="module")
def scenario():
    sc = dm.build()
    return sc, dm.run_oracle(sc)


def _pipeline(sc, scan_mode=0, overlap=None):
    from surfelmeshing_amd.pipeline import FramePipeline
    from surfelmeshing_amd._lib import IntegrateParams
    fx, fy, cx, cy = sc.camera
    pg = FramePipeline(dm.W, dm.H, fx, fy, cx, cy, sc.capacity, sc.pre, IntegrateParams.defaults())
    pg.reconstruction.set_scan_mode(scan_mode)
    if overlap is not None:
        pg.reconstruction.set_overlap(overlap)
    pg.reconstruction.debug_upload_surfels(sc.rows, sc.merge_count)
    assert pg.reconstruction.surfels_size() == sc.count
    return pg


def _run_call(smx, pg, k, call, own_buffers=False):
    """Writes the call's images into the pipeline's buffers (depth into filtered_A, which the call blends in place;
    normals, radius, and the colour under the call's position in the list) and runs it.  own_buffers: into buffers of
    the call's own instead, kept by the pipeline, so that nothing has to be waited for between two calls."""
    if call.kind == "regularize":
        pg.reconstruction.Regularize(None, call.frame, call.weight, call.radius_factor, call.window)
        return
    if own_buffers:
        pg.kept = getattr(pg, "kept", []) + [(pg.filtered_A, pg.normals, pg.radius)]
        pg.filtered_A = smx.CUDABuffer(dm.H, dm.W, np.uint16)
        pg.normals, pg.radius = smx.CUDABuffer(dm.H, dm.W, np.float32, 2), smx.CUDABuffer(dm.H, dm.W, np.float32)
    pg.color[k] = smx.CUDABuffer(dm.H, dm.W, np.uint8, 3)
    pg.filtered_A.Upload(call.depth)
    pg.normals.Upload(call.normals)
    pg.radius.Upload(call.radius)
    pg.color[k].Upload(call.color)
    pg.depth_final = pg.filtered_A
    pg.integrate_as(call.frame, k, call.pose)


@pytest.mark.parametrize("scan_mode", [0, 1, 8 + 16, 96, 256, 512])
def test_decision_maps_match_the_oracle_after_every_call(smx, scenario, scan_mode):
    """Scan modes that change the route a surfel takes (see test_stream_parity_every_frame)."""
    sc, snaps = scenario
    pg = _pipeline(sc, scan_mode)
    for k, (call, snap) in enumerate(zip(sc.calls, snaps)):
        _run_call(smx, pg, k, call)
        _compare_state(_OracleSide(snap), pg, check_scratch=call.kind == "integrate")
    assert snaps[-1].count > 40000


@pytest.mark.parametrize("overlap", [True, False])
def test_decision_maps_with_pipelining_on_and_off(smx, scenario, overlap):
    """Every call is compared as above; a last pass runs all calls with nothing read back in between, so that with
    pipelining on the regulariser of a call really runs beside the front of the next."""
    sc, snaps = scenario
    pg = _pipeline(sc, overlap=overlap)
    for k, (call, snap) in enumerate(zip(sc.calls, snaps)):
        _run_call(smx, pg, k, call)
        _compare_state(_OracleSide(snap), pg, check_scratch=call.kind == "integrate")
    pg = _pipeline(sc, overlap=overlap)
    for k, call in enumerate(sc.calls):
        _run_call(smx, pg, k, call, own_buffers=True)
    _compare_state(_OracleSide(snaps[-1]), pg)
