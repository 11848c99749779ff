"""The per-pixel association record (Scratch::assoc: first depth, conflict key, count, supporting surfel in one 16-byte
store of the tile kernel) against the oracle's images, at image sizes that cut the association tiles (32 x 8 pixels):

  104 x 60       the last tile column is 8 pixels wide, the last tile row 4 pixels high: columns 4..107, rows 12..71
                 of a 112 x 84 stream, so that the cut tiles lie inside the border preprocessing leaves without depth;
  96 x 8         exactly one tile row: rows 36..43 of a 96 x 72 stream (no stream survives preprocessing at 8 rows).

A window is that part of the preprocessed images, with the principal point moved by the window's first column and row.

Eight frames of the synthetic stream with a vanishing obstacle (conflicts, replacements) are preprocessed by the oracle
once per size; both sides integrate the same images, and after EVERY call rows, counters, blended depth and all
association images -- FIRST_DEPTH and CONFLICTING among them, which the library now unpacks from the record -- must
equal the oracle's bit for bit, on the routes that read the record: the default, the all-slot scans (scan mode 1), the
multi-launch blend (2), and with pipelining off."""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as orc
from common import small_pre, small_stream
from oracle_pipeline import OraclePipeline
from test_gpu_parity import _compare_state

pytestmark = pytest.mark.gpu

CAPACITY = 20000
# the obstacle is in every depth image the outlier filter compares frames 4 and 5 with (f - 4 .. f + 4) and in none of
# those of frames 14..19: two calls put its surfels into the map, six look through them (conflicts, then replacements)
FRAMES = [4, 5, 14, 15, 16, 17, 18, 19]
OBSTACLE_UNTIL = 10
# name -> (width, height of the stream; first, end column and first, end row of the window both sides integrate)
SIZES = {"104x60": (112, 84, 4, 108, 12, 72), "96x8_one_tile_row": (96, 72, 0, 96, 36, 44)}


def _scenario(Ws, Hs, x0, x1, y0, y1, obstacle_until=OBSTACLE_UNTIL):
    """The calls (frame, pose, images) and the oracle's snapshot after each of them."""
    s = small_stream(Ws, Hs, obstacle_until=obstacle_until)
    pre = small_pre(Ws)
    params = orc.IntegrateParams.defaults()
    pp = OraclePipeline(Ws, Hs, s.fx, s.fy, s.cx, s.cy, 16, pre, params)   # (its preprocessing only)
    for f in range(min(FRAMES) - 4, max(FRAMES) + 5):
        pp.upload(f, *s.frame(f))
    W, H = x1 - x0, y1 - y0
    camera = (s.fx, s.fy, s.cx - x0, s.cy - y0)
    rec = orc.Recon(CAPACITY, W, H, *camera)
    calls, snaps = [], []
    for f in FRAMES:
        pp.preprocess(f, s.outlier_frames(f), s.others_TR_reference(f))
        band = lambda a: np.ascontiguousarray(a[y0:y1, x0:x1])   # noqa: E731
        call = SimpleNamespace(frame=f, pose=s.pose(f), depth=band(pp.depth_final), normals=band(pp.normals.reshape(Hs, Ws, 2)),
                               radius=band(pp.radius), color=band(pp.color[f]))
        depth = call.depth.copy()
        rec.integrate(f, pre.depth_scaling, depth, call.normals, call.radius, call.color, call.pose, params)
        n = rec.surfels_size
        snaps.append(SimpleNamespace(rows=rec.surfels()[:, :n].copy(), count=n, surfel_count=rec.surfel_count, depth=depth,
                                     scratch={k: v.copy() for k, v in rec.scratch().items()}, stats=rec.stats()))
        calls.append(call)
    rec.close()
    return SimpleNamespace(W=W, H=H, camera=camera, pre=pre, calls=calls, snaps=snaps)


@pytest.fixture(scope="module")
def scenarios():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _scenario(*SIZES[name])
        return cache[name]
    return get


def _oracle_side(snap):
    """What _compare_state reads of an OraclePipeline."""
    return SimpleNamespace(depth_final=snap.depth,
                           recon=SimpleNamespace(surfels_size=snap.count, surfel_count=snap.surfel_count, surfels=lambda: snap.rows,
                                                 scratch=lambda: dict(snap.scratch), stats=lambda: snap.stats))


@pytest.mark.parametrize("scan_mode,overlap", [(0, True), (2, True), (1, True), (0, False)],
                         ids=["default", "multi_launch_blend", "all_slot_scans", "no_pipelining"])
@pytest.mark.parametrize("size", list(SIZES))
def test_association_record_matches_the_oracle_after_every_call(smx, scenarios, size, scan_mode, overlap):
    from surfelmeshing_amd._lib import IntegrateParams
    from surfelmeshing_amd.pipeline import FramePipeline
    sc = scenarios(size)
    pg = FramePipeline(sc.W, sc.H, *sc.camera, CAPACITY, sc.pre, IntegrateParams.defaults())
    pg.reconstruction.set_scan_mode(scan_mode)
    pg.reconstruction.set_overlap(overlap)
    seen_conflicts = 0
    for k, (call, snap) in enumerate(zip(sc.calls, sc.snaps)):
        pg.color[k] = smx.CUDABuffer(sc.H, sc.W, np.uint8, 3)
        pg.filtered_A.Upload(call.depth)
        pg.normals.Upload(call.normals)
        pg.radius.Upload(call.radius)
        pg.color[k].Upload(call.color)
        pg.depth_final = pg.filtered_A
        pg.integrate_as(call.frame, k, call.pose)
        _compare_state(_oracle_side(snap), pg, check_scratch=True)
        # (named once more: these two no longer are images of the library's own)
        for name in ("first_depth", "conflicting"):
            assert np.array_equal(pg.reconstruction.debug_download_scratch(name), snap.scratch[name]), (name, call.frame)
        seen_conflicts += int(np.count_nonzero(snap.scratch["conflicting"] != 0xFFFFFFFF))
    # the inputs are worth the name: a map, supported pixels in the cut tiles, conflict keys, finite first depths
    last = sc.snaps[-1]
    assert last.count > (300 if sc.H == 8 else 1000), last.count
    assert seen_conflicts > 0
    sup = last.scratch["supporting"].reshape(sc.H, sc.W)
    assert (sup[:, sc.W - sc.W % 32:] != 0xFFFFFFFF).any() or sc.W % 32 == 0
    assert (sup[sc.H - sc.H % 8:, :] != 0xFFFFFFFF).any() or sc.H % 8 == 0
