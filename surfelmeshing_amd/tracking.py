"""Camera tracking for a frame loop that comes without a trajectory: frame-to-model ICP of every new frame against the
surfel map (CUDASurfelReconstruction.Track / smx_recon_track), a constant-velocity prediction, and the policy for frames
that cannot be tracked.

Host plumbing around the C-ABI calls; all computing happens in libsmx.so.  The Tracker preprocesses a frame for
tracking into buffers of its own -- the call sequence of FramePipeline.preprocess(f, [], None): bilateral filter,
erosion, normals, radii, and NO outlier cull, because the cull needs the poses of later frames, which tracking is
there to find -- so it does not disturb the images the pipeline integrates.
"""
import numpy as np

from . import api
from ._lib import TrackParams, TrackRGBDParams

_BOTTOM = np.array([[0.0, 0.0, 0.0, 1.0]])


def _to44(T):
    return np.concatenate([np.asarray(T, np.float64).reshape(3, 4), _BOTTOM], axis=0)


def constant_velocity_prediction(previous, last):
    """pred = last . (previous^-1 . last) as a 3 x 4 float32; `last` itself while there is no previous pose."""
    if previous is None:
        return np.asarray(last, np.float32).reshape(3, 4).copy()
    P, L = _to44(previous), _to44(last)
    return (L @ np.linalg.inv(P) @ L)[:3].astype(np.float32)


class Tracker:
    """Tracks the frames of a FramePipeline against its map.

        tracker = Tracker(pipeline)
        tracker.set_pose(0, start_pose)              # the first frame: known (or the identity)
        outcome = tracker.track(f)                   # frames uploaded to the pipeline, in order
        pose = tracker.poses[f]

    Policy for a bad status (outcome.ok is False): the frame keeps the prediction, its index goes to `lost`, and the next
    prediction starts from it.  `outcomes` keeps the TrackOutcome of every tracked frame.

    rgbd=True tracks with the photometric term as well (TrackRGBD / smx_recon_track_rgbd, params a TrackRGBDParams): the
    colour image is the one the pipeline holds for the frame.  The policy is the same."""

    def __init__(self, pipeline, params=None, rgbd=False):
        self.pipeline = pipeline
        self.rgbd = bool(rgbd)
        if params is None:
            params = TrackRGBDParams.defaults() if self.rgbd else TrackParams.defaults()
        if isinstance(params, TrackRGBDParams) != self.rgbd:
            raise TypeError("params must be a %s" % ("TrackRGBDParams" if self.rgbd else "TrackParams"))
        self.params = params
        h, w = pipeline.h, pipeline.w
        self.filtered_A = api.CUDABuffer(h, w, np.uint16)
        self.filtered_B = api.CUDABuffer(h, w, np.uint16)
        self.normals = api.CUDABuffer(h, w, np.float32, 2)
        self.radius = api.CUDABuffer(h, w, np.float32)
        self.radius.Clear(0.0, pipeline.stream)
        self.poses = {}
        self.outcomes = {}
        self.lost = []
        self._order = []

    def set_pose(self, frame_index, global_T_frame):
        self.poses[frame_index] = np.asarray(global_T_frame, np.float32).reshape(3, 4).copy()
        self._order.append(frame_index)

    def preprocess(self, frame_index):
        """FramePipeline.preprocess(frame_index, [], None) into the tracker's own buffers: (depth, normals)."""
        pl = self.pipeline
        s, p = pl.stream, pl.pre
        api.BilateralFilteringAndDepthCutoffCUDA(
            s, p.bilateral_filter_sigma_xy, p.bilateral_filter_sigma_depth_factor, 0,
            p.bilateral_filter_radius_factor, p.max_depth_u16(), p.depth_valid_region_radius,
            pl.raw_depth[frame_index], self.filtered_A)
        src, dst = self.filtered_A, self.filtered_B
        if p.depth_erosion_radius > 0:
            api.ErodeDepthMapCUDA(s, p.depth_erosion_radius, src, dst)
        else:
            api.CopyWithoutBorderCUDA(s, src, dst)
        src, dst = dst, src
        api.ComputeNormalsAndDropBadPixelsCUDA(s, p.observation_angle_threshold_deg, p.depth_scaling, pl.fx, pl.fy,
                                               pl.cx, pl.cy, src, dst, self.normals)
        src, dst = dst, src
        api.ComputePointRadiiAndRemoveIsolatedPixelsCUDA(s, p.point_radius_extension_factor,
                                                         p.point_radius_clamp_factor, p.depth_scaling, pl.fx,
                                                         pl.fy, pl.cx, pl.cy, src, self.radius, dst)
        return dst, self.normals

    def predict(self):
        if not self._order:
            raise ValueError("no pose yet: call set_pose for the first frame")
        last = self.poses[self._order[-1]]
        previous = self.poses[self._order[-2]] if len(self._order) > 1 else None
        return constant_velocity_prediction(previous, last)

    def track(self, frame_index, prediction=None):
        """Tracks frame `frame_index` (uploaded to the pipeline) against the map as it stands; records and returns the
        TrackOutcome.  The pose kept for the frame is outcome.global_T_frame, or the prediction on a bad status."""
        pred = np.asarray(prediction, np.float32).reshape(3, 4) if prediction is not None else self.predict()
        depth, normals = self.preprocess(frame_index)
        pl = self.pipeline
        if self.rgbd:
            out = pl.reconstruction.TrackRGBD(pl.stream, pl.pre.depth_scaling, depth, normals, pl.color[frame_index], pred,
                                              self.params)
        else:
            out = pl.reconstruction.Track(pl.stream, pl.pre.depth_scaling, depth, normals, pred, self.params)
        self.outcomes[frame_index] = out
        if out.ok:
            pose = out.global_T_frame
        else:
            pose = pred
            self.lost.append(frame_index)
        self.set_pose(frame_index, pose)
        return out

    def trajectory(self):
        """[(frame index, 3 x 4 pose)] in tracking order."""
        return [(f, self.poses[f]) for f in self._order]

    def close(self):
        for b in (self.filtered_A, self.filtered_B, self.normals, self.radius):
            b.close()
