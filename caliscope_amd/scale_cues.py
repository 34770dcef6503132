"""Metric cues that ``CaptureVolume.scaled()`` turns into one scale factor — the reference's ``core/scale_cues.py`` under the
same names, fields and default sigmas.  A solved volume is a shape: each cue says how long one thing in it really is."""

from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class CameraDistance:
    """Measured distance between the centres of two cameras, by cam_id."""

    cam_a: int
    cam_b: int
    meters: float
    sigma_m: float = 0.01


@dataclass(frozen=True)
class SegmentLength:
    """Known distance between two tracked keypoints (the median over the frames that have both is compared with it)."""

    keypoint_id_a: int
    keypoint_id_b: int
    meters: float
    sigma_m: float = 0.02


@dataclass(frozen=True)
class DepthObservation:
    """Metric depth of one keypoint in one camera at one sync index (output of a depth estimator, one per detection)."""

    cam_id: int
    keypoint_id: int
    sync_index: int
    depth_m: float
    sigma_m: float = 0.1
