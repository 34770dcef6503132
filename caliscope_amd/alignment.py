"""Similarity transforms of a calibrated volume: ``target = s R source + t`` — host-side mirror of the reference's
``core/alignment.py`` (same names, checks and messages).  O(cameras) and one pass over the points; nothing here is device work."""

from __future__ import annotations

import logging
from dataclasses import dataclass, replace

import numpy as np

from caliscope_amd.cameras import CameraArray
from caliscope_amd.point_data import WorldPoints

logger = logging.getLogger(__name__)


@dataclass(frozen=True)
class SimilarityTransform:
    """``rotation`` (3 x 3, det +1), ``translation`` (3,) in target units, ``scale`` (> 0, target units per source unit)."""

    rotation: np.ndarray
    translation: np.ndarray
    scale: float

    def __post_init__(self):
        if self.rotation.shape != (3, 3):
            raise ValueError(f"Rotation must be 3x3, got {self.rotation.shape}")
        det = np.linalg.det(self.rotation)
        if not np.isclose(det, 1.0, atol=1e-6):
            raise ValueError(f"Rotation must be proper (det=+1), got det={det:.6f}")
        if not np.allclose(self.rotation @ self.rotation.T, np.eye(3), atol=1e-6):
            raise ValueError("Rotation matrix must be orthogonal")
        if self.translation.shape != (3,):
            raise ValueError(f"Translation must be 3-vector, got {self.translation.shape}")
        if self.scale <= 0:
            raise ValueError(f"Scale must be positive, got {self.scale}")

    def apply(self, points: np.ndarray) -> np.ndarray:
        """``s R p + t`` for every row of an N x 3 array."""
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError(f"Points must be Nx3 array, got shape {points.shape}")
        return self.scale * (self.rotation @ points.T).T + self.translation

    @property
    def inverse(self) -> "SimilarityTransform":
        rot, scale = self.rotation.T, 1.0 / self.scale
        return SimilarityTransform(rot, -scale * (rot @ self.translation), scale)

    @property
    def matrix(self) -> np.ndarray:
        """4 x 4 homogeneous form ``[[s R, t], [0, 1]]``."""
        out = np.eye(4, dtype=np.float64)
        out[:3, :3] = self.scale * self.rotation
        out[:3, 3] = self.translation
        return out


def estimate_similarity_transform(source_points: np.ndarray, target_points: np.ndarray, *, rigid: bool = False) -> SimilarityTransform:
    """Least-squares ``s, R, t`` of ``target ~ s R source + t`` (Umeyama); ``rigid`` fixes ``s = 1``.  A reflection is turned into
    a rotation by flipping the last row of ``Vt``, as the reference does."""
    if source_points.shape != target_points.shape:
        raise ValueError(f"Point arrays must have same shape, got {source_points.shape} and {target_points.shape}")
    if source_points.shape[0] < 3:
        raise ValueError(f"Need at least 3 points for similarity transform, got {source_points.shape[0]}")
    if source_points.shape[1] != 3:
        raise ValueError(f"Points must be 3D (Nx3), got shape {source_points.shape}")
    if np.any(np.isnan(source_points)) or np.any(np.isnan(target_points)):
        raise ValueError("Input points cannot contain NaN values")
    src_mean, dst_mean = np.mean(source_points, axis=0), np.mean(target_points, axis=0)
    src, dst = source_points - src_mean, target_points - dst_mean
    U, _, Vt = np.linalg.svd(src.T @ dst)
    if np.linalg.det(Vt.T @ U.T) < 0:
        Vt[-1, :] *= -1
    rotation = Vt.T @ U.T
    scale = 1.0 if rigid else np.sum(dst * (rotation @ src.T).T) / np.sum(src**2)
    translation = dst_mean - scale * (rotation @ src_mean)
    try:
        return SimilarityTransform(rotation, translation, float(scale))
    except ValueError as e:
        raise RuntimeError(f"Estimated transform is invalid: {e}")


def apply_similarity_transform(camera_array: CameraArray, world_points: WorldPoints, transform: SimilarityTransform):
    """``(new CameraArray, new WorldPoints)`` in the target frame; the inputs are not touched.  Points: ``s R X + t``.  A posed
    camera keeps looking at the same points: centre ``C' = s R C + t``, ``R_cam' = R_cam R^T`` (a rotation: the scale must not get
    into it), ``t' = -R_cam' C'``.  Cameras without a pose, and every other camera field, are carried over."""
    new_points = world_points.with_points(transform.apply(world_points.points))
    cameras = {}
    for cam_id, cam in camera_array.cameras.items():
        new = replace(cam, rotation=None, translation=None)
        if cam.rotation is not None and cam.translation is not None:
            centre = transform.scale * (transform.rotation @ (-cam.rotation.T @ cam.translation)) + transform.translation
            new.rotation = cam.rotation @ transform.rotation.T
            new.translation = -new.rotation @ centre
        cameras[cam_id] = new
    return CameraArray(cameras=cameras), new_points
