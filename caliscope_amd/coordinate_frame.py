"""Z-up world basis from a vertical and a heading (reference ``core/coordinate_frame.py``)."""

from __future__ import annotations

import numpy as np


def world_basis_from_up_and_forward(up, *, forward) -> np.ndarray:
    """3 x 3 rotation whose rows are the world axes in source coordinates (``p_world = R @ p_source``): ``up`` normalised is +Z,
    the part of ``forward`` perpendicular to it is +Y, +X = Y x Z.  ``ValueError`` when that part is shorter than 1e-6."""
    z = np.asarray(up, dtype=np.float64)
    z = z / np.linalg.norm(z)
    flat = np.asarray(forward, dtype=np.float64)
    flat = flat - np.dot(flat, z) * z
    length = float(np.linalg.norm(flat))
    if length < 1e-6:
        raise ValueError("forward points along gravity (pitch ~ +/-90 deg); the forward-to-+Y yaw anchor is undefined")
    y = flat / length
    return np.stack([np.cross(y, z), y, z])
