"""Per-camera vertical (up vector) from perspective fields: what feeds ``CaptureVolume.oriented``.

Host-side mirror of the reference's ``estimators/vertical_solver.py`` and of the numeric half of ``estimators/vertical.py`` under
the same names: :class:`GravityFit`, :func:`gravity_vec_from_roll_pitch`, :func:`roll_pitch_from_gravity_vec`, :func:`fit_gravity`,
:class:`VerticalEstimate` and :func:`sample_frame_indices`.  The field network, its weights, video decoding and the image
preprocessing are not part of this package: the feature starts where the network's four output fields exist as arrays.
:func:`estimate_vertical_from_fields` takes those fields for the sampled frames of every camera and returns the per-camera up
vectors and their frame-to-frame spread, aggregated as the reference aggregates them.

Where the work runs: every fit is a 2-DOF Levenberg-Marquardt on the unit sphere over four dense fields.  All fits of a call —
every frame of every camera, of any mix of shapes — go to the device in one call, ``cba_vertical_fit`` (``csrc/vertical_math.h``,
``csrc/vertical_lib.hip``): one pass over the pixels per step, FP64, sums in a fixed order, so a fit does not depend on the rest of
the batch.  There is no CPU fallback: without the library or a GPU the call raises ``BackendError``.  ``_solver`` replaces the device
call (an object with ``vertical_fit``, as :class:`DeviceVerticalFit`) — the CPU test-suite passes a g++ build of the same header.

Errors.  A fit whose final Hessian is exactly singular (all-zero confidences reach it) raises ``numpy.linalg.LinAlgError``, as the
reference's ``np.linalg.inv`` does.  A fit whose first cost is not finite (NaN or infinity in a field) raises ``ValueError``: a
deviation, the reference's behaviour there is undefined.  Mismatched shapes, a height or width below 2 and non-positive focal
lengths raise ``ValueError`` before anything is sent.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from caliscope_amd import _lib
from caliscope_amd.exceptions import BackendError

DEFAULT_NUM_STEPS = 30
FIELD_NAMES = ("up_field", "up_confidence", "latitude_field", "latitude_confidence")
STATUS_OK, STATUS_NONFINITE, STATUS_SINGULAR = 0, 1, 2


@dataclass(frozen=True)
class GravityFit:
    """The solver's result: gravity angles, Hessian uncertainties, run evidence."""

    roll_rad: float
    pitch_rad: float
    roll_uncertainty_rad: float
    pitch_uncertainty_rad: float
    gravity_uncertainty_rad: float
    initial_cost: float
    final_cost: float
    stop_step: int


@dataclass(frozen=True)
class VerticalEstimate:
    """Per-camera up vectors with a frame-to-frame stability diagnostic: ``up_per_cam`` maps cam_id to a unit up vector in that
    camera's frame (OpenCV convention, ``[0, -1, 0]`` for a level camera), the normalised mean over the sampled frames;
    ``spread_per_cam`` maps cam_id to the median angular deviation (degrees) of the per-frame up vectors from that mean."""

    up_per_cam: dict
    spread_per_cam: dict


def gravity_vec_from_roll_pitch(roll_rad: float, pitch_rad: float) -> np.ndarray:
    """Unit up vector in the OpenCV camera frame; [0, -1, 0] for a level camera."""
    sin_roll, cos_roll = np.sin(roll_rad), np.cos(roll_rad)
    sin_pitch, cos_pitch = np.sin(pitch_rad), np.cos(pitch_rad)
    return np.array([-sin_roll * cos_pitch, -cos_roll * cos_pitch, sin_pitch], dtype=np.float64)


def roll_pitch_from_gravity_vec(vec) -> tuple[float, float]:
    """Angles back out of the vector; a camera rolled beyond +/-90 degrees (y >= 0) takes the reflected branch."""
    eps = 1e-4
    x, y, z = float(vec[0]), float(vec[1]), float(vec[2])
    pitch = float(np.arcsin(np.clip(z, -1.0, 1.0)))
    roll = float(np.arcsin(np.clip(-x / (np.sqrt(max(1 - z**2, 0.0)) + eps), -1.0, 1.0)))
    if y >= 0:
        roll = -roll - np.pi * np.sign(x)
    return roll, pitch


def sample_frame_indices(num_frames: int, num_samples: int) -> tuple[int, ...]:
    """Evenly spaced frame indices covering the whole clip, first and last included, unique and ascending; a clip shorter than
    ``num_samples`` returns every frame."""
    if num_frames <= 0:
        raise ValueError(f"num_frames must be positive, got {num_frames}")
    if num_samples <= 0:
        raise ValueError(f"num_samples must be positive, got {num_samples}")
    if num_samples >= num_frames:
        return tuple(range(num_frames))
    spaced = np.linspace(0, num_frames - 1, num_samples).round().astype(int)
    return tuple(int(i) for i in np.unique(spaced))


# ---- the device call -------------------------------------------------------------------------------------------------------------

class VerticalDesc(C.Structure):
    _fields_ = [("n_fits", C.c_int32), ("num_steps", C.c_int32), ("n_pixels", C.c_int64), ("height", _lib.c_int32_p), ("width", _lib.c_int32_p),
                ("focal_x", _lib.c_double_p), ("focal_y", _lib.c_double_p), ("offset", _lib.c_int64_p), ("up_x", C.c_void_p), ("up_y", C.c_void_p),
                ("up_conf", C.c_void_p), ("lat", C.c_void_p), ("lat_conf", C.c_void_p), ("is_f32", C.c_int32)]


VERTICAL_SIGNATURES = {
    "cba_vertical_fit": (C.c_int, [C.POINTER(VerticalDesc), C.c_int32, _lib.c_double_p, _lib.c_int32_p, _lib.c_int32_p]),
}


def check_vertical_arguments(planes, height, width, focal_x, focal_y, offset, num_steps):
    """The arrays of a ``vertical_fit`` call in the layout of ``cba_vertical_desc``: five planes of one length and one dtype
    (float32 or float64; anything else is widened to float64), and the per-fit arrays.  ``ValueError`` for mismatched lengths, a
    side below 2, a non-positive or non-finite focal length, a pixel range outside the planes or a negative ``num_steps``."""
    if len(planes) != 5:
        raise ValueError("vertical_fit: five planes expected (up x, up y, up confidence, latitude, latitude confidence)")
    planes = [np.asarray(p) for p in planes]
    dtype = np.float32 if all(p.dtype == np.float32 for p in planes) else np.float64
    planes = [np.ascontiguousarray(p, dtype=dtype).reshape(-1) for p in planes]
    if len({len(p) for p in planes}) != 1:
        raise ValueError("vertical_fit: the five planes differ in length")
    height = np.ascontiguousarray(height, dtype=np.int32).reshape(-1)
    width = np.ascontiguousarray(width, dtype=np.int32).reshape(-1)
    focal_x = np.ascontiguousarray(focal_x, dtype=np.float64).reshape(-1)
    focal_y = np.ascontiguousarray(focal_y, dtype=np.float64).reshape(-1)
    offset = np.ascontiguousarray(offset, dtype=np.int64).reshape(-1)
    n = len(height)
    if not (len(width) == len(focal_x) == len(focal_y) == len(offset) == n):
        raise ValueError("vertical_fit: the per-fit arrays differ in length")
    num_steps = int(num_steps)
    if num_steps < 0:
        raise ValueError(f"vertical_fit: num_steps must not be negative, got {num_steps}")
    if n:
        if height.min() < 2 or width.min() < 2:
            raise ValueError("vertical_fit: every field needs a height and a width of at least 2")
        if not (np.isfinite(focal_x).all() and np.isfinite(focal_y).all() and focal_x.min() > 0 and focal_y.min() > 0):
            raise ValueError("vertical_fit: focal lengths must be positive and finite")
        if offset.min() < 0 or (offset + height.astype(np.int64) * width).max() > len(planes[0]):
            raise ValueError("vertical_fit: a fit's pixel range lies outside the planes")
    return planes, height, width, focal_x, focal_y, offset, num_steps


class DeviceVerticalFit:
    """The device call ``cba_vertical_fit`` on ``device_id``."""

    def __init__(self, device_id: int = 0):
        self.device_id = device_id

    def vertical_fit(self, planes, height, width, focal_x, focal_y, offset, num_steps=DEFAULT_NUM_STEPS):
        """``(fits[n, 8] float64, stop_step[n] int32, status[n] int32)`` for n fits over five packed planes; fit f reads pixels
        ``offset[f] : offset[f] + height[f] * width[f]`` of every plane.  A row of ``fits`` holds the first seven fields of
        :class:`GravityFit` and ``stop_step``."""
        planes, height, width, focal_x, focal_y, offset, num_steps = check_vertical_arguments(planes, height, width, focal_x, focal_y, offset, num_steps)
        n = len(height)
        fits, stop, status = np.zeros((n, 8), dtype=np.float64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        if n == 0:
            return fits, stop, status
        lib = _lib.bind(_lib.load(), VERTICAL_SIGNATURES)
        desc = VerticalDesc(n_fits=n, num_steps=num_steps, n_pixels=len(planes[0]), height=_lib.ptr(height), width=_lib.ptr(width),
                            focal_x=_lib.ptr(focal_x), focal_y=_lib.ptr(focal_y), offset=_lib.ptr(offset),
                            up_x=planes[0].ctypes.data, up_y=planes[1].ctypes.data, up_conf=planes[2].ctypes.data, lat=planes[3].ctypes.data,
                            lat_conf=planes[4].ctypes.data, is_f32=int(planes[0].dtype == np.float32))
        _lib.check(lib, lib.cba_vertical_fit(C.byref(desc), self.device_id, _lib.ptr(fits), _lib.ptr(stop), _lib.ptr(status)), "cba_vertical_fit")
        return fits, stop, status


# ---- the public fits -------------------------------------------------------------------------------------------------------------

def _field_set(index, up_field, up_confidence, latitude_field, latitude_confidence, focal_x_px, focal_y_px):
    """One field set in the reference's shapes -> (up (2, h, w), up confidence (h, w), latitude (h, w), its confidence (h, w), fx, fy)."""
    up = np.asarray(up_field)
    uc, lat, lc = np.asarray(up_confidence), np.asarray(latitude_field), np.asarray(latitude_confidence)
    if uc.ndim < 2:
        raise ValueError(f"field set {index}: up_confidence must be (h, w) or (1, h, w), got {uc.shape}")
    h, w = uc.shape[-2:]
    if h < 2 or w < 2:
        raise ValueError(f"field set {index}: fields of {h} x {w}; height and width must be at least 2")
    for name, arr, size in (("up_field", up, 2 * h * w), ("up_confidence", uc, h * w), ("latitude_field", lat, h * w), ("latitude_confidence", lc, h * w)):
        lead = (2, h, w) if name == "up_field" else (h, w)
        if arr.size != size or arr.shape[-len(lead):] != lead:
            raise ValueError(f"field set {index}: {name} has shape {arr.shape}, expected {lead} (leading axes of length 1 allowed)")
    fx, fy = float(focal_x_px), float(focal_y_px)
    if not (np.isfinite(fx) and np.isfinite(fy) and fx > 0 and fy > 0):
        raise ValueError(f"field set {index}: focal lengths must be positive and finite, got {fx}, {fy}")
    return up.reshape(2, h, w), uc.reshape(h, w), lat.reshape(h, w), lc.reshape(h, w), fx, fy


def fit_gravity_batch(field_sets, num_steps: int = DEFAULT_NUM_STEPS, *, device_id: int = 0, _solver=None) -> list[GravityFit]:
    """One :class:`GravityFit` per entry of ``field_sets``, all in one device call.  An entry is ``(up_field, up_confidence,
    latitude_field, latitude_confidence, focal_x_px, focal_y_px)`` in the shapes :func:`fit_gravity` accepts; entries may differ in
    shape.  float32 fields are sent as float32 and widened exactly on the device; any other dtype goes as float64.  An empty input
    returns an empty list without a launch."""
    if int(num_steps) < 0:
        raise ValueError(f"num_steps must not be negative, got {num_steps}")
    sets = [_field_set(i, *entry) for i, entry in enumerate(field_sets)]
    if not sets:
        return []
    all_f32 = all(a.dtype == np.float32 for s in sets for a in s[:4])
    dtype = np.float32 if all_f32 else np.float64
    sizes = np.array([s[1].size for s in sets], dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    planes = [np.concatenate([np.asarray(pick(s), dtype=dtype).reshape(-1) for s in sets])
              for pick in (lambda s: s[0][0], lambda s: s[0][1], lambda s: s[1], lambda s: s[2], lambda s: s[3])]
    backend = _solver or DeviceVerticalFit(device_id)
    fits, stop, status = backend.vertical_fit(planes, [s[1].shape[0] for s in sets], [s[1].shape[1] for s in sets], [s[4] for s in sets],
                                              [s[5] for s in sets], offset, int(num_steps))
    fits, stop, status = np.asarray(fits, dtype=np.float64), np.asarray(stop), np.asarray(status)
    if fits.shape != (len(sets), 8) or stop.shape != (len(sets),) or status.shape != (len(sets),):
        raise BackendError(f"vertical_fit returned shapes {fits.shape}, {stop.shape}, {status.shape} for {len(sets)} fits")
    for i, code in enumerate(status.tolist()):
        if code == STATUS_NONFINITE:
            raise ValueError(f"field set {i}: the cost at the start vector is not finite (NaN or infinity in a field or a confidence)")
        if code == STATUS_SINGULAR:
            raise np.linalg.LinAlgError(f"field set {i}: Singular matrix (the Hessian at the solution cannot be inverted)")
        if code != STATUS_OK:
            raise BackendError(f"field set {i}: unknown fit status {code}")
    return [GravityFit(*(float(v) for v in row[:7]), stop_step=int(s)) for row, s in zip(fits, stop.tolist())]


def fit_gravity(up_field, up_confidence, latitude_field, latitude_confidence, focal_x_px: float, focal_y_px: float,
                num_steps: int = DEFAULT_NUM_STEPS, *, device_id: int = 0, _solver=None) -> GravityFit:
    """Fit roll and pitch to the field network's outputs, focal fixed: ``up_field`` (2, h, w) or (1, 2, h, w), ``up_confidence``
    (h, w) or (1, h, w), ``latitude_field`` (1, h, w) or (1, 1, h, w) in radians, ``latitude_confidence`` (h, w) or (1, h, w);
    the focal lengths in pixels of the fields (the camera's focal times the preprocessor's resize scale)."""
    return fit_gravity_batch([(up_field, up_confidence, latitude_field, latitude_confidence, focal_x_px, focal_y_px)], num_steps,
                             device_id=device_id, _solver=_solver)[0]


def _angle_deg(vec_a, vec_b) -> float:
    cosine = float(np.clip(np.dot(vec_a, vec_b), -1.0, 1.0))
    return float(np.degrees(np.arccos(cosine)))


def aggregate_up_vectors(ups) -> tuple[np.ndarray, float]:
    """(consensus, spread) of the per-frame up vectors of one camera: the normalised mean, and the median angle (degrees) of the
    frames from it."""
    stacked = np.array(ups)
    consensus = stacked.mean(axis=0)
    consensus = consensus / np.linalg.norm(consensus)
    return consensus, float(np.median([_angle_deg(up, consensus) for up in ups]))


def estimate_vertical_from_fields(fields_per_cam, cameras, *, num_steps: int = DEFAULT_NUM_STEPS, device_id: int = 0, _solver=None) -> VerticalEstimate:
    """Per-camera up vectors from the field network's outputs.  ``fields_per_cam`` maps cam_id to the camera's sampled frames, each
    a mapping with ``up_field``, ``up_confidence``, ``latitude_field``, ``latitude_confidence`` and the preprocessor's ``scale_x``,
    ``scale_y`` (field resolution / original, per axis).  ``cameras`` is a ``CameraArray`` (or a mapping cam_id -> camera); the
    focal prior of a frame is ``matrix[0, 0] * scale_x`` and ``matrix[1, 1] * scale_y``.  All frames of all cameras are fitted in one
    device call.  ``up_per_cam`` of the result goes straight into ``CaptureVolume.oriented``."""
    lookup = getattr(cameras, "cameras", cameras)
    sets, owner = [], []
    for cam_id, frames in fields_per_cam.items():
        camera = lookup[cam_id]
        if camera.matrix is None:
            raise ValueError(f"Camera {cam_id} lacks an intrinsic matrix; vertical estimation needs a focal prior. Calibrate intrinsics first.")
        frames = list(frames)
        if not frames:
            raise ValueError(f"No frames given for cam {cam_id}")
        fx, fy = float(camera.matrix[0, 0]), float(camera.matrix[1, 1])
        for frame in frames:
            sets.append((*(frame[name] for name in FIELD_NAMES), fx * float(frame["scale_x"]), fy * float(frame["scale_y"])))
            owner.append(cam_id)
    fits = fit_gravity_batch(sets, num_steps, device_id=device_id, _solver=_solver)
    up_per_cam, spread_per_cam = {}, {}
    for cam_id in fields_per_cam:
        ups = [gravity_vec_from_roll_pitch(f.roll_rad, f.pitch_rad) for f, o in zip(fits, owner) if o == cam_id]
        up_per_cam[cam_id], spread_per_cam[cam_id] = aggregate_up_vectors(ups)
    return VerticalEstimate(up_per_cam=up_per_cam, spread_per_cam=spread_per_cam)


__all__ = ["GravityFit", "VerticalEstimate", "DeviceVerticalFit", "fit_gravity", "fit_gravity_batch", "estimate_vertical_from_fields",
           "gravity_vec_from_roll_pitch", "roll_pitch_from_gravity_vec", "sample_frame_indices", "aggregate_up_vectors", "DEFAULT_NUM_STEPS"]
