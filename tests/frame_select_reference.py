"""A plain NumPy selector that stands in for fsel_select of caliscope_amd/csrc/frame_select_math.h.  TEST INFRASTRUCTURE.

Written from the header's comments, not from its code: per tilt bin the eligible frame of largest tilt magnitude (lowest frame on
ties), then greedy rounds by ``popcount(fresh) + 0.2 edge + 0.3 corner + 0.3 distance`` with the 0.01 stop.  Every round recomputes
every frame's distance to ALL selected frames from scratch (no running minimum), everything is float64, nothing is parallel: a
mistake of the workgroup argmax, of a stride loop or of the running distance cannot be shared with it.

It takes the per-frame outputs of the backend under test (cell masks, pose features, orientation features) and the corner counts,
so that it checks the discrete selection alone; the per-frame arithmetic has its own checks.  It also returns the smallest margin
of every discrete decision it made, as tests/golden/make_frame_selection_fixtures.py does: the top two of each bin, the top two of
each round that selected, |best score - 0.01|, the distance of tilt_direction * 8 / 2 pi to an integer and |tilt_magnitude - 0.1|.
Rivals that are bit-identical twins of the winner are left out (such a tie is exact and goes to the lowest frame).  The scenes
have to keep every margin at or above frame_select_fixtures.MARGIN_FLOOR, so that no choice hangs on rounding.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

N_BINS = 8
MIN_TILT = 0.1
MIN_SCORE = 0.01
EDGE_WEIGHT, CORNER_WEIGHT, DIVERSITY_WEIGHT = 0.2, 0.3, 0.3


@dataclass
class ReferenceSelection:
    selected: np.ndarray   # [target], -1 beyond n_selected
    n_selected: int
    n_anchors: int
    bin_mask: int
    eligible: int
    min_margin: float      # inf when no decision was made


def popcount(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def grid_masks(grid):
    edge = sum(1 << (r * grid + c) for r in range(grid) for c in range(grid) if r in (0, grid - 1) or c in (0, grid - 1))
    corner = (1 << 0) | (1 << (grid - 1)) | (1 << ((grid - 1) * grid)) | (1 << ((grid - 1) * grid + grid - 1))
    return np.uint64(edge), np.uint64(corner)


def _best(values, frames, twin_of):
    """The frame of largest value, lowest frame on ties, and its margin to the best rival that is not its twin (inf: none)."""
    order = np.lexsort((frames, -values))
    win = int(frames[order[0]])
    rivals = [float(values[k]) for k in order[1:] if twin_of[int(frames[k])] != twin_of[win]]
    return win, float(values[order[0]]), (float(values[order[0]]) - rivals[0] if rivals else np.inf)


def select(cell_mask, pose_features, orientation, corners, *, grid, min_corners, target) -> ReferenceSelection:
    """One camera.  ``cell_mask`` [nf] uint64, ``pose_features`` [nf, 5], ``orientation`` [nf, 3], ``corners`` [nf]."""
    mask = np.ascontiguousarray(cell_mask, dtype=np.uint64)
    pose = np.asarray(pose_features, dtype=np.float64).reshape(-1, 5)
    orient = np.asarray(orientation, dtype=np.float64).reshape(-1, 3)
    corners = np.asarray(corners)
    nf = len(mask)
    eligible = corners >= min_corners
    # twins: frames whose features are equal bit for bit
    ids, twin_of = {}, []
    for f in range(nf):
        twin_of.append(ids.setdefault((int(mask[f]), pose[f].tobytes(), orient[f].tobytes(), bool(eligible[f])), len(ids)))
    margins = []
    frames = np.flatnonzero(eligible)
    # phase 1: one anchor per occupied tilt bin
    bins = np.full(nf, -1)
    for f in frames:
        direction, tilt = orient[f, 0], orient[f, 1]
        margins.append(abs(tilt - MIN_TILT))
        if tilt >= MIN_TILT:
            q = direction * N_BINS / (2 * np.pi)
            margins.append(abs(q - round(q)))
            bins[f] = min(int(q), N_BINS - 1)
    anchors, bin_mask = [], 0
    for b in range(N_BINS):
        members = frames[bins[frames] == b]
        if len(members):
            win, _, margin = _best(orient[members, 1], members, twin_of)
            margins.append(margin)
            anchors.append(win)
            bin_mask |= 1 << b
    selected = anchors[:target]
    # phase 2: greedy coverage and diversity
    if len(anchors) < target:
        edge, corner = grid_masks(grid)
        while len(selected) < target:
            rest = np.array([f for f in frames if f not in selected], dtype=np.int64)
            if len(rest) == 0:
                break
            covered = np.uint64(0)
            for s in selected:
                covered |= mask[s]
            fresh = mask[rest] & ~covered
            score = popcount(fresh) + EDGE_WEIGHT * popcount(fresh & edge) + CORNER_WEIGHT * popcount(fresh & corner)
            if selected:
                d = np.sqrt(((pose[rest][:, None, :] - pose[selected][None, :, :]) ** 2).sum(axis=2)).min(axis=1)
                score = score + DIVERSITY_WEIGHT * d
            win, best, margin = _best(score.astype(np.float64), rest, twin_of)
            margins.append(abs(best - MIN_SCORE))
            if best < MIN_SCORE:
                break
            margins.append(margin)
            selected.append(win)
    out = np.full(target, -1, dtype=np.int32)
    out[:len(selected)] = selected
    return ReferenceSelection(out, len(selected), len(anchors), bin_mask, int(eligible.sum()), float(min(margins)) if margins else np.inf)


def check_call(call, result, *, grid=5, min_corners, target, label=""):
    """The reference on every camera of a ``calibration_edge_scenes.SelCall`` against a backend's FrameSelection ``result``
    (fed that backend's own per-frame outputs): selected, n_selected, n_anchors, bin_mask and eligible equal.  Returns the smallest
    margin over the call."""
    worst = np.inf
    corners = call.corners
    for c, name in enumerate(call.labels):
        a, b = int(call.cam_frame_start[c]), int(call.cam_frame_start[c + 1])
        ref = select(result.cell_mask[a:b], result.pose_features[a:b], result.orientation[a:b], corners[a:b], grid=grid, min_corners=min_corners,
                     target=target)
        where = (label, name, target, min_corners)
        assert result.selected[c].tolist() == ref.selected.tolist(), (where, result.selected[c].tolist(), ref.selected.tolist())
        assert int(result.n_selected[c]) == ref.n_selected and int(result.n_anchors[c]) == ref.n_anchors, where
        assert int(result.bin_mask[c]) == ref.bin_mask, where
        assert int(result.eligible[c]) == ref.eligible == int((corners[a:b] >= min_corners).sum()), where
        worst = min(worst, ref.min_margin)
    return worst
