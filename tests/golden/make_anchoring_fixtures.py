"""Outputs of the REFERENCE's own scale report and anchoring operations on random tables, stored as fixtures.

    python tests/golden/make_anchoring_fixtures.py          (build container only: imports /root/reference/src)

What is run is the reference's code, unmodified: ``CaptureVolume.compute_volumetric_scale_accuracy``, ``align_to_object``, ``rotate``,
``translate``, ``scaled`` (all three cue types), ``oriented``, ``grounded``, ``centered`` (core/capture_volume.py:755-1329),
``estimate_similarity_transform`` and, through every one of the operations, ``apply_similarity_transform`` (core/alignment.py), and the
properties of ``VolumetricScaleReport`` (core/scale_accuracy.py).  None of them reaches ``cv2``; the reference imports it (and
``rtoml``) at module level, so the two stub modules of ``make_reference_host_fixtures.py`` satisfy the imports.  Nothing of the
reference is copied: a fixture holds the random INPUT tables and cameras this script made, the arguments of every call, and what the
reference returned, warned or raised.

Cases (``anchoring/anchor_NN.npz``): two to five rigid objects, some static (world points at STATIC_SYNC_INDEX, seen in every frame);
frames with holes, shuffled rows; sparse camera ids with one unposed camera; objects whose ``obj_loc_z`` is all NaN (planar boards),
objects with NaN z on some keypoints only, observations with NaN ``obj_loc_x``; a keypoint whose ``obj_loc`` differs between its rows
(the first row in table order is the one that counts); an object whose object points coincide (D_ref = 0; never the target of
``align_to_object``, whose rigid fit has no defined rotation there); world points dropped at
random (observations without a world point, groups of 2 and 3 joined rows); now and then a DUPLICATE world key; keypoint ids shared
between objects in odd cases (ambiguous depth cues) and distinct in even ones.  Three frames are made for ``align_to_object``: one
that shows a single object, one whose object has observations but no world point, one whose object has two world points.

Per case the calls are listed in ``ops`` (JSON): name, arguments, and either ``error`` (the exception's type and message) or the key
of the stored result (camera rotations and translations, NaN for the unposed camera; world coordinates) with the ``warnings`` raised.
Consumer: tests/test_anchoring.py."""
import json
import sys
import warnings
from pathlib import Path

import numpy as np
import pandas as pd

HERE = Path(__file__).parent
OUT = HERE / "anchoring"
N_CASES = 8
STATIC = -1
WORLD_COLS = ["sync_index", "object_id", "keypoint_id", "x_coord", "y_coord", "z_coord"]
IMG_COLS = ["sync_index", "cam_id", "object_id", "keypoint_id", "img_loc_x", "img_loc_y", "obj_loc_x", "obj_loc_y", "obj_loc_z"]
SINGLE, NO_WORLD, TWO_ROWS = 70, 71, 72  # the frames made for align_to_object


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def random_case(seed):
    rng = np.random.default_rng(4000 + seed)
    n_obj = int(rng.integers(2, 6))
    static = sorted(o for o in range(n_obj) if rng.random() < 0.35)
    if seed % 2 == 0 and not static:
        static = [n_obj - 1]
    if len(static) == n_obj:
        static = static[1:]
    frames = sorted(rng.choice(40, size=int(rng.integers(4, 12)), replace=False).tolist())
    cam_ids = sorted(rng.choice(12, size=4, replace=False).tolist())
    unposed = cam_ids[int(rng.integers(1, 4))]  # never the lowest id: the anchor of the tests is a posed camera either way
    distinct_kp = seed % 2 == 0
    cams = {}
    for c in cam_ids:
        R = random_rotation(rng)
        centre = rng.normal(size=3) * 2.0 + np.array([0.0, 0.0, -6.0])
        cams[c] = (None, None) if c == unposed else (R, -R @ centre)
    world, img, shapeless = [], [], []
    for o in range(n_obj):
        nk = int(rng.choice([3, 4, 4, 6, 12, 35]))
        kind = ("planar", "solid", "mixed", "planar", "coincident")[(o + seed) % 5]
        if kind == "coincident" and o == 0:
            kind = "solid"  # (object 0 is the one the single-object frame shows: align_to_object needs a shape to fit)
        if kind == "coincident":
            shapeless.append(o)
        pts = rng.uniform(-0.3, 0.3, size=(nk, 3))
        if kind == "coincident":
            pts[:] = pts[0]
        loc = pts.copy()
        if kind == "planar":
            pts[:, 2] = 0.0
            loc[:, 2] = np.nan
        elif kind == "mixed":
            gone = rng.random(nk) < 0.3
            gone[0] = True
            loc[gone, 2] = np.nan
        kp_id = (lambda k: 20 * o + k) if distinct_kp else (lambda k: k)
        special = (SINGLE,) if o == 0 else (NO_WORLD, TWO_ROWS) if o == 1 else ()
        for si in list(frames) + list(special):
            R, t = random_rotation(rng), rng.normal(size=3) * 0.5
            placed = 1.002 * (pts @ R.T) + t + rng.normal(size=pts.shape) * 0.002
            for k in range(nk):
                seen = False
                for c in cam_ids:
                    if rng.random() < 0.8 or si in special:
                        x = loc[k] + (0.01 if rng.random() < 0.03 else 0.0)  # now and then another obj_loc for the same keypoint
                        if rng.random() < 0.05 and si not in special:
                            x = np.array([np.nan, x[1], x[2]])
                        img.append((si, c, o, kp_id(k), float(rng.uniform(0, 400)), float(rng.uniform(0, 400)), *x.tolist()))
                        seen = True
                if o in static or si == NO_WORLD or (si == TWO_ROWS and k >= 2):
                    continue
                if seen and (rng.random() < 0.8 or si == SINGLE):
                    for _ in range(2 if rng.random() < 0.03 else 1):
                        world.append((si, o, kp_id(k), *placed[k].tolist()))
        if o in static:
            R, t = random_rotation(rng), rng.normal(size=3) * 0.5
            placed = 1.002 * (pts @ R.T) + t + rng.normal(size=pts.shape) * 0.002
            for k in range(nk):
                if rng.random() < 0.9:
                    world.append((STATIC, o, kp_id(k), *placed[k].tolist()))
    world = [world[i] for i in rng.permutation(len(world))]
    img = [img[i] for i in rng.permutation(len(img))]
    return rng, world, img, static, cam_ids, cams, frames, shapeless


def main():
    sys.path.insert(0, str(HERE))
    from make_reference_host_fixtures import _stub_modules

    _stub_modules()
    sys.path.insert(0, "/root/reference/src")
    from caliscope.cameras.camera_array import CameraArray, CameraData
    from caliscope.core.alignment import estimate_similarity_transform
    from caliscope.core.capture_volume import CaptureVolume
    from caliscope.core.constraints import ConstraintSet
    from caliscope.core.point_data import STATIC_SYNC_INDEX, ImagePoints, WorldPoints
    from caliscope.core.scale_cues import CameraDistance, DepthObservation, SegmentLength

    assert STATIC_SYNC_INDEX == STATIC
    OUT.mkdir(exist_ok=True)
    K = np.array([[400.0, 0.0, 200.0], [0.0, 400.0, 200.0], [0.0, 0.0, 1.0]])
    cue_types = {"CameraDistance": CameraDistance, "SegmentLength": SegmentLength, "DepthObservation": DepthObservation}
    for case in range(N_CASES):
        rng, world, img, static, cam_ids, cams, frames, shapeless = random_case(case)
        wdf = pd.DataFrame(world, columns=WORLD_COLS).astype({c: "int64" for c in WORLD_COLS[:3]})
        wdf["frame_time"] = np.where(wdf["sync_index"] == STATIC, np.nan, wdf["sync_index"] * 0.1)
        idf = pd.DataFrame(img, columns=IMG_COLS).astype({c: "int64" for c in IMG_COLS[:4]})
        array = CameraArray({c: CameraData(cam_id=c, size=(400, 400), matrix=K.copy(), distortions=np.zeros(5), rotation=R, translation=t, error=0.1 * c,
                                           grid_count=c) for c, (R, t) in cams.items()})
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vol = CaptureVolume(array, ImagePoints(idf), WorldPoints(wdf), ConstraintSet((), frozenset(static)))
        wtab, itab = vol.world_points.df, vol.image_points.df
        out = dict(world=wtab[WORLD_COLS].to_numpy(dtype=np.float64), image=itab[IMG_COLS].to_numpy(dtype=np.float64),
                   static=np.array(static, dtype=np.int64), cam_ids=np.array(cam_ids, dtype=np.int64),
                   cam_R=np.array([np.full((3, 3), np.nan) if cams[c][0] is None else cams[c][0] for c in cam_ids]),
                   cam_t=np.array([np.full(3, np.nan) if cams[c][1] is None else cams[c][1] for c in cam_ids]))

        # -- the scale report -------------------------------------------------------------------------------------------
        rep = vol.compute_volumetric_scale_accuracy()
        out["frame_errors"] = np.array([[fe.sync_index, fe.object_id, fe.distance_rmse_mm, fe.distance_mean_signed_error_mm, fe.distance_max_error_mm,
                                         fe.n_corners, fe.n_distance_pairs, fe.n_cameras_contributing, fe.sum_squared_errors_m2,
                                         fe.sum_squared_relative_errors, *fe.centroid] for fe in rep.frame_errors], dtype=np.float64).reshape(-1, 13)
        nan_if_none = lambda v: float("nan") if v is None else float(v)  # noqa: E731
        out["report_scalars"] = np.array([rep.pooled_rmse_mm, rep.median_rmse_mm, rep.max_rmse_mm, rep.n_frames_sampled, rep.mean_signed_error_mm,
                                          rep.min_sync_index, rep.max_sync_index, rep.pooled_relative_rmse_pct, *map(nan_if_none, rep.split_relative_rmse_pct),
                                          rep.worst_frame.sync_index if rep.worst_frame else -99, rep.worst_frame.object_id if rep.worst_frame else -99],
                                         dtype=np.float64)
        for name in ("per_frame_relative_rmse_pct", "per_frame_rmse_mm", "per_object_relative_rmse_pct"):
            d = getattr(rep, name)
            out[name] = np.array([[k, v] for k, v in d.items()], dtype=np.float64).reshape(-1, 2)
        out["report_static"] = np.array(sorted(rep.static_object_ids), dtype=np.int64)

        # -- operations ---------------------------------------------------------------------------------------------------
        ops = []

        def run(name, call, **args):
            op = {"op": name, "args": args, "error": None, "warnings": [], "key": None}
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                try:
                    new = call()
                except (ValueError, TypeError, RuntimeError) as e:
                    op["error"] = [type(e).__name__, str(e)]
                    new = None
            op["warnings"] = [str(w.message) for w in caught]
            if new is not None:
                key = f"op{len(ops):02d}"
                op["key"] = key
                out[key + "_xyz"] = new.world_points.points
                out[key + "_R"] = np.array([np.full((3, 3), np.nan) if new.camera_array.cameras[c].rotation is None else new.camera_array.cameras[c].rotation
                                            for c in cam_ids])
                out[key + "_t"] = np.array([np.full(3, np.nan) if new.camera_array.cameras[c].translation is None else new.camera_array.cameras[c].translation
                                            for c in cam_ids])
                cam = new.camera_array.cameras[cam_ids[0]]
                assert cam.error == 0.1 * cam_ids[0] and cam.grid_count == cam_ids[0] and np.array_equal(cam.matrix, K)
                assert new.image_points is vol.image_points and new.constraints is vol.constraints
            ops.append(op)
            return new

        # (a rigid fit to coinciding object points has no defined rotation: such objects are left to the scale report, where they give D_ref = 0)
        moving = [o for o in sorted(set(wtab["object_id"])) if o not in static and o not in shapeless]
        mid = frames[len(frames) // 2]
        for si in (frames[0], mid, frames[-1]):
            for o in moving[:2]:
                run("align_to_object", lambda: vol.align_to_object(si, o), sync_index=si, object_id=int(o))
        run("align_to_object", lambda: vol.align_to_object(SINGLE), sync_index=SINGLE, object_id=None)
        run("align_to_object", lambda: vol.align_to_object(mid), sync_index=mid, object_id=None)          # several markers (or one: whatever the frame holds)
        run("align_to_object", lambda: vol.align_to_object(999), sync_index=999, object_id=None)
        run("align_to_object", lambda: vol.align_to_object(mid, 99), sync_index=mid, object_id=99)
        run("align_to_object", lambda: vol.align_to_object(NO_WORLD, 1), sync_index=NO_WORLD, object_id=1)
        run("align_to_object", lambda: vol.align_to_object(TWO_ROWS, 1), sync_index=TWO_ROWS, object_id=1)
        run("align_to_object", lambda: vol.align_to_object(None), sync_index=None, object_id=None)
        run("align_to_object", lambda: vol.align_to_object(None, int(moving[0])), sync_index=None, object_id=int(moving[0]))
        for o in [o for o in static if o not in shapeless]:
            run("align_to_object", lambda: vol.align_to_object(None, o), sync_index=None, object_id=int(o))
            run("align_to_object", lambda: vol.align_to_object(mid, o), sync_index=mid, object_id=int(o))

        for axis, angle in (("x", 90.0), ("y", -37.5), ("z", 191.0), ("w", 10.0)):
            run("rotate", lambda: vol.rotate(axis, angle), axis=axis, angle_degrees=angle)
        shift = rng.normal(size=3).tolist()
        run("translate", lambda: vol.translate(*shift), x=shift[0], y=shift[1], z=shift[2])
        run("translate", lambda: vol.translate(z=0.25), z=0.25)

        posed = [c for c in cam_ids if cams[c][0] is not None]
        unposed = [c for c in cam_ids if cams[c][0] is None][0]

        def scaled(cue_rows):
            return run("scaled", lambda: vol.scaled(*[cue_types[r[0]](*r[1:]) for r in cue_rows]), cues=cue_rows)

        s = float(rng.uniform(0.5, 3.0))
        d01 = float(np.linalg.norm(vol._camera_center(posed[0]) - vol._camera_center(posed[1])))
        d02 = float(np.linalg.norm(vol._camera_center(posed[0]) - vol._camera_center(posed[2])))
        scaled([["CameraDistance", posed[0], posed[1], s * d01]])
        scaled([["CameraDistance", posed[0], posed[1], s * d01, 0.02]])
        # a segment between two keypoints of one object that share frames
        kps = wtab[wtab["object_id"] == moving[0]]["keypoint_id"].value_counts().index.tolist()[:2]
        seg = None
        try:
            seg = vol._compile_cue(SegmentLength(int(kps[0]), int(kps[1]), 1.0))[0]
        except ValueError:
            pass
        agreeing = [["CameraDistance", posed[0], posed[1], s * d01 * 1.001], ["CameraDistance", posed[0], posed[2], s * d02 * 0.999, 0.015]]
        if seg:
            agreeing.append(["SegmentLength", int(kps[0]), int(kps[1]), s * seg * 1.002])
            scaled([["SegmentLength", int(kps[0]), int(kps[1]), s * seg]])
        # depth cues by outcome, found with the reference's own compiler
        by_outcome = {}
        for _ in range(4000):
            row = wtab.iloc[int(rng.integers(len(wtab)))]
            cue = DepthObservation(int(rng.choice(cam_ids)), int(row["keypoint_id"]), int(row["sync_index"]) + (1000 if rng.random() < 0.05 else 0), 1.0)
            res = vol._compile_depth_cue(cue)
            by_outcome.setdefault(res if isinstance(res, str) else "ok", []).append((cue, res))
        good = [["DepthObservation", c.cam_id, c.keypoint_id, c.sync_index, s * r[0] * float(rng.uniform(0.99, 1.01)), 0.1] for c, r in by_outcome.get("ok", [])[:40]]
        bad = [["DepthObservation", c.cam_id, c.keypoint_id, c.sync_index, 1.5] for reason, lst in sorted(by_outcome.items()) if reason != "ok"
               for c, _ in lst[:3]]
        out["depth_outcomes"] = np.array(sorted(by_outcome), dtype="U32")
        scaled(agreeing + good[:5])
        scaled(agreeing[:1] + [["CameraDistance", posed[0], posed[2], 1.5 * s * d02, 0.001]] + agreeing[2:])  # disagreement
        mixed = good + bad
        mixed = [mixed[i] for i in rng.permutation(len(mixed))]
        scaled(mixed)
        scaled(agreeing[:1] + mixed)
        scaled(bad)                                                                                            # all unresolvable
        scaled([])
        scaled([["CameraDistance", posed[0], unposed, 1.0]])
        scaled([["CameraDistance", posed[0], 77, 1.0]])
        scaled([["CameraDistance", posed[0], posed[0], 1.0]])
        scaled([["SegmentLength", 9999, int(kps[0]), 1.0]])

        def oriented(up):
            return run("oriented", lambda: vol.oriented({int(c): np.array(v) for c, v in up}), up=[[int(c), list(map(float, v))] for c, v in up])

        g = random_rotation(rng)[0]
        oriented([(c, cams[c][0] @ (g + rng.normal(size=3) * 0.03)) for c in posed])
        oriented([(posed[1], cams[posed[1]][0] @ g * 3.0)])
        oriented([(posed[0], cams[posed[0]][0] @ g), (posed[1], -(cams[posed[1]][0] @ g))])   # the verticals cancel
        oriented([(posed[0], [0.0, 0.0, 1.0])])                                               # vertical along the anchor's optical axis
        oriented([(unposed, [0.0, -1.0, 0.0])])
        oriented([(55, [0.0, -1.0, 0.0])])
        oriented([])
        run("grounded", lambda: vol.grounded(), mode="lowest_point", lowest_point_height_m=0.0)
        run("grounded", lambda: vol.grounded(lowest_point_height_m=0.04), mode="lowest_point", lowest_point_height_m=0.04)
        run("grounded", lambda: vol.grounded("plane"), mode="plane", lowest_point_height_m=0.0)
        run("centered", lambda: vol.centered())
        first = run("scaled", lambda: vol.scaled(CameraDistance(posed[0], posed[1], s * d01)), cues=[["CameraDistance", posed[0], posed[1], s * d01]])
        run("chain", lambda: first.oriented({posed[0]: cams[posed[0]][0] @ g}).grounded().centered(),
            cues=[["CameraDistance", posed[0], posed[1], s * d01]], up=[[int(posed[0]), (cams[posed[0]][0] @ g).tolist()]])
        out["ops"] = np.array(json.dumps(ops))

        # -- estimate_similarity_transform ----------------------------------------------------------------------------------
        est = []
        for k, (n, rigid, flat) in enumerate([(3, False, False), (10, True, False), (40, False, False), (6, False, True), (2, False, False), (5, True, True)]):
            src = rng.normal(size=(n, 3))
            if flat:
                src[:, 2] = 0.0
            R, t, sc = random_rotation(rng), rng.normal(size=3), float(rng.uniform(0.3, 3.0))
            dst = sc * src @ R.T + t + rng.normal(size=src.shape) * 0.01
            if k == 3:
                dst[:, 0] = -dst[:, 0]  # a mirrored target: the reflection fix
            out[f"est{k}_src"], out[f"est{k}_dst"] = src, dst
            try:
                tr = estimate_similarity_transform(src, dst, rigid=rigid)
                out[f"est{k}_R"], out[f"est{k}_t"], out[f"est{k}_s"] = tr.rotation, tr.translation, np.array(tr.scale)
                out[f"est{k}_inv"] = tr.inverse.matrix
                est.append({"rigid": rigid, "error": None})
            except (ValueError, RuntimeError) as e:
                est.append({"rigid": rigid, "error": [type(e).__name__, str(e)]})
        out["est"] = np.array(json.dumps(est))
        np.savez_compressed(OUT / f"anchor_{case:02d}.npz", **out)
        n_err = sum(op["error"] is not None for op in ops)
        print(f"anchor_{case:02d}: {len(wtab)} world rows, {len(itab)} image rows, {len(rep.frame_errors)} report entries, static {static}, "
              f"{len(ops)} ops ({n_err} errors, {sum(bool(op['warnings']) for op in ops)} with warnings), depth outcomes {sorted(by_outcome)}")


if __name__ == "__main__":
    main()
