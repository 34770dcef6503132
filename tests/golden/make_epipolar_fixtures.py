"""Choices of the REFERENCE's own epipolar builder on scripted 2-D-only sessions, stored as fixtures.

    python tests/golden/make_epipolar_fixtures.py REFERENCE_SRC      (build container only: imports the reference's src/)

What is run is the reference's ``build_epipolar_pose_network`` (core/bootstrap_pose/epipolar_pose_builder.py), unmodified: pooled
correspondences, scaffold candidates by cheirality, triangulation of each candidate, resection of every other camera, the
third-view score, the anchor-relative StereoPairs, then its stereo-RMSE stage and ``apply_to``.  The reference imports ``cv2``; it
is not installed here, so a stub module answers with the scripted results of tests/epipolar_script.py (the same ones its
``ScriptedEpipolar`` hook gives caliscope_amd.epipolar_pose): ``undistortPoints``, ``findEssentialMat``, ``recoverPose``,
``triangulatePoints``, ``solvePnPRansac``, ``projectPoints`` and ``Rodrigues``.  The stub recognises a pair and its keys from the
normalised points it is handed.  Nothing of the reference is copied: the fixtures hold the session this script made and what the
reference chose for it.  Pair (0, 1) gets the twisted-pair solution with the most cheirality inliers; camera 4 shares < 50 points
with every cloud.  Consumer: tests/test_epipolar_reference_fixtures.py.
"""
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).parent
OUT = HERE / "epipolar"
sys.path.insert(0, str(HERE.parent.parent))

from tests import epipolar_script as S  # noqa: E402

N_CASES = 3


def _stub_cv2(df, poses):
    from scipy.spatial.transform import Rotation

    und = S.undistort(df[["img_loc_x", "img_loc_y"]].to_numpy())
    who = {(float(x), float(y)): (int(c), int(s), int(k)) for (x, y), c, s, k in zip(und, df.cam_id, df.sync_index, df.keypoint_id)}
    state = {}

    def ident(points):
        info = [who[(float(x), float(y))] for x, y in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
        return info[0][0], np.array([[s, k] for _, s, k in info]).reshape(-1, 2)

    cv2 = types.ModuleType("cv2")
    for i, name in enumerate(("SOLVEPNP_ITERATIVE", "SOLVEPNP_EPNP", "SOLVEPNP_P3P", "SOLVEPNP_DLS", "SOLVEPNP_UPNP", "SOLVEPNP_AP3P",
                              "SOLVEPNP_IPPE", "SOLVEPNP_IPPE_SQUARE", "SOLVEPNP_SQPNP", "RANSAC")):
        setattr(cv2, name, i)

    def rodrigues(a):
        a = np.asarray(a, dtype=np.float64)
        if a.shape == (3, 3):
            return Rotation.from_matrix(a).as_rotvec().reshape(3, 1), None
        return Rotation.from_rotvec(a.reshape(3)).as_matrix(), None

    def undistort_points(points, matrix, dist, P=None):
        return S.undistort(points).reshape(-1, 1, 2)

    def find_essential(a, b, cameraMatrix=None, method=None, prob=None, threshold=None):
        ca, keys = ident(a)
        cb, _ = ident(b)
        R, t = S.relative_pose(poses, ca, cb)
        state["pair"] = (ca, cb)
        E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        return E, S.ransac_inlier(keys[:, 0], keys[:, 1]).astype(np.uint8).reshape(-1, 1)

    def recover_pose(E, a, b, cameraMatrix=None):
        ca, keys = ident(a)
        cb, _ = ident(b)
        R, t = S.relative_pose(poses, ca, cb)
        mask = S.cheiral((ca, cb), keys[:, 0], keys[:, 1])
        return int(mask.sum()), R, t.reshape(3, 1), (mask.astype(np.uint8) * 255).reshape(-1, 1)

    def triangulate_points(P1, P2, a, b):
        return S.triangulate(P2[:, :3], P2[:, 3], np.asarray(a).T, np.asarray(b).T)

    def solve_pnp_ransac(obj, uv, K, dist, reprojectionError=None, iterationsCount=None, flags=None):
        R, t = S.pnp(np.asarray(obj).reshape(-1, 3), np.asarray(uv).reshape(-1, 2))
        return True, Rotation.from_matrix(R).as_rotvec().reshape(3, 1), t.reshape(3, 1), np.arange(len(obj)).reshape(-1, 1)

    def project_points(obj, rvec, tvec, K, dist):
        R = Rotation.from_rotvec(np.asarray(rvec, dtype=np.float64).reshape(3)).as_matrix()
        return S.project(np.asarray(obj).reshape(-1, 3), R, np.asarray(tvec, dtype=np.float64).reshape(3)).reshape(-1, 1, 2), None

    cv2.Rodrigues, cv2.undistortPoints, cv2.findEssentialMat, cv2.recoverPose = rodrigues, undistort_points, find_essential, recover_pose
    cv2.triangulatePoints, cv2.solvePnPRansac, cv2.projectPoints = triangulate_points, solve_pnp_ransac, project_points
    sys.modules["cv2"] = cv2
    sys.modules.setdefault("rtoml", types.ModuleType("rtoml"))


def main(reference_src):
    sys.path.insert(0, reference_src)
    OUT.mkdir(exist_ok=True)
    for case in range(N_CASES):
        df, poses, _ = S.session(case)
        _stub_cv2(df, poses)
        for m in [m for m in sys.modules if m.startswith("caliscope.")]:
            del sys.modules[m]  # (re-import against this case's stub)
        from caliscope.cameras.camera_array import CameraArray, CameraData
        from caliscope.core.bootstrap_pose import epipolar_pose_builder as epb
        from caliscope.core.point_data import ImagePoints

        def cams():
            return CameraArray(cameras={c: CameraData(cam_id=c, size=(1280, 720), matrix=S.K.copy(), distortions=np.zeros(5))
                                        for c in range(S.N_CAMS)})

        scores, captured = [], {}
        assemble, finish = epb._assemble_from_scaffold, epb.estimate_pnp_paired_pose_network

        def assemble_rec(pair, *a, **k):
            poses_out, score = assemble(pair, *a, **k)
            scores.append((pair[0], pair[1], score[0], score[1], score[2], len(poses_out)))
            return poses_out, score

        def finish_rec(aggregated, *a, **k):
            captured.update(aggregated)
            return finish(aggregated, *a, **k)

        epb._assemble_from_scaffold, epb.estimate_pnp_paired_pose_network = assemble_rec, finish_rec
        arr = cams()
        net = epb.build_epipolar_pose_network(ImagePoints(df), arr)
        net.apply_to(arr)
        agg = sorted(captured)
        best = min(range(len(scores)), key=lambda i: (scores[i][2:5], i))
        np.savez_compressed(
            OUT / f"epi_{case:02d}.npz",
            df_int=df[["sync_index", "cam_id", "object_id", "keypoint_id"]].to_numpy(np.int64), df_xy=df[["img_loc_x", "img_loc_y"]].to_numpy(),
            true_R=np.array([poses[c][0] for c in range(S.N_CAMS)]), true_t=np.array([poses[c][1] for c in range(S.N_CAMS)]),
            scores=np.array(scores, dtype=np.float64), scaffold=np.array(scores[best][:2], dtype=np.int64),
            agg_keys=np.array(agg, dtype=np.int64).reshape(-1, 2), agg_R=np.array([captured[p].rotation for p in agg]).reshape(-1, 3, 3),
            agg_t=np.array([np.ravel(captured[p].translation) for p in agg]).reshape(-1, 3),
            posed=np.array([arr.cameras[c].rotation is not None for c in range(S.N_CAMS)]),
            out_R=np.array([arr.cameras[c].rotation if arr.cameras[c].rotation is not None else np.full((3, 3), np.nan) for c in range(S.N_CAMS)]),
            out_t=np.array([np.ravel(arr.cameras[c].translation) if arr.cameras[c].translation is not None else np.full(3, np.nan)
                            for c in range(S.N_CAMS)]),
        )
        print(f"epi_{case:02d}: scores {[(int(a), int(b), int(f), round(w, 6), int(c)) for a, b, f, w, c, _ in scores]}, scaffold {scores[best][:2]}, "
              f"pairs {agg}")


if __name__ == "__main__":
    main(sys.argv[1])
