"""Outputs of the REFERENCE's own pose-network host stages on random camera-to-object poses, stored as fixtures.

    python tests/golden/make_pose_network_fixtures.py          (build container only: imports /root/reference/src)

What is run is the reference's code, unmodified (core/bootstrap_pose/): ``compute_relative_poses``, ``reject_outliers``, ``aggregate_poses``
(-> ``quaternion_average``), ``PairedPoseNetwork.from_raw_estimates`` with injected error scores, and ``apply_to`` (anchor choice, largest
connected component).  The reference imports ``cv2`` at module level; it is not installed here, so a stub module stands in: the ``SOLVEPNP_*``
constants the signatures name and ``Rodrigues`` through scipy's ``Rotation``.  None of the stages above calls OpenCV otherwise.  Nothing of the
reference is copied: the fixtures hold the random INPUT poses this script made and what the reference returned for them.

Cases: four to six cameras (one of them ignored in some cases), a board (object 0) and sometimes a second object over a few dozen frames;
rotation and translation outliers; NaN poses; a pair seen fewer than 5 times; a pair never seen together (bridged); a camera that never shares
a view (disconnected).  Consumer: tests/test_pose_network_host.py.
"""
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).parent
OUT = HERE / "pose_network"
N_CASES = 6


def _stub_cv2():
    from scipy.spatial.transform import Rotation

    cv2 = types.ModuleType("cv2")
    for i, name in enumerate(("SOLVEPNP_ITERATIVE", "SOLVEPNP_EPNP", "SOLVEPNP_P3P", "SOLVEPNP_DLS", "SOLVEPNP_UPNP", "SOLVEPNP_AP3P",
                              "SOLVEPNP_IPPE", "SOLVEPNP_IPPE_SQUARE", "SOLVEPNP_SQPNP")):
        setattr(cv2, name, i)

    def rodrigues(a):
        a = np.asarray(a, dtype=np.float64)
        if a.shape == (3, 3):
            return Rotation.from_matrix(a).as_rotvec().reshape(3, 1), None
        return Rotation.from_rotvec(a.reshape(3)).as_matrix(), None

    cv2.Rodrigues = rodrigues
    rtoml = types.ModuleType("rtoml")
    sys.modules.setdefault("cv2", cv2)
    sys.modules.setdefault("rtoml", rtoml)


def random_poses(seed):
    """Camera-to-object poses keyed (cam, sync, obj) of a rig seeing a moving board; cameras, ignore flags."""
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(500 + seed)
    n_cams = int(rng.integers(4, 7))
    cams = list(range(n_cams))
    rig_R = [Rotation.from_rotvec(rng.normal(0, 0.8, 3)).as_matrix() for _ in cams]
    rig_t = [rng.normal(0, 1.0, 3) for _ in cams]
    lone = cams[-1]  # never shares a view
    no_pair = (0, n_cams - 2)  # never seen together: bridged
    sparse = (1, 2)  # seen together fewer than 5 times
    poses = {}
    n_frames = int(rng.integers(20, 40))
    for f in range(n_frames):
        for o in ((0, 1) if seed % 2 else (0,)):
            Rb = Rotation.from_rotvec(rng.normal(0, 0.5, 3)).as_matrix()
            tb = rng.normal(0, 0.3, 3) + [0, 0, 2.0]
            seeing = [c for c in cams[:-1] if rng.random() < 0.8]
            if f % 2 == 0 and no_pair[1] in seeing:
                seeing = [c for c in seeing if c != no_pair[0]]
            elif no_pair[0] in seeing and no_pair[1] in seeing:
                seeing.remove(no_pair[1])
            if f > 2 and sparse[0] in seeing and sparse[1] in seeing:
                seeing.remove(sparse[1])
            for c in seeing:
                R = rig_R[c] @ Rb  # world -> camera composed with object -> world
                t = rig_R[c] @ tb + rig_t[c]
                R = Rotation.from_rotvec(Rotation.from_matrix(R).as_rotvec() + rng.normal(0, 0.003, 3)).as_matrix()
                t = t + rng.normal(0, 0.003, 3)
                u = rng.random()
                if u < 0.04:
                    R = Rotation.from_rotvec(rng.normal(0, 1.0, 3)).as_matrix() @ R  # rotation outlier
                elif u < 0.08:
                    t = t * rng.uniform(1.5, 3.0)  # translation outlier
                elif u < 0.10:
                    t = t * np.nan  # NaN pose
                poses[(c, f, o)] = (R, t, float(rng.uniform(0.001, 0.01)))
    poses[(lone, 10_000, 0)] = (np.eye(3), np.array([0.0, 0.0, 2.0]), 0.001)
    ignore = [c == 1 and seed % 3 == 2 for c in cams]
    return cams, ignore, poses


def main():
    _stub_cv2()
    sys.path.insert(0, "/root/reference/src")
    from caliscope.cameras.camera_array import CameraArray, CameraData
    from caliscope.core.bootstrap_pose.paired_pose_network import PairedPoseNetwork
    from caliscope.core.bootstrap_pose.pose_network_builder import aggregate_poses, compute_relative_poses, reject_outliers
    from caliscope.core.bootstrap_pose.stereopairs import StereoPair

    OUT.mkdir(exist_ok=True)
    for case in range(N_CASES):
        cams, ignore, poses = random_poses(case)
        arr = CameraArray(cameras={c: CameraData(cam_id=c, size=(640, 480), ignore=ig) for c, ig in zip(cams, ignore)})
        keys = sorted(poses)
        rel = compute_relative_poses(poses, arr)
        rel_keys = sorted(rel, key=lambda k: (k[0], k[1], k[2]))
        key_of = {id(sp): k for k, sp in rel.items()}
        filtered = reject_outliers(rel)
        kept = sorted((k[0][0], k[0][1], k[1], k[2]) for sps in filtered.values() for k in (key_of[id(sp)] for sp in sps))
        agg = aggregate_poses(filtered)
        agg_keys = sorted(agg)
        rng = np.random.default_rng(900 + case)
        errors = {p: float(rng.uniform(0.001, 0.02)) for p in agg_keys}
        raw = {p: StereoPair(p[0], p[1], errors[p], agg[p].translation, agg[p].rotation) for p in agg_keys}
        net = PairedPoseNetwork.from_raw_estimates(raw)
        net_keys = sorted(net._pairs)
        applied = CameraArray(cameras={c: CameraData(cam_id=c, size=(640, 480), ignore=ig) for c, ig in zip(cams, ignore)})
        net.apply_to(applied)
        posed = np.array([applied.cameras[c].rotation is not None for c in cams])
        anchor = [c for c in cams if posed[c] and np.array_equal(applied.cameras[c].rotation, np.eye(3))
                  and not np.any(applied.cameras[c].translation)]
        np.savez_compressed(
            OUT / f"pnet_{case:02d}.npz",
            cams=np.array(cams), ignore=np.array(ignore),
            in_keys=np.array(keys, dtype=np.int64), in_R=np.array([poses[k][0] for k in keys]), in_t=np.array([poses[k][1] for k in keys]),
            in_rmse=np.array([poses[k][2] for k in keys]),
            rel_keys=np.array([(k[0][0], k[0][1], k[1], k[2]) for k in rel_keys], dtype=np.int64).reshape(-1, 4),
            rel_R=np.array([rel[k].rotation for k in rel_keys]).reshape(-1, 3, 3), rel_t=np.array([rel[k].translation for k in rel_keys]).reshape(-1, 3),
            kept=np.array(kept, dtype=np.int64).reshape(-1, 4),
            agg_keys=np.array(agg_keys, dtype=np.int64).reshape(-1, 2), agg_R=np.array([agg[p].rotation for p in agg_keys]).reshape(-1, 3, 3),
            agg_t=np.array([agg[p].translation for p in agg_keys]).reshape(-1, 3), errors=np.array([errors[p] for p in agg_keys]),
            net_keys=np.array(net_keys, dtype=np.int64).reshape(-1, 2), net_R=np.array([net._pairs[p].rotation for p in net_keys]).reshape(-1, 3, 3),
            net_t=np.array([net._pairs[p].translation for p in net_keys]).reshape(-1, 3),
            net_err=np.array([net._pairs[p].error_score for p in net_keys]),
            posed=posed, anchor=np.array(anchor, dtype=np.int64),
            out_R=np.array([applied.cameras[c].rotation if posed[c] else np.full((3, 3), np.nan) for c in cams]),
            out_t=np.array([np.ravel(applied.cameras[c].translation) if posed[c] else np.full(3, np.nan) for c in cams]),
        )
        print(f"pnet_{case:02d}: {len(keys)} views, {len(rel_keys)} relative, {len(kept)} kept, {len(agg_keys)} pairs, {len(net_keys)} links, "
              f"posed {posed.astype(int).tolist()}, anchor {anchor}")


if __name__ == "__main__":
    main()
