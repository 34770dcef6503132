"""caliscope_amd: multi-camera calibration and reconstruction on the MI355X.  The sub-modules are imported by name; the two entry points
of the per-recording stage, the uncertainty report and the reliability report are also reachable from the package (loaded on first use, so that importing the
package stays as cheap)."""

_EXPORTS = {"reconstruct_trajectories": "caliscope_amd.reconstruction", "reconstruct_xyz": "caliscope_amd.reconstruction",
            "RefineOptions": "caliscope_amd.trajectory_refinement", "CovarianceOptions": "caliscope_amd.trajectory_uncertainty",
            "SmootherOptions": "caliscope_amd.trajectory_smoother", "smooth_trajectories": "caliscope_amd.trajectory_smoother",
            "smoothed_frame": "caliscope_amd.trajectory_smoother", "DeviceTrajectorySmoother": "caliscope_amd.trajectory_smoother",
            "Skeleton": "caliscope_amd.trajectory_skeleton", "SkeletonOptions": "caliscope_amd.trajectory_skeleton",
            "adjust_skeleton": "caliscope_amd.trajectory_skeleton", "DeviceSkeletonAdjuster": "caliscope_amd.trajectory_skeleton",
            "TimeOffsetOptions": "caliscope_amd.time_offsets", "TimeOffsets": "caliscope_amd.time_offsets",
            "estimate_time_offsets": "caliscope_amd.time_offsets", "apply_time_offsets": "caliscope_amd.time_offsets",
            "DeviceTimeOffsetSolver": "caliscope_amd.time_offsets",
            "UncertaintyReport": "caliscope_amd.uncertainty", "DeviceUncertainty": "caliscope_amd.uncertainty",
            "ReliabilityReport": "caliscope_amd.reliability", "DeviceReliability": "caliscope_amd.reliability"}

__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        import importlib

        return getattr(importlib.import_module(_EXPORTS[name]), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
