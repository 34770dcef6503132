"""The launch geometry of the blocked Cholesky (csrc/chol_schedule.h, shared by k_chol_step's role decode and enqueue_chol_factor's grid) replayed
on the host by tests/native/chol_schedule_check.cpp: single writers, no read of a block another workgroup of the launch writes (the side slot of
the early update included), every block updated by P_0 .. P_j-1 once each in order before the launch that solves it — for 1 to 40 column blocks
and both schedules (the parent's, CBA_CHOL_EARLY=0, passes all but "column k + 1 is complete at launch k")."""
import subprocess

from tests.native_build import CSRC, NATIVE, compile_native


def test_schedule_replay():
    exe = compile_native(NATIVE / "chol_schedule_check.cpp", flags=("-Wall", "-Werror"), include=(CSRC,), shared=False)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(proc.stdout[-3000:], proc.stderr[-3000:])
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "all checks passed" in proc.stdout
