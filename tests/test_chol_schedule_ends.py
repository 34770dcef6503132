"""The solver's launch sequence of the dense solve with its last launch folded into the backward substitution (k_chol_last_apply; csrc/chol_schedule.h:
chol_last_apply_for_each_read / _action) replayed on the host by tests/native/chol_schedule_ends_check.cpp for 1 to 40 column blocks, both schedules,
with and without T: single writers per launch, no read of a block another workgroup of the launch writes, every block updated by P_0 .. P_j-1 once
each in order before it is solved, every block of T given its terms once each in order from final operands, and the last launch's private rhs
block, private block of T and row sums fed only by what earlier launches finished."""
import subprocess

from tests.native_build import CSRC, NATIVE, compile_native


def test_schedule_ends_replay():
    exe = compile_native(NATIVE / "chol_schedule_ends_check.cpp", flags=("-Wall", "-Werror"), include=(CSRC,), shared=False)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(proc.stdout[-3000:], proc.stderr[-3000:])
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "all checks passed" in proc.stdout
