"""The solver's launch sequence of the blocked Cholesky with the paired first launch (csrc/chol_schedule.h: launches -1 and 0 as one, D_0 factored
privately by every workgroup, D_0 and U_10 read from side slots) replayed on the host by tests/native/chol_schedule_pair_check.cpp for 1 to 40 column
blocks, with and without T: single writers, no read of a block another workgroup of the launch writes, every block updated by P_0 .. P_j-1 once each
in order before its solve or factorisation, and every block of W, Xinv and T with the unpaired sequence's history at the end."""
import subprocess

from tests.native_build import CSRC, NATIVE, compile_native


def test_paired_schedule_replay():
    exe = compile_native(NATIVE / "chol_schedule_pair_check.cpp", flags=("-Wall", "-Werror"), include=(CSRC,), shared=False)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(proc.stdout[-3000:], proc.stderr[-3000:])
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "all checks passed" in proc.stdout
