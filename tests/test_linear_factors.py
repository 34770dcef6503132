"""The no-residual form of ``project_factors`` (csrc/ba_math.h) — what ``k_tprep`` and ``k_jv`` evaluate per observation under a linear loss, where
the residual would reach them only through a row scale of exactly 1.0 — against the full form, on the host (tests/native/linear_factors_check.cpp):
G, Yr, Aint and B bit for bit, for pinhole and fisheye rows, six and nine parameters, general and small rotation angles, and points on the optical
axis.  Runs without a GPU."""
import subprocess

from tests.native_build import CSRC, NATIVE, compile_native


def test_no_residual_factors_are_bit_equal():
    exe = compile_native(NATIVE / "linear_factors_check.cpp", flags=("-Wall", "-Werror", "-Wno-unknown-pragmas"), include=(CSRC,), shared=False)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(proc.stdout[-3000:], proc.stderr[-3000:])
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "all checks passed" in proc.stdout
    assert proc.stdout.count("bit-equal") == 20  # 2 models x 2 parameter counts x (2 angles x 2 points + 1)
