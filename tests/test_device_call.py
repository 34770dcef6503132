"""csrc/device_call.h (the buffers and the device selection of every one-shot device call) on the CPU: tests/native/device_call_check.cpp
compiled by g++ against the stand-in HIP of tests/native/fake_hip with AddressSanitizer and UndefinedBehaviorSanitizer, run as a
program of its own.  No GPU, no Python in the process under the sanitizers."""
import subprocess

from tests.native_build import CSRC, NATIVE, compile_native

# the sanitizer runtimes linked statically: the program does not depend on the order in which shared libraries are loaded
SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan")


def test_device_buffers_under_injected_failures_and_sanitizers():
    """A failure injected at every allocation and every copy of a representative call: nothing later reaches HIP, status() is the first
    failure, out() writes nothing, every block is freed exactly once; the success path (round trip, zero count, null host pointer, a
    size beyond size_t refused before the allocator) and the three answers of select_device.  Exit status 0, and no sanitizer report."""
    exe = compile_native(NATIVE / "device_call_check.cpp", flags=SANITIZE, include=(NATIVE / "fake_hip", CSRC), shared=False)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(proc.stdout[-3000:], proc.stderr[-3000:])
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    assert "Sanitizer" not in proc.stderr and "runtime error" not in proc.stderr
    assert "all checks passed" in proc.stdout
