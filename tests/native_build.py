"""The one place where the tests compile C++ for the host: the g++ command line, the temporary directory and the once-per-process
cache of what was built and loaded.  The harness modules (tests/*_native.py) and the fixtures that need a host build call
``load_native`` / ``compile_native`` with their sources, their own flags and include directories, and keep their ``argtypes``."""

from __future__ import annotations

import ctypes as C
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "caliscope_amd" / "csrc"
INCLUDE = ROOT / "include"
NATIVE = ROOT / "tests" / "native"

_TMP = tempfile.TemporaryDirectory(prefix="native_build_")  # removed when the interpreter exits
_BUILT: dict[tuple, Path] = {}
_LOADED: dict[tuple, C.CDLL] = {}


def compile_native(*sources, flags=(), include=(), shared=True) -> Path:
    """``g++ -O2 -std=c++17`` of ``sources`` with ``flags`` and ``-I`` for every directory of ``include``: a shared library, or with
    ``shared=False`` a program.  Built once per process and argument set, in a temporary directory; returns the file."""
    key = (tuple(map(str, sources)), tuple(flags), tuple(map(str, include)), shared)
    if key not in _BUILT:
        stem = Path(key[0][0]).stem
        out = Path(tempfile.mkdtemp(prefix=f"{stem}_", dir=_TMP.name)) / (f"lib{stem}.so" if shared else stem)
        subprocess.run(["g++", "-O2", "-std=c++17", *flags, *(("-shared", "-fPIC") if shared else ()), *(f"-I{d}" for d in key[2]), *key[0], "-o", str(out)],
                       check=True)
        _BUILT[key] = out
    return _BUILT[key]


def load_native(*sources, flags=(), include=()) -> C.CDLL:
    """The shared library of ``compile_native``, loaded once per process (one ``CDLL`` object, so ``argtypes`` set on it stay)."""
    key = (tuple(map(str, sources)), tuple(flags), tuple(map(str, include)))
    if key not in _LOADED:
        _LOADED[key] = C.CDLL(str(compile_native(*sources, flags=flags, include=include)))
    return _LOADED[key]
