"""ctypes loader of the wavefront-maximum check (tests/wave_reduce_check/wave_reduce_check.hip): TEST INFRASTRUCTURE ONLY.  Builds
tests/wave_reduce_check/_build/libwave_reduce_check.so for gfx950 on first use (hipcc cross-compiles without a GPU; __graft_entry__.build() calls build() so that the
library travels with the tree)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "wave_reduce_check", "wave_reduce_check.hip")
_LIB = os.path.join(_HERE, "wave_reduce_check", "_build", "libwave_reduce_check.so")
_DEP = os.path.join(os.path.dirname(_HERE), "diffsol_amd", "csrc", "dsh_device.hpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIPFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-Wall"]  # the device library's flags (csrc/Makefile)

_lib = None


def build(force=False):
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in (_SRC, _DEP)):
        os.makedirs(os.path.dirname(_LIB), exist_ok=True)
        tmp = _LIB + ".tmp%d" % os.getpid()
        subprocess.run([HIPCC] + HIPFLAGS + ["-shared", "-o", tmp, _SRC], check=True)
        os.replace(tmp, _LIB)
    return _LIB


def wave_max_both(patterns):
    """patterns: [npat, 64] doubles, one wavefront each.  Returns (bits of wave_max_nonneg_f64, bits of wave_max_u64(d2u(.))) as two uint64 arrays [npat]."""
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.wave_max_both.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    a = np.ascontiguousarray(patterns, dtype=np.float64)
    assert a.ndim == 2 and a.shape[1] == 64
    new, old = np.zeros(a.shape[0], dtype=np.uint64), np.zeros(a.shape[0], dtype=np.uint64)
    rc = _lib.wave_max_both(a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0], new.ctypes.data_as(C.POINTER(C.c_ulonglong)), old.ctypes.data_as(C.POINTER(C.c_ulonglong)))
    if rc != 0:
        raise RuntimeError(f"wave_max_both: HIP error {rc}")
    return new, old
