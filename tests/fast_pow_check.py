"""ctypes loader of the fast-power check (tests/fast_pow_check/fast_pow_check.hip): TEST INFRASTRUCTURE ONLY.  Builds
tests/fast_pow_check/_build/libfast_pow_check.so for gfx950 on first use (hipcc cross-compiles without a GPU; __graft_entry__.build() calls build() so that the
library travels with the tree)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "fast_pow_check", "fast_pow_check.hip")
_LIB = os.path.join(_HERE, "fast_pow_check", "_build", "libfast_pow_check.so")
_CSRC = os.path.join(os.path.dirname(_HERE), "diffsol_amd", "csrc")
_DEPS = [os.path.join(_CSRC, h) for h in ("dsh_adaptive_kernel.hpp", "dsh_resident.hpp", "dsh_device.hpp", "dsh_internal.hpp")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the FASTFLAGS of csrc/Makefile: what dsh_adaptive_fast.hip, the one user of the helpers, is compiled with
FASTFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-ffp-contract=fast", "-freciprocal-math", "-fapprox-func", "-fno-math-errno"]

_lib = None


def build(force=False):
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in [_SRC] + _DEPS):
        os.makedirs(os.path.dirname(_LIB), exist_ok=True)
        tmp = _LIB + ".tmp%d" % os.getpid()
        subprocess.run([HIPCC] + FASTFLAGS + ["-shared", "-o", tmp, _SRC], check=True)
        os.replace(tmp, _LIB)
    return _LIB


def _load():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        _lib.fast_pow_both.argtypes = [dp, ip, C.c_int, dp, dp]
        _lib.fast_pow_err_ulp.argtypes = [dp, dp, C.c_int, C.c_int, C.c_int, dp]
        _lib.fast_pow_err_ulp.restype = None
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def fast_pow_both(x, k):
    """x: arguments, k: 0 for pow_p08(x) beside pow(x, 0.8), k > 0 for root_k(x, k) beside pow(x, 1.0 / k) (one int, or one per argument).
    Returns (helper, plain pow) as two float64 arrays, both evaluated on the device."""
    lib = _load()
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.int32), x.shape))
    new, ref = np.zeros_like(x), np.zeros_like(x)
    rc = lib.fast_pow_both(_dp(x), k.ctypes.data_as(C.POINTER(C.c_int)), len(x), _dp(new), _dp(ref))
    if rc != 0:
        raise RuntimeError(f"fast_pow_both: HIP error {rc}")
    return new, ref


def err_ulp(x, got, num, den):
    """|got - x^(num/den)| / x^(num/den) in units of 2^-53, the power by powl in 80-bit long double on the host."""
    lib = _load()
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    got = np.ascontiguousarray(got, dtype=np.float64).ravel()
    assert x.shape == got.shape
    err = np.zeros_like(x)
    lib.fast_pow_err_ulp(_dp(x), _dp(got), len(x), num, den, _dp(err))
    return err
