"""ctypes loader of the controller-power check (tests/ctrl_pow_check/ctrl_pow_check.hip): TEST INFRASTRUCTURE ONLY.  Builds
tests/ctrl_pow_check/_build/libctrl_pow_check.so for gfx950 on first use (hipcc cross-compiles without a GPU; __graft_entry__.build() calls build() so that the
library travels with the tree).  The long-double reference is fast_pow_check.err_ulp."""
import ctypes as C
import os
import subprocess

import numpy as np

from fast_pow_check import FASTFLAGS, HIPCC

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ctrl_pow_check", "ctrl_pow_check.hip")
_LIB = os.path.join(_HERE, "ctrl_pow_check", "_build", "libctrl_pow_check.so")
_CSRC = os.path.join(os.path.dirname(_HERE), "diffsol_amd", "csrc")
_DEPS = [os.path.join(_CSRC, h) for h in ("dsh_adaptive_kernel.hpp", "dsh_resident.hpp", "dsh_device.hpp", "dsh_internal.hpp")]

_lib = None


def build(force=False):
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in [_SRC] + _DEPS):
        os.makedirs(os.path.dirname(_LIB), exist_ok=True)
        tmp = _LIB + ".tmp%d" % os.getpid()
        subprocess.run([HIPCC] + FASTFLAGS + ["-shared", "-o", tmp, _SRC], check=True)
        os.replace(tmp, _LIB)
    return _LIB


def ctrl_pow_both(x, k):
    """x, k: one (argument, k) pair per lane, dealt to wavefronts of 64 in order; the last wavefront is padded with (1.0, 1), which is inside the helper's domain.
    Returns (inv_root_2k_group, pow(x, -(0.5 / k))) as two float64 arrays, both evaluated on the device."""
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        _lib.ctrl_pow_both.argtypes = [dp, ip, C.c_int, dp, dp]
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.int32), x.shape))
    n, pad = len(x), (-len(x)) % 64
    xp, kp = np.concatenate([x, np.ones(pad)]), np.concatenate([k, np.ones(pad, dtype=np.int32)])
    new, ref = np.zeros_like(xp), np.zeros_like(xp)
    dp = C.POINTER(C.c_double)
    rc = _lib.ctrl_pow_both(xp.ctypes.data_as(dp), kp.ctypes.data_as(C.POINTER(C.c_int)), len(xp), new.ctypes.data_as(dp), ref.ctypes.data_as(dp))
    if rc != 0:
        raise RuntimeError(f"ctrl_pow_both: error {rc}")
    return new[:n], ref[:n]
