"""ctypes loader of the ballot-decision check (tests/ballot_decide_check/ballot_decide_check.hip): TEST INFRASTRUCTURE ONLY.  Builds
tests/ballot_decide_check/_build/libballot_decide_check.so for gfx950 on first use (hipcc cross-compiles without a GPU; __graft_entry__.build() calls build() so
that the library travels with the tree)."""
import ctypes as C
import os
import subprocess

import numpy as np

from fast_pow_check import FASTFLAGS, HIPCC

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "ballot_decide_check", "ballot_decide_check.hip")
_LIB = os.path.join(_HERE, "ballot_decide_check", "_build", "libballot_decide_check.so")
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


def newton_first(m, eta08, tol):
    """m [nw, 64]: the lanes' weighted mean squares of the first Newton update, one wavefront per row; eta08, tol: one value per wavefront (or a scalar).
    Returns (new decision, eta08 * sqrt(wave max) < tol, took the undecided path) as three bool arrays [nw], all evaluated on the device."""
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        dp = C.POINTER(C.c_double)
        _lib.newton_first_both.argtypes = [dp, dp, dp, C.c_int, C.POINTER(C.c_int)]
    m = np.ascontiguousarray(m, dtype=np.float64)
    assert m.ndim == 2 and m.shape[1] == 64, m.shape
    nw = m.shape[0]
    eta08 = np.ascontiguousarray(np.broadcast_to(np.asarray(eta08, dtype=np.float64), (nw,)))
    tol = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, dtype=np.float64), (nw,)))
    out = np.zeros((nw, 3), dtype=np.int32)
    dp = C.POINTER(C.c_double)
    rc = _lib.newton_first_both(m.ctypes.data_as(dp), eta08.ctypes.data_as(dp), tol.ctypes.data_as(dp), nw, out.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != 0:
        raise RuntimeError(f"newton_first_both: error {rc}")
    return out[:, 0].astype(bool), out[:, 1].astype(bool), out[:, 2].astype(bool)

