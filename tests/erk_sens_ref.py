"""ctypes loader of the Tsit45 checker with forward sensitivities (tests/erk_sens_ref/erk_sens_ref.cpp): TEST INFRASTRUCTURE ONLY.  Builds
tests/erk_sens_ref/_build/liberk_sens_ref.so on first use with the flags of the plain checker (tests/erk_ref.py: no contraction, no fast math).  The library has its own
model registry and pow switch: load DiffSL host twins and set the pow through THIS module."""
import ctypes as C
import os
import subprocess

import numpy as np

import erk_ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "erk_sens_ref", "erk_sens_ref.cpp")
_PLAIN = os.path.join(_HERE, "erk_ref", "erk_ref.cpp")
_LIB = os.path.join(_HERE, "erk_sens_ref", "_build", "liberk_sens_ref.so")
_ORACLE = os.path.join(os.path.dirname(_HERE), "oracle")

_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_long)
_lib = None


def build(force=False):
    deps = [_SRC, _PLAIN] + [os.path.join(_ORACLE, f) for f in os.listdir(_ORACLE) if f.endswith(".hpp")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        os.makedirs(os.path.dirname(_LIB), exist_ok=True)
        tmp = _LIB + ".tmp%d" % os.getpid()
        subprocess.run(["g++"] + erk_ref.CXXFLAGS + ["-shared", "-o", tmp, _SRC, "-ldl"], check=True)
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.erk_model_dims.argtypes = [C.c_int, C.c_int, _ip]
        L.erk_load_external_model.argtypes = [C.c_char_p]
        L.erks_solve_to_points.argtypes = [C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_double, C.c_double, C.c_double, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _lp]
        L.erks_solve_ensemble.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_int, C.c_double, C.c_double, C.c_double, _dp, C.c_int, _dp, C.c_int,
                                          C.c_int, C.c_int, _dp, _dp, _lp, _ip, _lp, _dp]
        _lib = L
    return _lib


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def set_det_pow(on):
    """pow() of the step-size controller: libm (the reference's) or include/diffsol_detpow.h (bit-comparable with the device kernel)."""
    lib().erk_set_det_pow(C.c_int(1 if on else 0))


def model_dims(model, model_size=0):
    o = (C.c_int * 3)()
    lib().erk_model_dims(model, model_size, o)
    return dict(n=o[0], nparams=o[1], has_mass=bool(o[2]))


def load_external_model(so_path):
    mid = lib().erk_load_external_model(so_path.encode())
    if mid < 0:
        raise RuntimeError("checker: cannot load " + so_path)
    return mid


def _sens_atol(sens_atol, n):
    """None: the sensitivities stay out of the error control; a scalar / [1]: one value for every state; [n]: per state"""
    if sens_atol is None:
        return _d(np.zeros(1)) + (0,)
    sa = np.asarray(sens_atol, dtype=float).reshape(-1)
    assert sa.size in (1, n)
    return _d(sa) + (sa.size,)


def _raise(rc):
    raise RuntimeError({-100: "MassMatrixNotSupported", -101: "checker: the model has no parameter sensitivities"}.get(rc, f"checker: OdeErr {-rc}"))


def solve_to_points(model, p, t_points, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, sens_rtol=1e-6, sens_atol=(1e-6,)):
    """the reference's test harness on one IVP.  Returns (y [npoints, n], sens [nparams, npoints, n], dict(steps, error_test_failures, rhs_calls, jac_muls))."""
    n = model_dims(model, model_size)["n"]
    p_a, p_p = _d(np.asarray(p, dtype=float).reshape(-1))
    a_a, a_p = _d(np.broadcast_to(np.asarray(atol, dtype=float).reshape(-1), (n,)))
    sa_a, sa_p, nsa = _sens_atol(sens_atol, n)
    t_a, t_p = _d(t_points)
    y = np.empty((t_a.size, n))
    s = np.empty((t_a.size, p_a.size, n))
    cnt = (C.c_long * 4)()
    rc = lib().erks_solve_to_points(model, model_size, p_p, p_a.size, rtol, a_p, t0, h0, sens_rtol, sa_p, nsa, t_p, t_a.size, y.ctypes.data_as(_dp), s.ctypes.data_as(_dp), cnt)
    if rc != 0:
        _raise(rc)
    return y, s.transpose(1, 0, 2), dict(steps=cnt[0], error_test_failures=cnt[1], rhs_calls=cnt[2], jac_muls=cnt[3])


def solve_ensemble(model, p, t_eval, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, sens_rtol=1e-6, sens_atol=(1e-6,), group=1, nthreads=8,
                   options=None):
    """solve_dense_sensitivities per member (group 1) or per lock-step group of `group` members.  atol: [n] / scalar, or [nsys, n] per member.  options: see
    erk_ref.options_array.
    Returns dict(y [nsys, nt, n], sens [nparams, nsys, nt, n], stats [nsys, 5], status [nsys], rhs_calls [nsys], jac_muls [nsys], failed)."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    nsys, np_ = p.shape
    n = model_dims(model, model_size)["n"]
    at = np.asarray(atol, dtype=float)
    rows = nsys if at.ndim == 2 else 1
    a_a, a_p = _d(at.reshape(nsys, n) if at.ndim == 2 else np.broadcast_to(at.reshape(-1), (n,)))
    sa_a, sa_p, nsa = _sens_atol(sens_atol, n)
    te, te_p = _d(np.atleast_1d(t_eval))
    y = np.full((nsys, te.size, n), np.nan)
    s = np.full((nsys, te.size, np_, n), np.nan)
    stats = np.zeros((nsys, 5), dtype=np.int64)
    calls = np.zeros((nsys, 2), dtype=np.int64)
    status = np.zeros(nsys, dtype=np.int32)
    o_a, o_p = erk_ref.options_array(options)
    failed = lib().erks_solve_ensemble(model, model_size, nsys, p.ctypes.data_as(_dp), np_, rtol, a_p, rows, t0, h0, sens_rtol, sa_p, nsa, te_p, te.size, nthreads, group,
                                       y.ctypes.data_as(_dp), s.ctypes.data_as(_dp), stats.ctypes.data_as(_lp), status.ctypes.data_as(_ip), calls.ctypes.data_as(_lp), o_p)
    if failed < 0:
        _raise(failed)
    return dict(y=y, sens=np.ascontiguousarray(s.transpose(2, 0, 1, 3)), stats=stats, status=status, rhs_calls=calls[:, 0], jac_muls=calls[:, 1], failed=int(failed))
