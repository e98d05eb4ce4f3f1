"""ctypes loader of the Tsit45 checker with integrated outputs (tests/erk_out_ref/erk_out_ref.cpp): TEST INFRASTRUCTURE ONLY.  Builds
tests/erk_out_ref/_build/liberk_out_ref.so on first use with the flags of the plain checker (tests/erk_ref.py: no contraction, no fast math).  The library has its own
model registry and pow switch: load DiffSL host twins and set the pow through THIS module."""
import ctypes as C
import os
import subprocess

import numpy as np

import erk_ref

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "erk_out_ref", "erk_out_ref.cpp")
_PLAIN = os.path.join(_HERE, "erk_ref", "erk_ref.cpp")
_LIB = os.path.join(_HERE, "erk_out_ref", "_build", "liberk_out_ref.so")
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
        L.erko_model_nout.argtypes = [C.c_int, C.c_int]
        L.erko_solve_to_points.argtypes = [C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_double, C.c_double, C.c_int, C.c_double, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _lp]
        L.erko_solve_ensemble.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, _dp, C.c_int, _dp,
                                          C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _lp, _ip, _dp, _ip, _ip, _lp, _dp]
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
    return dict(n=o[0], nparams=o[1], has_mass=bool(o[2]), nout=lib().erko_model_nout(model, model_size))


def load_external_model(so_path):
    mid = lib().erk_load_external_model(so_path.encode())
    if mid < 0:
        raise RuntimeError("checker: cannot load " + so_path)
    return mid


def _out_atol(out_atol, nout):
    """None: the outputs stay out of the error test; a scalar / [1]: one value for every output; [nout]: one each"""
    if out_atol is None:
        return _d(np.zeros(1)) + (0,)
    oa = np.asarray(out_atol, dtype=float).reshape(-1)
    assert oa.size in (1, nout)
    return _d(oa) + (oa.size,)


def solve_to_points(model, p, t_points, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, integrate_out=True, out_rtol=1e-6, out_atol=None):
    """the reference's test harness on one IVP.  Returns (y [npoints, n], g [npoints, nout] or None, dict(steps, error_test_failures, rhs_calls))."""
    dims = model_dims(model, model_size)
    n, nout = dims["n"], dims["nout"]
    p_a, p_p = _d(np.asarray(p, dtype=float).reshape(-1))
    a_a, a_p = _d(np.broadcast_to(np.asarray(atol, dtype=float).reshape(-1), (n,)))
    oa_a, oa_p, noa = _out_atol(out_atol, nout)
    t_a, t_p = _d(t_points)
    y = np.empty((t_a.size, n))
    g = np.empty((t_a.size, nout))
    cnt = (C.c_long * 3)()
    rc = lib().erko_solve_to_points(model, model_size, p_p, p_a.size, rtol, a_p, t0, h0, 1 if integrate_out else 0, out_rtol, oa_p, noa, t_p, t_a.size,
                                    y.ctypes.data_as(_dp), g.ctypes.data_as(_dp), cnt)
    if rc != 0:
        raise RuntimeError("MassMatrixNotSupported" if rc == -100 else f"checker: OdeErr {-rc}")
    return y, (g if integrate_out else None), dict(steps=cnt[0], error_test_failures=cnt[1], rhs_calls=cnt[2])


def solve_ensemble(model, p, t_eval, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, group=1, nthreads=8, steps_cap=0, integrate_out=True, out_rtol=1e-6,
                   out_atol=None, options=None):
    """solve_dense (steps_cap = 0; t_eval the save points) or solve (steps_cap > 0; t_eval = [t_final]) per member (group 1) or per lock-step group of `group`
    members, with the outputs integrated.  atol: [n] / scalar, or [nsys, n] per member.  options: see erk_ref.options_array.  Returns dict(y [nsys, cols, n] (the states), g [nsys, cols, nout] (None without
    integrate_out), t [nsys, cols] (steps only), stats [nsys, 5], status, t_root, root_idx, ncols, rhs_calls, failed)."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    nsys, np_ = p.shape
    dims = model_dims(model, model_size)
    n, nout = dims["n"], dims["nout"]
    at = np.asarray(atol, dtype=float)
    rows = nsys if at.ndim == 2 else 1
    a_a, a_p = _d(at.reshape(nsys, n) if at.ndim == 2 else np.broadcast_to(at.reshape(-1), (n,)))
    oa_a, oa_p, noa = _out_atol(out_atol, nout)
    te, te_p = _d(np.atleast_1d(t_eval))
    cols = steps_cap if steps_cap > 0 else te.size
    y = np.full((nsys, cols, n), np.nan)
    g = np.full((nsys, cols, nout), np.nan)
    t = np.full((nsys, max(steps_cap, 1)), np.nan)
    stats = np.zeros((nsys, 5), dtype=np.int64)
    calls = np.zeros(nsys, dtype=np.int64)
    status, ridx, ncols = (np.zeros(nsys, dtype=np.int32) for _ in range(3))
    troot = np.full(nsys, np.nan)
    o_a, o_p = erk_ref.options_array(options)
    failed = lib().erko_solve_ensemble(model, model_size, nsys, p.ctypes.data_as(_dp), np_, rtol, a_p, rows, t0, h0, 1 if integrate_out else 0, out_rtol, oa_p, noa, te_p,
                                       te.size, nthreads, group, steps_cap, y.ctypes.data_as(_dp), g.ctypes.data_as(_dp), t.ctypes.data_as(_dp), stats.ctypes.data_as(_lp),
                                       status.ctypes.data_as(_ip), troot.ctypes.data_as(_dp), ridx.ctypes.data_as(_ip), ncols.ctypes.data_as(_ip), calls.ctypes.data_as(_lp), o_p)
    return dict(y=y, g=(g if integrate_out else None), t=t, stats=stats, status=status, t_root=troot, root_idx=ridx, ncols=ncols, rhs_calls=calls, failed=int(failed))
