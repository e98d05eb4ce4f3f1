"""ctypes loader of the Tsit45 checker (tests/erk_ref/erk_ref.cpp): TEST INFRASTRUCTURE ONLY.  Builds tests/erk_ref/_build/liberk_ref.so on first use with the flags
of the oracle's Makefile (no contraction, no fast math)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "erk_ref", "erk_ref.cpp")
_LIB = os.path.join(_HERE, "erk_ref", "_build", "liberk_ref.so")
_ORACLE = os.path.join(os.path.dirname(_HERE), "oracle")
CXXFLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-pthread"]

_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_long)
_lib = None


def build(force=False):
    deps = [_SRC] + [os.path.join(_ORACLE, f) for f in os.listdir(_ORACLE) if f.endswith(".hpp")]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        os.makedirs(os.path.dirname(_LIB), exist_ok=True)
        tmp = _LIB + ".tmp%d" % os.getpid()
        subprocess.run(["g++"] + CXXFLAGS + ["-shared", "-o", tmp, _SRC, "-ldl"], check=True)
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.erk_tableau.argtypes = [_dp]
        L.erk_model_dims.argtypes = [C.c_int, C.c_int, _ip]
        L.erk_load_external_model.argtypes = [C.c_char_p]
        L.erk_solve_to_points.argtypes = [C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_double, C.c_double, _dp, C.c_int, C.c_int, _dp, _lp]
        L.erk_solve_ensemble.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_int, C.c_double, C.c_double, _dp, C.c_int, C.c_int, C.c_int,
                                         C.c_int, _dp, _dp, _lp, _ip, _dp, _ip, _ip, _dp]
        _lib = L
    return _lib


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


OPTION_DEFAULTS = dict(max_error_test_failures=40, min_timestep=1e-13, pi_control_integral=0.5, pi_control_proportional=0.0, max_steps=0)


def options_array(options):
    """the `options` argument of the three *_solve_ensemble entries: None (every default), or the five doubles of SolveOptions (erk_ref.cpp) from a dict of
    max_error_test_failures, min_timestep, pi_control_integral, pi_control_proportional (the reference's OdeSolverOptions fields ExplicitRk reads) and max_steps (the
    device ABI's step cap, which the reference does not have; <= 0: 10 000 000)"""
    if options is None:
        return None, None
    unknown = set(options) - set(OPTION_DEFAULTS)
    if unknown:
        raise KeyError(f"checker: unknown options {sorted(unknown)}")
    return _d([float({**OPTION_DEFAULTS, **options}[k]) for k in OPTION_DEFAULTS])


def set_det_pow(on):
    """pow() of the step-size controller: libm (the reference's) or include/diffsol_detpow.h (bit-comparable with the device kernel)."""
    lib().erk_set_det_pow(C.c_int(1 if on else 0))


def tableau():
    out = np.zeros(99)
    lib().erk_tableau(out.ctypes.data_as(_dp))
    return dict(c=out[0:7].tolist(), b=out[7:14].tolist(), d=out[14:21].tolist(), a=out[21:70].reshape(7, 7).tolist(), beta=out[70:98].reshape(4, 7).tolist(),
                order=int(out[98]))


def model_dims(model, model_size=0):
    o = (C.c_int * 3)()
    lib().erk_model_dims(model, model_size, o)
    return dict(n=o[0], nparams=o[1], has_mass=bool(o[2]))


def load_external_model(so_path):
    mid = lib().erk_load_external_model(so_path.encode())
    if mid < 0:
        raise RuntimeError("checker: cannot load " + so_path)
    return mid


def solve_to_points(model, p, t_points, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, use_tstop=False):
    """the reference's test harness on one IVP.  Returns (y [npoints, n], dict(steps, error_test_failures, rhs_calls)); raises on an OdeErr / a mass matrix."""
    n = model_dims(model, model_size)["n"]
    p_a, p_p = _d(np.asarray(p, dtype=float).reshape(-1))
    a_a, a_p = _d(np.broadcast_to(np.asarray(atol, dtype=float).reshape(-1), (n,)))
    t_a, t_p = _d(t_points)
    y = np.empty((t_a.size, n))
    cnt = (C.c_long * 3)()
    rc = lib().erk_solve_to_points(model, model_size, p_p, p_a.size, rtol, a_p, t0, h0, t_p, t_a.size, 1 if use_tstop else 0, y.ctypes.data_as(_dp), cnt)
    if rc != 0:
        raise RuntimeError("MassMatrixNotSupported" if rc == -100 else f"checker: OdeErr {-rc}")
    return y, dict(steps=cnt[0], error_test_failures=cnt[1], rhs_calls=cnt[2])


def solve_ensemble(model, p, t_eval, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, group=1, nthreads=8, steps_cap=0, options=None):
    """solve_dense (steps_cap = 0; t_eval the save points) or solve (steps_cap > 0; t_eval = [t_final]) per member (group 1) or per lock-step group of `group`
    members.  atol: [n] / scalar, or [nsys, n] per member.  options: see options_array.  Returns dict(y [nsys, cols, n], t [nsys, cols] (steps only), stats [nsys, 5], status, t_root, root_idx, ncols, failed)."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    nsys, np_ = p.shape
    n = model_dims(model, model_size)["n"]
    at = np.asarray(atol, dtype=float)
    rows = nsys if at.ndim == 2 else 1
    a_a, a_p = _d(at.reshape(nsys, n) if at.ndim == 2 else np.broadcast_to(at.reshape(-1), (n,)))
    te, te_p = _d(np.atleast_1d(t_eval))
    cols = steps_cap if steps_cap > 0 else te.size
    y = np.full((nsys, cols, n), np.nan)
    t = np.full((nsys, max(steps_cap, 1)), np.nan)
    stats = np.zeros((nsys, 5), dtype=np.int64)
    status, ridx, ncols = (np.zeros(nsys, dtype=np.int32) for _ in range(3))
    troot = np.full(nsys, np.nan)
    o_a, o_p = options_array(options)
    failed = lib().erk_solve_ensemble(model, model_size, nsys, p.ctypes.data_as(_dp), np_, rtol, a_p, rows, t0, h0, te_p, te.size, nthreads, group, steps_cap,
                                      y.ctypes.data_as(_dp), t.ctypes.data_as(_dp), stats.ctypes.data_as(_lp), status.ctypes.data_as(_ip), troot.ctypes.data_as(_dp),
                                      ridx.ctypes.data_as(_ip), ncols.ctypes.data_as(_ip), o_p)
    return dict(y=y, t=t, stats=stats, status=status, t_root=troot, root_idx=ridx, ncols=ncols, failed=int(failed))
