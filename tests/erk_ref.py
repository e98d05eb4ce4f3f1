"""ctypes loader of the Tsit45 checker (tests/erk_ref/erk_ref.cpp): TEST INFRASTRUCTURE ONLY.  Builds tests/erk_ref/_build/liberk_ref.so on first use with the flags
of the oracle's Makefile (no contraction, no fast math).  One library serves the three modes of the checker — plain (this module's solve_*), with forward
sensitivities (erk_sens_ref.py) and with integrated outputs (erk_out_ref.py) — so it has one model registry and one pow switch: a model id or the switch set through
any of the three modules holds in all of them."""
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

PLAIN, SENS, INTEGRATE_OUT = 0, 1, 2   # ErkMode::kind


class _Mode(C.Structure):   # ErkMode of erk_ref.cpp
    _fields_ = [("kind", C.c_int), ("rtol", C.c_double), ("atol", _dp), ("natol", C.c_int)]


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
        mp = C.POINTER(_Mode)
        L.erk_tableau.argtypes = [_dp]
        L.erk_model_dims.argtypes = [C.c_int, C.c_int, _ip]
        L.erk_model_nout.argtypes = [C.c_int, C.c_int]
        L.erk_load_external_model.argtypes = [C.c_char_p]
        L.erk_solve_to_points.argtypes = [C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_double, C.c_double, mp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _lp]
        L.erk_solve_ensemble.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_int, C.c_double, C.c_double, mp, _dp, C.c_int, C.c_int, C.c_int,
                                         C.c_int, _dp, _dp, _dp, _dp, _lp, _ip, _dp, _ip, _ip, _lp, _dp]
        _lib = L
    return _lib


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _ptr(a, typ=_dp):
    return None if a is None else a.ctypes.data_as(typ)


OPTION_DEFAULTS = dict(max_error_test_failures=40, min_timestep=1e-13, pi_control_integral=0.5, pi_control_proportional=0.0, max_steps=0)


def options_array(options):
    """the `options` argument of erk_solve_ensemble: None (every default), or the five doubles of SolveOptions (erk_ref.cpp) from a dict of
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
    return dict(n=o[0], nparams=o[1], has_mass=bool(o[2]), nout=lib().erk_model_nout(model, model_size))


def load_external_model(so_path):
    mid = lib().erk_load_external_model(so_path.encode())
    if mid < 0:
        raise RuntimeError("checker: cannot load " + so_path)
    return mid


def _mode(kind, aug_rtol, aug_atol, size):
    """the ErkMode of a solve (null: plain) with the tolerances of its augmented part.  aug_atol None: the part stays out of the error test; a scalar / [1]: one
    value for every component; [size]: one each (size: n for the sensitivities, nout for the outputs)"""
    if kind == PLAIN:
        return None, None
    a = np.zeros(1) if aug_atol is None else np.asarray(aug_atol, dtype=float).reshape(-1)
    assert a.size in (1, size)
    a_a, a_p = _d(a)
    return a_a, C.byref(_Mode(kind, aug_rtol, a_p, 0 if aug_atol is None else a.size))


def _raise(rc):
    raise RuntimeError({-100: "MassMatrixNotSupported", -101: "checker: the model has no parameter sensitivities",
                        -102: "checker: sensitivities with root functions are not restated"}.get(rc, f"checker: OdeErr {-rc}"))


def run_to_points(model, p, t_points, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, use_tstop=False, kind=PLAIN, aug_rtol=0.0, aug_atol=None):
    """erk_solve_to_points in any mode: dict(y [npoints, n], g [npoints, nout] (INTEGRATE_OUT, else None), s [npoints, nparams, n] (SENS, else None),
    counters dict(steps, error_test_failures, rhs_calls, jac_muls)); raises on an OdeErr, a mass matrix or a mode the model cannot be asked"""
    dims = model_dims(model, model_size)
    n = dims["n"]
    p_a, p_p = _d(np.asarray(p, dtype=float).reshape(-1))
    a_a, a_p = _d(np.broadcast_to(np.asarray(atol, dtype=float).reshape(-1), (n,)))
    m_a, m_p = _mode(kind, aug_rtol, aug_atol, n if kind == SENS else dims["nout"])
    t_a, t_p = _d(t_points)
    y = np.empty((t_a.size, n))
    g = np.empty((t_a.size, dims["nout"])) if kind == INTEGRATE_OUT else None
    s = np.empty((t_a.size, p_a.size, n)) if kind == SENS else None
    cnt = (C.c_long * 4)()
    rc = lib().erk_solve_to_points(model, model_size, p_p, p_a.size, rtol, a_p, t0, h0, m_p, t_p, t_a.size, 1 if use_tstop else 0, _ptr(y), _ptr(g), _ptr(s), cnt)
    if rc != 0:
        _raise(rc)
    return dict(y=y, g=g, s=s, counters=dict(steps=cnt[0], error_test_failures=cnt[1], rhs_calls=cnt[2], jac_muls=cnt[3]))


def run_ensemble(model, p, t_eval, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, group=1, nthreads=8, steps_cap=0, options=None, kind=PLAIN, aug_rtol=0.0,
                 aug_atol=None):
    """erk_solve_ensemble in any mode: solve_dense (steps_cap = 0; t_eval the save points) or solve (steps_cap > 0; t_eval = [t_final]) per member (group 1) or
    per lock-step group of `group` members.  atol: [n] / scalar, or [nsys, n] per member.  options: see options_array.  Returns dict(y [nsys, cols, n], g [nsys, cols,
    nout] (INTEGRATE_OUT, else None), s [nsys, cols, nparams, n] (SENS, else None), t [nsys, cols] (steps only), stats [nsys, 5], status, t_root, root_idx, ncols,
    rhs_calls, jac_muls [nsys], failed); raises on a mode the model cannot be asked"""
    p = np.ascontiguousarray(p, dtype=np.float64)
    nsys, np_ = p.shape
    dims = model_dims(model, model_size)
    n = dims["n"]
    at = np.asarray(atol, dtype=float)
    rows = nsys if at.ndim == 2 else 1
    a_a, a_p = _d(at.reshape(nsys, n) if at.ndim == 2 else np.broadcast_to(at.reshape(-1), (n,)))
    m_a, m_p = _mode(kind, aug_rtol, aug_atol, n if kind == SENS else dims["nout"])
    te, te_p = _d(np.atleast_1d(t_eval))
    cols = steps_cap if steps_cap > 0 else te.size
    y = np.full((nsys, cols, n), np.nan)
    g = np.full((nsys, cols, dims["nout"]), np.nan) if kind == INTEGRATE_OUT else None
    s = np.full((nsys, cols, np_, n), np.nan) if kind == SENS else None
    t = np.full((nsys, max(steps_cap, 1)), np.nan)
    stats = np.zeros((nsys, 5), dtype=np.int64)
    calls = np.zeros((nsys, 2), dtype=np.int64)
    status, ridx, ncols = (np.zeros(nsys, dtype=np.int32) for _ in range(3))
    troot = np.full(nsys, np.nan)
    o_a, o_p = options_array(options)
    failed = lib().erk_solve_ensemble(model, model_size, nsys, _ptr(p), np_, rtol, a_p, rows, t0, h0, m_p, te_p, te.size, nthreads, group, steps_cap, _ptr(y), _ptr(g),
                                      _ptr(s), _ptr(t), _ptr(stats, _lp), _ptr(status, _ip), _ptr(troot), _ptr(ridx, _ip), _ptr(ncols, _ip), _ptr(calls, _lp), o_p)
    if failed < 0:
        _raise(failed)
    return dict(y=y, g=g, s=s, t=t, stats=stats, status=status, t_root=troot, root_idx=ridx, ncols=ncols, rhs_calls=calls[:, 0].copy(), jac_muls=calls[:, 1].copy(),
                failed=int(failed))


def solve_to_points(model, p, t_points, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, use_tstop=False):
    """the reference's test harness on one IVP.  Returns (y [npoints, n], dict(steps, error_test_failures, rhs_calls)); raises on an OdeErr / a mass matrix."""
    r = run_to_points(model, p, t_points, model_size=model_size, rtol=rtol, atol=atol, t0=t0, h0=h0, use_tstop=use_tstop)
    return r["y"], {k: r["counters"][k] for k in ("steps", "error_test_failures", "rhs_calls")}


def solve_ensemble(model, p, t_eval, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, group=1, nthreads=8, steps_cap=0, options=None):
    """solve_dense (steps_cap = 0; t_eval the save points) or solve (steps_cap > 0; t_eval = [t_final]) per member (group 1) or per lock-step group of `group`
    members.  atol: [n] / scalar, or [nsys, n] per member.  options: see options_array.  Returns dict(y [nsys, cols, n], t [nsys, cols] (steps only), stats [nsys, 5], status, t_root, root_idx, ncols, failed)."""
    r = run_ensemble(model, p, t_eval, model_size=model_size, rtol=rtol, atol=atol, t0=t0, h0=h0, group=group, nthreads=nthreads, steps_cap=steps_cap, options=options)
    return {k: r[k] for k in ("y", "t", "stats", "status", "t_root", "root_idx", "ncols", "failed")}
