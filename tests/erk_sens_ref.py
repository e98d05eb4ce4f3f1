"""The Tsit45 checker with forward sensitivities: the SENS mode of tests/erk_ref.py (one library, one model registry, one pow switch).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import erk_ref
from erk_ref import build, load_external_model, model_dims, set_det_pow  # noqa: F401  (this module's public names)


def solve_to_points(model, p, t_points, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, sens_rtol=1e-6, sens_atol=(1e-6,)):
    """the reference's test harness on one IVP.  sens_atol None: the sensitivities stay out of the error control; a scalar / [1]: one value for every state; [n]: per
    state.  Returns (y [npoints, n], sens [nparams, npoints, n], dict(steps, error_test_failures, rhs_calls, jac_muls))."""
    r = erk_ref.run_to_points(model, p, t_points, model_size=model_size, rtol=rtol, atol=atol, t0=t0, h0=h0, kind=erk_ref.SENS, aug_rtol=sens_rtol, aug_atol=sens_atol)
    return r["y"], r["s"].transpose(1, 0, 2), r["counters"]


def solve_ensemble(model, p, t_eval, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, sens_rtol=1e-6, sens_atol=(1e-6,), group=1, nthreads=8,
                   options=None):
    """solve_dense_sensitivities per member (group 1) or per lock-step group of `group` members.  atol: [n] / scalar, or [nsys, n] per member.  options: see
    erk_ref.options_array.
    Returns dict(y [nsys, nt, n], sens [nparams, nsys, nt, n], stats [nsys, 5], status [nsys], rhs_calls [nsys], jac_muls [nsys], ncols [nsys], failed)."""
    r = erk_ref.run_ensemble(model, p, t_eval, model_size=model_size, rtol=rtol, atol=atol, t0=t0, h0=h0, group=group, nthreads=nthreads, options=options,
                             kind=erk_ref.SENS, aug_rtol=sens_rtol, aug_atol=sens_atol)
    return dict(y=r["y"], sens=np.ascontiguousarray(r["s"].transpose(2, 0, 1, 3)), **{k: r[k] for k in ("stats", "status", "rhs_calls", "jac_muls", "ncols", "failed")})
