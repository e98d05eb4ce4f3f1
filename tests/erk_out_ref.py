"""The Tsit45 checker with integrated outputs: the INTEGRATE_OUT mode of tests/erk_ref.py (one library, one model registry, one pow switch).  TEST INFRASTRUCTURE
ONLY.  out_atol None: the outputs stay out of the error test; a scalar / [1]: one value for every output; [nout]: one each.  Without integrate_out the solve is the
plain one and g is None."""
import erk_ref
from erk_ref import build, load_external_model, model_dims, set_det_pow  # noqa: F401  (this module's public names)


def _mode(integrate_out, out_rtol, out_atol):
    return dict(kind=erk_ref.INTEGRATE_OUT, aug_rtol=out_rtol, aug_atol=out_atol) if integrate_out else {}


def solve_to_points(model, p, t_points, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, integrate_out=True, out_rtol=1e-6, out_atol=None):
    """the reference's test harness on one IVP.  Returns (y [npoints, n], g [npoints, nout] or None, dict(steps, error_test_failures, rhs_calls))."""
    r = erk_ref.run_to_points(model, p, t_points, model_size=model_size, rtol=rtol, atol=atol, t0=t0, h0=h0, **_mode(integrate_out, out_rtol, out_atol))
    return r["y"], r["g"], {k: r["counters"][k] for k in ("steps", "error_test_failures", "rhs_calls")}


def solve_ensemble(model, p, t_eval, *, model_size=0, rtol=1e-6, atol=(1e-6,), t0=0.0, h0=1.0, group=1, nthreads=8, steps_cap=0, integrate_out=True, out_rtol=1e-6,
                   out_atol=None, options=None):
    """solve_dense (steps_cap = 0; t_eval the save points) or solve (steps_cap > 0; t_eval = [t_final]) per member (group 1) or per lock-step group of `group`
    members, with the outputs integrated.  atol: [n] / scalar, or [nsys, n] per member.  options: see erk_ref.options_array.  Returns dict(y [nsys, cols, n] (the states), g [nsys, cols, nout] (None without
    integrate_out), t [nsys, cols] (steps only), stats [nsys, 5], status, t_root, root_idx, ncols, rhs_calls, failed)."""
    r = erk_ref.run_ensemble(model, p, t_eval, model_size=model_size, rtol=rtol, atol=atol, t0=t0, h0=h0, group=group, nthreads=nthreads, steps_cap=steps_cap,
                             options=options, **_mode(integrate_out, out_rtol, out_atol))
    return {k: r[k] for k in ("y", "g", "t", "stats", "status", "t_root", "root_idx", "ncols", "rhs_calls", "failed")}
