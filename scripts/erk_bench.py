"""Tsit45 against the existing device-resident routes on a NON-STIFF sweep (MI355X): 100 000 logistic members (DiffSL text, n = 1), same rtol / atol / t_eval,
exact arithmetic on every side.  Wall time per solve from HIP events around the launch (Solver.set_kernel_timing), median of --reps after --warmup, and
steps / right-hand-side calls per member from the kernels' counters.

    python scripts/erk_bench.py [--nb 100000] [--reps 20] [--warmup 3] [--group 64]

Prints one JSON line per method."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("DSH_RESIDENT_ARITH", "exact")

import diffsol_amd as H  # noqa: E402
from diffsol_amd import diffsl  # noqa: E402

LOGISTIC = """
in = [r, k]
r { 1 } k { 1 }
u_i { y = 0.1 }
F_i { r * y * (1 - y / k) }
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--group", type=int, default=64, choices=[1, 64])
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    p = np.stack([rng.uniform(0.5, 2.0, a.nb), rng.uniform(0.5, 3.0, a.nb)], axis=1)
    t_eval = [0.5, 1.0, 2.0, 4.0, 8.0]
    model = diffsl.DiffslModel(LOGISTIC)
    exact = p[None, :, 1] / (1.0 + (p[None, :, 1] / 0.1 - 1.0) * np.exp(-p[None, :, 0] * np.asarray(t_eval)[:, None]))
    for name, method in (("tsit45", H.METHOD_TSIT45), ("bdf", H.METHOD_BDF), ("esdirk34", H.METHOD_ESDIRK34), ("tr_bdf2", H.METHOD_TR_BDF2)):
        s = H.Solver(model, p, nbatch=a.nb, method=method, rtol=1e-6, atol=[1e-8])
        s.set_kernel_timing(True)
        ms = []
        for k in range(a.warmup + a.reps):
            n0, t0 = s.kernel_timing()
            y, tot = s.solve_dense_adaptive(t_eval, group=a.group, deterministic_pow=True)
            n1, t1 = s.kernel_timing()
            if k >= a.warmup:
                ms.append(t1 - t0)
        err = float(np.max(np.abs(y[:, :, 0] - exact) / (np.abs(exact) * 1e-6 + 1e-8)))
        steps = tot["number_of_steps"] / a.nb
        fails = tot["number_of_error_test_failures"] / a.nb
        rec = dict(method=name, nb=a.nb, group=a.group, reps=a.reps, kernel_ms_median=statistics.median(ms), kernel_ms_min=min(ms), kernel_ms_max=max(ms),
                   steps_per_member=steps, error_test_failures_per_member=fails, newton_iterations_per_member=tot["number_of_nonlinear_solver_iterations"] / a.nb,
                   failed_members=tot["failed_members"], max_weighted_error=err)
        if name == "tsit45":
            rec["rhs_calls_per_member"] = 2 + 6 * (steps + fails)  # init + initial step size + 6 stages per attempt (first same as last)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
