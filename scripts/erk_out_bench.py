"""What integrate_out costs on the device-resident Tsit45 (profiles/erk_tsit45_out.md).

    python scripts/erk_out_bench.py [--reps 7] [--out results.json]

100 000 exponential-decay members (x' = -k x, y' = -k y from y0; DiffSL text), 8 save points, tolerances 1e-6, four solvers alive in this process and called alternately
(the order rotates every round) after two warm-up rounds:
  plain       Solver.solve_dense_adaptive of the model: the states
  integrate   the same model with out_i { x, y } and integrate_out=True: g = integral of the outputs, outside the error test (no output tolerances)
  integrate_tol  the same with out_rtol = out_atol = 1e-6: g inside the error test
  augmented   the work-around: the integrals appended as two more states (4 states), so they sit in the state error test
Host clock around the call with the results left on the device (want_host=False: the call returns after the stream is synchronised); per member (group 1) and in
wavefront groups (group 64).  The largest weighted error of the integral against y0 (1 - exp(-k t)) / k is taken from one more call that copies the results back."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diffsol_amd as H  # noqa: E402
from diffsol_amd import diffsl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--nb", type=int, default=100_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()

DECAY = "in_i { k = 0.1, y0 = 1.0 }\nu_i { x = y0, y = y0 }\nF_i { -k * u_i }\nout_i { x, y }\n"
AUGMENTED = "in_i { k = 0.1, y0 = 1.0 }\nu_i { x = y0, y = y0, gx = 0, gy = 0 }\nF_i { -k * x, -k * y, x, y }\n"
TOL = 1e-6
nb = args.nb
rng = np.random.default_rng(7)
p = np.stack([rng.uniform(0.05, 2.0, nb), rng.uniform(0.5, 5.0, nb)], axis=1)
t_eval = np.linspace(0.0, 10.0, 8)
exact = (p[None, :, 1] * (1.0 - np.exp(-p[None, :, 0] * t_eval[:, None])) / p[None, :, 0])[:, :, None]   # [nt, nb, 1]: both integrals


def worst(g):
    return float((np.abs(g - exact) / (np.abs(exact) * TOL + TOL)).max())


decay, augmented = diffsl.DiffslModel(DECAY), diffsl.DiffslModel(AUGMENTED)
kw = dict(nbatch=nb, method=H.METHOD_TSIT45, rtol=TOL)
solvers = {
    "plain": H.Solver(decay, p, atol=[TOL] * 2, **kw),
    "integrate": H.Solver(decay, p, atol=[TOL] * 2, integrate_out=True, **kw),
    "integrate_tol": H.Solver(decay, p, atol=[TOL] * 2, integrate_out=True, out_rtol=TOL, out_atol=[TOL], **kw),
    "augmented": H.Solver(augmented, p, atol=[TOL] * 4, **kw),
}
res = {}
for group in (1, 64):
    names = list(solvers)
    times = {k: [] for k in names}
    steps = {}
    for rep in range(args.reps + 2):
        order = names[rep % len(names):] + names[:rep % len(names)]
        for k in order:
            t0 = time.perf_counter()
            _, tot = solvers[k].solve_dense_adaptive(t_eval, want_host=False, group=group)
            dt = time.perf_counter() - t0
            if rep >= 2:
                times[k].append(dt)
            steps[k] = (tot["number_of_steps"], tot["number_of_error_test_failures"], tot["failed_members"])
    row = {}
    for k in names:
        v = np.asarray(times[k]) * 1e3
        row[k] = dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), steps=steps[k][0], error_test_failures=steps[k][1], failed=steps[k][2])
    for k in ("integrate", "integrate_tol"):
        row[k]["worst_weighted_error_of_g"] = worst(solvers[k].solve_dense_adaptive(t_eval, group=group)[0])
    row["augmented"]["worst_weighted_error_of_g"] = worst(solvers["augmented"].solve_dense_adaptive(t_eval, group=group)[0][:, :, 2:])
    res[f"group{group}"] = row
    print(f"group {group}", json.dumps(row), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(dict(nb=nb, nt=len(t_eval), tol=TOL, reps=args.reps, **res), f, indent=1)
