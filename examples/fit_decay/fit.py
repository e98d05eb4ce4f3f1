"""A multi-start least-squares fit, one Gauss-Newton iteration per device call — the objective of the reference's gradient example
(examples/intro-logistic-closures/src/solve_adjoint_sens_sum_squares.rs: g = 2 (soln - data)) with forward sensitivities, for a whole ensemble of starts at once.

    python examples/fit_decay/fit.py [nstarts] [--method {bdf,tsit45}]

Model: x' = -k x, y' = -k y from x(0) = y(0) = y0, observed through out_i { x + y, k x } at t = 0 ... 10.  The data are the closed-form outputs at the true
(k, y0) = (0.1, 1.0), the defaults of the model.  Every member starts within +-20 % of the truth and iterates p <- p - gn^-1 grad: Solver.solve_dense_sens_fit integrates the states and their
sensitivities, reduces them against the data on the device and returns per member only the loss, its gradient and the Gauss-Newton matrix (7 doubles here).
--method tsit45 integrates with the explicit Tsit45 and its forward sensitivities instead of the BDF (the model is not stiff: no Jacobian, no LU, no Newton)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from diffsol_amd import METHOD_BDF, METHOD_TSIT45, Solver, diffsl  # noqa: E402

DECAY = "in_i { k = 0.1, y0 = 1.0 }\nu_i { x = y0, y = y0 }\nF_i { -k * u_i }\nout_i { x + y, k * x }\n"

ap = argparse.ArgumentParser()
ap.add_argument("nstarts", nargs="?", type=int, default=4096)
ap.add_argument("--method", choices=["bdf", "tsit45"], default="bdf")
args = ap.parse_args()
nb, method = args.nstarts, {"bdf": METHOD_BDF, "tsit45": METHOD_TSIT45}[args.method]
true = np.array([0.1, 1.0])
t_eval = np.linspace(0.0, 10.0, 11)
e = np.exp(-true[0] * t_eval)
data = np.stack([2 * true[1] * e, true[0] * true[1] * e], axis=1)        # [nt, nout]: shared by all members
model = diffsl.DiffslModel(DECAY)                                       # DiffSL -> HIP source -> hiprtc (cached on disk)
p = true * np.random.default_rng(0).uniform(0.8, 1.2, (nb, 2))          # the starts
print(f"{nb} starts; worst relative parameter error {np.abs(p / true - 1).max():.2e}")
for it in range(6):
    solver = Solver(model, p, nbatch=nb, method=method, sens=True, sens_rtol=1e-8, sens_atol=[1e-8], rtol=1e-8, atol=[1e-8, 1e-8])
    loss, grad, totals, gn = solver.solve_dense_sens_fit(t_eval, data, gauss_newton=True)
    p = p - np.linalg.solve(gn, grad[:, :, None])[:, :, 0]              # [nb, 2, 2] \ [nb, 2]
    print(f"iteration {it}: largest loss {loss.max():.3e}, {totals['number_of_steps']} steps, {totals['failed_members']} failures; "
          f"worst relative parameter error {np.abs(p / true - 1).max():.2e}")
