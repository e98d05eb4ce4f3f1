"""Area under the concentration curve for a sweep of clearances, one launch — integrate_out on the device-resident Tsit45.

    python examples/auc_sweep/run.py [nmembers]

Model: one compartment after an intravenous bolus, c' = -(cl / v) c from c(0) = dose / v, written in DiffSL with out_i { c }.  With integrate_out the solver state
carries g(t) = integral of c from 0 to t next to the state, so solve_dense returns the AUC up to every save point instead of c.  Every member has its own clearance
(log-uniform over two decades); the closed form is AUC(t) = dose / cl * (1 - exp(-cl t / v)).  The integral is not a state of the model: it stays out of the state
error test and costs 12 doubles per lane instead of 14 (README.md).  out_rtol / out_atol put the integral into the error test of its own accord."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from diffsol_amd import OdeBuilder, diffsl  # noqa: E402

ONE_COMPARTMENT = "in_i { cl = 1.0, v = 10.0, dose = 100.0 }\nu_i { c = dose / v }\nF_i { -(cl / v) * c }\nout_i { c }\n"

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
rng = np.random.default_rng(1)
cl = 10.0 ** rng.uniform(-1.0, 1.0, nb)                         # clearance, L/h
v, dose = 10.0, 100.0
p = np.stack([cl, np.full(nb, v), np.full(nb, dose)], axis=1)
t_eval = np.array([0.0, 1.0, 2.0, 4.0, 8.0, 12.0, 24.0, 48.0])  # h
rtol, atol = 1e-6, 1e-6

model = diffsl.DiffslModel(ONE_COMPARTMENT)                     # DiffSL -> HIP source -> hiprtc (cached on disk)
solver = OdeBuilder().model(model).p(p).nbatch(nb).rtol(rtol).atol([atol]).integrate_out(True).out_rtol(rtol).out_atol([atol]).tsit45()
auc, reason = solver.solve_dense(t_eval)                        # [nt, nbatch, nout = 1]
_, totals = solver.last_solve_info()

exact = dose / cl[None, :] * (1.0 - np.exp(-cl[None, :] * t_eval[:, None] / v))
err = np.abs(auc[:, :, 0] - exact) / (np.abs(exact) * rtol + atol)
print(f"{nb} clearances, {len(t_eval)} save points, {totals['number_of_steps']} steps in all, {totals['failed_members']} failures")
print(f"AUC(0-48 h): {auc[-1, :, 0].min():.3f} .. {auc[-1, :, 0].max():.3f} mg h / L; largest weighted error against the closed form {err.max():.3f}")
assert totals["failed_members"] == 0 and err.max() < 15.0, err.max()
