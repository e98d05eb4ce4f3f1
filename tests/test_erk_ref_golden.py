"""CPU tier of the Tsit45 feature: the checker (tests/erk_ref) against the reference's snapshot counters and closed forms, the tableau constants of the kernel and of
the checker against the golden file, the order conditions, and the Python surface.  The refusals that dshs_create makes (mass matrix, host-driven solve) need a HIP
device to build the solver's context, so they are tested in tests/test_gpu_erk.py."""
import json
import os
import re

import numpy as np
import pytest

import erk_ref as E
from helpers import ORACLE_MODEL, weighted_error_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "reference_tsit45.json")) as f:
        return json.load(f)


def seqsum(v):
    s = 0.0
    for x in v:
        s += x
    return s


@pytest.mark.parametrize("det_pow", [False, True])
def test_checker_reproduces_the_exponential_decay_snapshot_and_closed_form(gold, det_pow):
    """test_tsit45_nalgebra_exponential_decay (explicit_rk.rs:362-384): 9 steps, 0 error-test failures, 56 right-hand sides; test_ode_solver's bound
    (ode_solver/mod.rs:164-167): weighted error norm below 20 at every point."""
    snap = gold["snapshots"]["exponential_decay"]
    E.set_det_pow(det_pow)
    try:
        p, t = [0.1, 1.0], [float(k) for k in range(10)]
        y, c = E.solve_to_points(ORACLE_MODEL["exponential_decay"], p, t, rtol=1e-6, atol=[1e-6], h0=1.0)
    finally:
        E.set_det_pow(False)
    assert c["steps"] == snap["number_of_steps"] and c["error_test_failures"] == snap["number_of_error_test_failures"] and c["rhs_calls"] == snap["number_of_calls"]
    for k, tk in enumerate(t):
        assert weighted_error_norm(y[k], np.full(2, p[1] * np.exp(-p[0] * tk)), [1e-6], 1e-6) < 20.0


def test_checker_tstop_harness_hits_every_point(gold):
    """test_tstop_tsit45 (explicit_rk.rs:538-543): set_stop_time at every point, state.y there within the same bound"""
    p, t = [0.1, 1.0], [float(k) for k in range(10)]
    y, _ = E.solve_to_points(ORACLE_MODEL["exponential_decay"], p, t, rtol=1e-6, atol=[1e-6], h0=1.0, use_tstop=True)
    for k, tk in enumerate(t):
        assert weighted_error_norm(y[k], np.full(2, p[1] * np.exp(-p[0] * tk)), [1e-6], 1e-6) < 20.0


def test_checker_refuses_a_mass_matrix():
    """explicit_rk_rejects_mass_matrices (runge_kutta.rs:236-239)"""
    with pytest.raises(RuntimeError, match="MassMatrixNotSupported"):
        E.solve_to_points(ORACLE_MODEL["robertson"], [0.04, 1e4, 3e7], [1.0], rtol=1e-4, atol=[1e-6])


def kernel_tableau():
    src = open(os.path.join(ROOT, "diffsol_amd", "csrc", "dsh_erk_kernel.hpp")).read()
    blk = src[src.index("TSIT45-TABLEAU-BEGIN"):src.index("TSIT45-TABLEAU-END")]
    blk = re.sub(r"//[^\n]*", "", blk)
    arr = {}
    for name, body in re.findall(r"constexpr double (\w+)(?:\[\d+\])+ = \{(.*?)\};", blk, re.S):
        arr[name] = [float(x) for x in re.findall(r"-?\d+\.\d*(?:[eE][-+]?\d+)?", body)]
    c, b, d, low, beta = arr["kTsitC"], arr["kTsitB"], arr["kTsitD"], arr["kTsitALower"], arr["kTsitBeta"]
    a = [[0.0] * 7 for _ in range(7)]
    k = 0
    for i in range(2, 6):
        for j in range(1, i):
            a[i][j] = low[k]
            k += 1
    for i in range(1, 6):  # erk_a(i, 0)
        a[i][0] = c[i] - seqsum(a[i][1:i])
    a[6][:6] = b[:6]
    return dict(a=a, b=b, c=c, d=d, beta=[beta[q * 7:(q + 1) * 7] for q in range(4)])


@pytest.mark.parametrize("which", ["kernel", "checker"])
def test_tableau_constants_equal_the_reference(gold, which):
    tab = kernel_tableau() if which == "kernel" else E.tableau()
    for key in ("a", "b", "c", "d", "beta"):
        assert tab[key] == gold["tableau"][key], key
    assert gold["tableau"]["order"] == 4 and (which == "kernel" or tab["order"] == 4)


def test_order_conditions_hold_to_rounding(gold):
    """sum b = 1, sum_j a_ij = c_i, sum d = 0 (d = b - bhat, both weight sets sum to one) to the rounding of a 7-term sum of doubles of magnitude <= 1: 4e-16 — or,
    where the reference's own constants miss that (row sums: entries up to 13 in magnitude), the residual measured on them and recorded in the golden file."""
    t, r = gold["tableau"], gold["order_condition_residuals"]
    bound = lambda key: max(4e-16, r[key])
    assert abs(seqsum(t["b"]) - 1.0) <= bound("sum_b_minus_1")
    assert max(abs(seqsum(t["a"][i]) - t["c"][i]) for i in range(7)) <= bound("max_row_sum_a_minus_c")
    assert abs(seqsum(t["d"])) <= bound("abs_sum_d")
    assert all(t["a"][i][j] == 0.0 for i in range(7) for j in range(i, 7)) and t["a"][6][:6] == t["b"][:6] and t["c"][0] == 0.0 and t["c"][6] == 1.0  # check_explicit_rk


def test_checker_stays_under_the_acceptance_bound_on_the_large_ensemble_ranges():
    """the parameter ranges of tests/test_gpu_erk.py's 100 000-member run, sampled: the checker alone is under the reference's bound, so a GPU failure means the kernel"""
    rng = np.random.default_rng(7)
    nb = 512
    p = np.stack([rng.uniform(0.05, 2.0, nb), rng.uniform(0.5, 5.0, nb)], axis=1)
    t = [0.5, 1.0, 2.0, 4.0]
    r = E.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, t, rtol=1e-6, atol=[1e-6], h0=1.0)
    assert r["failed"] == 0
    exact = p[:, None, 1:2] * np.exp(-p[:, None, 0:1] * np.asarray(t)[None, :, None]) * np.ones((1, 1, 2))
    worst = max(weighted_error_norm(r["y"][b, k], exact[b, k], [1e-6], 1e-6) for b in range(nb) for k in range(len(t)))
    print("checker, worst weighted error norm:", worst)
    assert worst < 20.0


def test_python_surface_exports_tsit45():
    import diffsol_amd
    from diffsol_amd import _ffi, solver
    assert diffsol_amd.METHOD_TSIT45 == 3 and solver.METHOD_TSIT45 == 3 and "METHOD_TSIT45" in diffsol_amd.__all__
    assert callable(diffsol_amd.OdeBuilder().tsit45)
    assert "dsh_erk_solve_resident" in _ffi.DEVICE_ABI and "dsh_erk_solve_resident_steps" in _ffi.DEVICE_ABI
    hdr = open(os.path.join(ROOT, "include", "diffsol_hip_solver.h")).read()
    assert re.search(r"#define DSHS_METHOD_TSIT45 3\b", hdr)


def test_device_library_exports_the_tsit45_entries_and_admits_the_static_models():
    """no GPU needed: the symbols resolve and dsh_model_has_resident(3, ..) answers from the model registry"""
    from diffsol_amd import MODELS, _ffi
    dev = _ffi.load_device_lib()
    assert dev.dsh_erk_solve_resident and dev.dsh_erk_solve_resident_steps
    assert dev.dsh_model_has_resident(3, MODELS["exponential_decay"], 0) == 1
    assert dev.dsh_model_has_resident(3, MODELS["exponential_decay_with_root"], 0) == 1
    assert dev.dsh_model_has_resident(3, MODELS["robertson_ode"], 1) == 1
    assert dev.dsh_model_has_resident(3, MODELS["robertson"], 0) == 0        # mass matrix
    assert dev.dsh_model_has_resident(3, MODELS["heat1d"], 20) == 0          # run-time sized, n > 8
    assert dev.dsh_model_has_resident(3, MODELS["robertson_ode"], 4) == 0    # 12 states
