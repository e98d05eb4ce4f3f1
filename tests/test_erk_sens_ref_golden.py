"""CPU tier of Tsit45 with forward sensitivities: the checker (tests/erk_sens_ref) against the reference's snapshot counters and the closed form, and the device
library's admission rule and exports (no GPU needed: they answer from the model registry).

The acceptance bound.  test_ode_solver (ode_solver/mod.rs) weighs the error of the states AND of the sensitivities with the problem's STATE tolerances (rtol, atol;
tests/golden/reference_tsit45_sens.json records that reading) and asserts a norm below 20 for the states and below 29 for the sensitivities.  These tests hold the
sensitivities to 20 as well — the tighter of the two."""
import json
import os
import re

import numpy as np
import pytest

import erk_ref as E
import erk_sens_ref as S
from helpers import ORACLE_MODEL, weighted_error_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 20.0


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "reference_tsit45_sens.json")) as f:
        g = json.load(f)
    assert g["acceptance"]["state_bound"] == BOUND and g["acceptance"]["sens_bound"] >= BOUND
    return g


def closed_form(p, t):
    """y = y0 e^{-kt} (both states), dy/dk = -t y0 e^{-kt}, dy/dy0 = e^{-kt}; p [..., 2], t [nt] -> y [..., nt, 2], sens [2, ..., nt, 2]"""
    p, t = np.asarray(p, dtype=float), np.asarray(t, dtype=float)
    k, y0 = p[..., 0:1, None], p[..., 1:2, None]
    e = np.exp(-k * t[:, None]) * np.ones(2)
    return y0 * e, np.stack([-t[:, None] * y0 * e, e])


def worst_norms(y, sens, p, t, rtol, atol):
    """largest weighted error norm over members and save points: states, d/dk, d/dy0; y [nb, nt, 2], sens [2, nb, nt, 2]"""
    ye, se = closed_form(p, t)

    def worst(a, r):
        e = (a - r) / (np.abs(r) * rtol + atol)
        return float(np.sqrt(np.mean(e * e, axis=-1)).max())
    return worst(y, ye), worst(sens[0], se[0]), worst(sens[1], se[1])


@pytest.mark.parametrize("det_pow", [False, True])
def test_checker_reproduces_the_sensitivity_snapshot_and_the_closed_form(gold, det_pow):
    """test_tsit45_nalgebra_exponential_decay_sens (explicit_rk.rs:447-470): 10 steps, 0 error-test failures, 62 right-hand sides, 122 Jacobian products, with the
    harness of test_ode_solver (step past each point, interpolate the state and the sensitivities there)"""
    snap, pb = gold["snapshot"], gold["problem"]
    t = [float(k) for k in range(pb["npoints"])]
    S.set_det_pow(det_pow)
    try:
        y, s, c = S.solve_to_points(ORACLE_MODEL["exponential_decay"], pb["p"], t, rtol=pb["rtol"], atol=pb["atol"], h0=pb["h0"], sens_rtol=pb["sens_rtol"],
                                    sens_atol=pb["sens_atol"])
    finally:
        S.set_det_pow(False)
    assert (c["steps"], c["error_test_failures"], c["rhs_calls"], c["jac_muls"]) == (snap["number_of_steps"], snap["number_of_error_test_failures"], snap["number_of_calls"],
                                                                                     snap["number_of_jac_muls"]) == (10, 0, 62, 122)
    norms = worst_norms(y[None], s[:, None], np.asarray(pb["p"])[None], t, pb["rtol"], pb["atol"][0])
    print("checker, snapshot problem: worst weighted error norms (y, dy/dk, dy/dy0)", norms)
    assert max(norms) < BOUND
    for k, tk in enumerate(t):  # the project's own norm helper says the same
        assert weighted_error_norm(s[0, k], np.full(2, -tk * np.exp(-0.1 * tk)), pb["atol"], pb["rtol"]) < BOUND


@pytest.mark.parametrize("det_pow", [False, True])
def test_without_sensitivity_error_control_the_steps_are_the_plain_solvers(gold, det_pow):
    """turn_off_sensitivities_error_control: the sensitivities ride along, the states and the step sequence are those of problem.tsit45() — 9 steps (the plain checker's
    snapshot), the same right-hand sides, bitwise the same states"""
    pb = gold["problem"]
    t = [float(k) for k in range(pb["npoints"])]
    S.set_det_pow(det_pow)
    E.set_det_pow(det_pow)
    try:
        y, s, c = S.solve_to_points(ORACLE_MODEL["exponential_decay"], pb["p"], t, rtol=pb["rtol"], atol=pb["atol"], h0=pb["h0"], sens_atol=None)
        yp, cp = E.solve_to_points(ORACLE_MODEL["exponential_decay"], pb["p"], t, rtol=pb["rtol"], atol=pb["atol"], h0=pb["h0"])
    finally:
        S.set_det_pow(False)
        E.set_det_pow(False)
    assert c["steps"] == cp["steps"] == 9 and c["error_test_failures"] == cp["error_test_failures"] and c["rhs_calls"] == cp["rhs_calls"]
    assert c["jac_muls"] == 2 + 2 * 6 * c["steps"]  # two at t0, then one per stage 1..6 and parameter
    assert np.array_equal(y, yp)
    assert max(worst_norms(y[None], s[:, None], np.asarray(pb["p"])[None], t, pb["rtol"], pb["atol"][0])) < BOUND


SWEEP_T = [0.0, 0.5, 1.0, 2.0, 4.0]


def sweep_params(nb, seed=11):
    """the ranges of the GPU tests (tests/test_gpu_erk_sens.py): k in [0.05, 2], y0 in [0.5, 5]"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.05, 2.0, nb), rng.uniform(0.5, 5.0, nb)], axis=1)


@pytest.mark.parametrize("group", [1, 64])
def test_checker_stays_under_the_bound_on_the_gpu_accuracy_ranges(group):
    """512 sampled members of the 4096-member GPU accuracy run, per member and in lock-step groups of 64: the checker alone is under the bound, so a GPU failure means the
    kernel"""
    p = sweep_params(512)
    r = S.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, SWEEP_T, rtol=1e-6, atol=[1e-6], sens_rtol=1e-6, sens_atol=[1e-6], group=group)
    assert r["failed"] == 0 and not r["status"].any()
    norms = worst_norms(r["y"], r["sens"], p, SWEEP_T, 1e-6, 1e-6)
    print("checker, group", group, ": worst weighted error norms (y, dy/dk, dy/dy0)", norms)
    assert max(norms) < BOUND
    if group == 64:  # one step sequence per group
        assert all(len(np.unique(r["stats"][g:g + 64, 0])) == 1 for g in range(0, 512, 64))
    assert (r["jac_muls"] == 2 + 12 * (r["stats"][:, 0] + r["stats"][:, 3])).all()


def test_sensitivities_of_a_model_with_root_functions_are_refused():
    """the checker does not restate sensitivities across a root, and the device refuses the combination: both entries say so rather than integrating past the root"""
    root, p = ORACLE_MODEL["exponential_decay_with_root"], np.array([[0.5, 1.0], [1.0, 2.0]])   # both members cross 0.6 before t = 4
    with pytest.raises(RuntimeError, match="sensitivities with root functions are not restated"):
        S.solve_ensemble(root, p, SWEEP_T)
    with pytest.raises(RuntimeError, match="sensitivities with root functions are not restated"):
        S.solve_to_points(root, p[0], SWEEP_T)
    assert (E.solve_ensemble(root, p, SWEEP_T)["root_idx"] == 0).all()   # the plain mode takes the model and stops at its root


def test_device_library_admission_rule_and_exports():
    """dsh_erk_model_has_sens: N (14 + 12 NP) <= 112 doubles per lane, parameter derivatives, no root functions, on top of dsh_model_has_resident(3, ..)"""
    from diffsol_amd import MODELS, _ffi
    dev = _ffi.load_device_lib()
    assert dev.dsh_erk_solve_resident_sens
    assert dev.dsh_erk_model_has_sens(MODELS["exponential_decay"], 0) == 1           # 2 states, 2 parameters: 76
    assert dev.dsh_erk_model_has_sens(MODELS["robertson_ode"], 1) == 0               # 3 states, 3 parameters: 150
    assert dev.dsh_erk_model_has_sens(MODELS["exponential_decay_with_root"], 0) == 0  # a root function
    assert dev.dsh_erk_model_has_sens(MODELS["robertson"], 0) == 0                   # mass matrix
    assert dev.dsh_erk_model_has_sens(MODELS["heat1d"], 20) == 0                     # run-time sized
    assert "dsh_erk_model_has_sens" in _ffi.DEVICE_ABI and "dsh_erk_solve_resident_sens" in _ffi.DEVICE_ABI
    hdr = open(os.path.join(ROOT, "include", "diffsol_hip.h")).read()
    assert re.search(r"\bint dsh_erk_model_has_sens\(int model, int64_t size\);", hdr) and re.search(r"\bint dsh_erk_solve_resident_sens\(dsh_ctx\* ctx, int method,", hdr)


def test_the_admission_bound_is_one_function_with_the_documented_shapes():
    """erk_sens_admitted (csrc/dsh_erk_kernel.hpp) read from the source: admits (2, 2), (2, 3), (4, 1), (1, 8); excludes (3, 3), (3, 2), (2, 4), (4, 2), (1, 9)"""
    src = open(os.path.join(ROOT, "diffsol_amd", "csrc", "dsh_erk_kernel.hpp")).read()
    cap = int(re.search(r"constexpr int kErkMaxLaneDoubles = (\d+);", src).group(1))
    assert re.search(r"erk_sens_admitted\(int64_t n, int64_t np\) \{ return n >= 1 && np >= 1 && n \* \(14 \+ 12 \* np\) <= kErkMaxLaneDoubles; \}", src)
    assert cap <= 112  # the plain kernel's largest instantiation (N = 8) is what was shown to compile without scratch: never above it
    admitted = lambda n, q: n * (14 + 12 * q) <= cap
    if cap == 112:
        assert all(admitted(*s) for s in ((2, 2), (2, 3), (4, 1), (1, 8)))
    assert not any(admitted(*s) for s in ((3, 3), (3, 2), (2, 4), (4, 2), (1, 9)))


def test_python_surface():
    import diffsol_amd
    assert callable(diffsol_amd.OdeBuilder().tsit45_sens)
