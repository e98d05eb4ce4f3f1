"""The Tsit45 checker with integrated outputs (tests/erk_out_ref) on the CPU: with integrate_out off it is the plain checker bit for bit; with it on and no output
tolerances the states and counters stay the plain run's (the reference's snapshot included) and g follows the closed form under the reference's own bound
(assert_eq_norm(.., 15.0), ode_solver/method.rs:1122); a root stops the solve with g interpolated at the root (method.rs:1167-1185); output tolerances cost steps."""
import numpy as np
import pytest

import erk_out_ref as EO
import erk_ref as E
from helpers import ORACLE_MODEL, weighted_error_norm

RTOL, ATOL = 1e-6, [1e-6]
BOUND = 15.0   # method.rs:1122
# tolerances on g for which the error of g, not of y, decides the step size (confirmed below: the step count exceeds the plain run's)
OUT_RTOL, OUT_ATOL = 1e-10, [1e-12]


def decay_g(p, t):
    """integral from 0 to t of y0 exp(-k s): both states of exponential_decay, identity output"""
    k, y0 = p
    return np.full(2, y0 * (1.0 - np.exp(-k * t)) / k)


@pytest.fixture(params=[False, True], ids=["libm_pow", "portable_pow"])
def det_pow(request):
    E.set_det_pow(request.param)
    EO.set_det_pow(request.param)
    yield request.param
    E.set_det_pow(False)
    EO.set_det_pow(False)


@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("model,size,t_eval,rtol,atol", [("exponential_decay", 0, [0.5, 1.0, 2.5, 6.0], 1e-6, [1e-6, 1e-6]),
                                                         ("robertson_ode", 1, [1e-4, 1e-3, 4e-3], 1e-4, [1e-8, 1e-14, 1e-6])])
def test_off_is_the_plain_checker_bit_for_bit(det_pow, model, size, t_eval, rtol, atol, group):
    """With integrate_out off both sides now run the same code of the one checker, so that half proves less than it did when they were two programs; what the checker
    computed then is held by the recorded hashes of tests/test_erk_checker_parity.py.  The half with integrate_out on still compares two modes"""
    rng = np.random.default_rng(5)
    nb = 7
    if model == "exponential_decay":
        p = np.stack([rng.uniform(0.05, 2.0, nb), rng.uniform(0.5, 5.0, nb)], axis=1)
    else:
        p = np.stack([0.04 * 2 ** rng.uniform(-1, 1, nb), 1e4 * 2 ** rng.uniform(-1, 1, nb), 3e7 * 2 ** rng.uniform(-1, 1, nb)], axis=1)
    for steps_cap in (0, 48):
        te = t_eval if steps_cap == 0 else t_eval[-1:]
        a = E.solve_ensemble(ORACLE_MODEL[model], p, te, model_size=size, rtol=rtol, atol=atol, group=group, steps_cap=steps_cap)
        for on in (False, True):   # on, without output tolerances: the states and every counter are still the plain run's
            b = EO.solve_ensemble(ORACLE_MODEL[model], p, te, model_size=size, rtol=rtol, atol=atol, group=group, steps_cap=steps_cap, integrate_out=on)
            assert a["failed"] == 0 and b["failed"] == 0
            for key in ("y", "t", "stats", "status", "t_root", "root_idx", "ncols"):
                assert np.array_equal(a[key], b[key], equal_nan=True), (key, on, steps_cap)
            assert (b["g"] is None) == (not on)


def test_on_keeps_the_reference_snapshot_and_g_follows_the_closed_form(det_pow):
    """test_tsit45_nalgebra_exponential_decay's counters (explicit_rk.rs:362-384) are untouched by integrate_out without output tolerances: 9 steps, 0 failures,
    56 right-hand sides; g at every point within the bound"""
    p, t = [0.1, 1.0], [float(k) for k in range(10)]
    y0, c0 = E.solve_to_points(ORACLE_MODEL["exponential_decay"], p, t, rtol=RTOL, atol=ATOL)
    y, g, c = EO.solve_to_points(ORACLE_MODEL["exponential_decay"], p, t, rtol=RTOL, atol=ATOL)
    assert np.array_equal(y, y0) and c == c0
    assert (c["steps"], c["error_test_failures"], c["rhs_calls"]) == (9, 0, 56)
    worst = max(weighted_error_norm(g[k], decay_g(p, tk), ATOL, RTOL) for k, tk in enumerate(t))
    print("integrate_out, harness points: largest weighted error of g", worst)
    assert worst <= BOUND
    assert np.array_equal(g[0], np.zeros(2))


@pytest.mark.parametrize("group", [1, 4])
def test_g_at_every_save_point_and_every_accepted_step(det_pow, group):
    rng = np.random.default_rng(11)
    nb = 8
    p = np.stack([rng.uniform(0.05, 2.0, nb), rng.uniform(0.5, 5.0, nb)], axis=1)
    t_eval = [0.0, 0.5, 1.0, 2.5, 6.0, 10.0]
    dense = EO.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, t_eval, rtol=RTOL, atol=ATOL, group=group)
    steps = EO.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, [10.0], rtol=RTOL, atol=ATOL, group=group, steps_cap=64)
    assert dense["failed"] == 0 and steps["failed"] == 0 and (dense["ncols"] == len(t_eval)).all() and steps["ncols"].max() <= 64
    worst = 0.0
    for b in range(nb):
        for k, tk in enumerate(t_eval):
            worst = max(worst, weighted_error_norm(dense["g"][b, k], decay_g(p[b], tk), ATOL, RTOL))
        assert np.array_equal(steps["g"][b, 0], np.zeros(2)) and steps["t"][b, 0] == 0.0   # write_out before the first step: g(t0) = 0
        for c in range(steps["ncols"][b]):
            worst = max(worst, weighted_error_norm(steps["g"][b, c], decay_g(p[b], steps["t"][b, c]), ATOL, RTOL))
        assert np.isnan(steps["g"][b, steps["ncols"][b]:]).all()
    print("integrate_out, save points and accepted steps: largest weighted error of g", worst)
    assert worst <= BOUND


def test_stops_on_the_root_with_g_at_the_root(det_pow):
    """test_dense_solve_integrate_out_stops_on_root (method.rs:1167-1185) with Tsit45"""
    p = np.array([[0.1, 1.0]])
    t_eval = [float(k) for k in range(11)]
    r = EO.solve_ensemble(ORACLE_MODEL["exponential_decay_with_root"], p, t_eval, rtol=RTOL, atol=ATOL)
    t_root = -np.log(0.6) / 0.1
    ncols = int(r["ncols"][0])
    assert r["failed"] == 0 and r["root_idx"][0] == 0 and abs(r["t_root"][0] - t_root) < 1e-3
    assert ncols < len(t_eval) and ncols == int(np.floor(t_root)) + 2     # t = 0..5 drained, then the column at the root
    e = weighted_error_norm(r["g"][0, ncols - 1], np.full(2, 1.0 * 0.4 / 0.1), ATOL, RTOL)
    print("integrate_out at the root: weighted error of g", e)
    assert e <= BOUND
    assert np.isnan(r["g"][0, ncols:]).all() and not np.isnan(r["g"][0, :ncols]).any()
    plain = E.solve_ensemble(ORACLE_MODEL["exponential_decay_with_root"], p, t_eval, rtol=RTOL, atol=ATOL)
    assert np.array_equal(plain["y"], r["y"], equal_nan=True) and plain["t_root"][0] == r["t_root"][0]
    st = EO.solve_ensemble(ORACLE_MODEL["exponential_decay_with_root"], p, [10.0], rtol=RTOL, atol=ATOL, steps_cap=64)   # solve: the last column is the root's
    last = int(st["ncols"][0]) - 1
    assert st["t"][0, last] == r["t_root"][0] and np.array_equal(st["g"][0, last], r["g"][0, ncols - 1])


@pytest.mark.parametrize("out_atol", [OUT_ATOL, [1e-12, 1e-11]], ids=["one_out_atol", "out_atol_per_output"])
def test_output_error_control_bites(det_pow, out_atol):
    p = np.array([[0.1, 1.0]])
    t_eval = [1.0, 5.0, 10.0]
    plain = EO.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, t_eval, rtol=RTOL, atol=ATOL)
    tight = EO.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, t_eval, rtol=RTOL, atol=ATOL, out_rtol=OUT_RTOL, out_atol=out_atol)
    print("steps without / with output tolerances:", plain["stats"][0, 0], tight["stats"][0, 0])
    assert plain["failed"] == 0 and tight["failed"] == 0
    assert tight["stats"][0, 0] > plain["stats"][0, 0]
    for k, tk in enumerate(t_eval):   # the closed form under the OUTPUT tolerances
        assert weighted_error_norm(tight["g"][0, k], decay_g(p[0], tk), out_atol, OUT_RTOL) <= BOUND


def test_a_diffsl_out_function_is_called_at_the_stage_time():
    """out_i { x * y + t } through ExternalFns::out: x = cos(w t), y = -sin(w t), so g(T) = -sin^2(w T) / (2 w) + T^2 / 2 in closed form"""
    import diffsl_models as DM
    code = """
in = [w]
w { 1 }
u_i { x = 1, y = 0, z = 0.5 }
F_i { w * y, -w * x, -0.3 * z }
out_i { x * y + t }
"""
    so, _ = DM.host_model_so(code)
    mid = EO.load_external_model(so)
    assert EO.model_dims(mid)["nout"] == 1
    w = 1.3
    T = 4.0
    r = EO.solve_ensemble(mid, np.array([[w]]), [T], rtol=1e-8, atol=[1e-10] * 3)
    # x = cos(w t), y = -sin(w t): integral of x y + t = -sin^2(w T) / (2 w) + T^2 / 2
    exact = -np.sin(w * T) ** 2 / (2 * w) + T * T / 2
    assert r["failed"] == 0 and abs(r["g"][0, 0, 0] - exact) < 1e-6 * abs(exact)
