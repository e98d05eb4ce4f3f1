"""The options of the Tsit45 checkers (tests/erk_ref, erk_sens_ref, erk_out_ref: `options=dict(...)`) pinned to the reference's text, on the CPU: the exits behind a
rejected step, the two stop-time exits, and the step cap of the device ABI.  What the GPU tier (tests/test_gpu_erk_exits.py) compares the kernels with is what these
tests hold to the lines cited beside each (paths relative to the reference's crates/diffsol/src/ode_solver).

The rejections come from dy/dt = a y^2 (DYDT_Y2 of tests/test_gpu_erk.py) integrated towards its blow-up: y = 1 / (1/y0 - a t), so with a = 1 the component that
starts at 2 leaves every bound at t = 0.5."""
import numpy as np
import pytest

import erk_out_ref as EO
import erk_ref as E
import erk_sens_ref as S
from helpers import ORACLE_MODEL

DYDT_Y2 = """
in = [a]
a { 1 }
u_i { x = 1, z = 2, w = 0.5 }
F_i { a * x * x, a * z * z, a * w * w }
"""
T_BLOW = [0.2, 0.4, 0.45, 0.6]      # a = 1: the last save point lies behind the blow-up at t = 0.5
TOL = dict(rtol=1e-6, atol=[1e-8] * 3)
P1 = np.array([[1.0]])
DECAY = ORACLE_MODEL["exponential_decay"]
P_DECAY = np.array([[0.1, 1.0], [1.0, 2.0], [2.0, 0.5]])
T_DECAY = [0.5, 1.0, 2.5, 6.0]


@pytest.fixture(autouse=True)
def det_pow():
    for m in (E, S, EO):
        m.set_det_pow(True)
    yield
    for m in (E, S, EO):
        m.set_det_pow(False)


_twin = []


def blow_up():
    """the checker's id of DYDT_Y2's host twin (one registry behind the three modules)"""
    if not _twin:
        import diffsl_models as DM
        so, _ = DM.host_model_so(DYDT_Y2)
        _twin.append(E.load_external_model(so))
    return _twin[0]


def columns(r):
    """the array a checker's columns are compared in: the integrated outputs of erk_out_ref, the states otherwise"""
    return r["g"] if r.get("g") is not None else r["y"]


def ncols_of(r):
    """columns written before the exit: the checker's count, or (erk_sens_ref returns none) the columns that are not NaN"""
    return r["ncols"] if "ncols" in r else np.isfinite(r["y"][:, :, 0]).sum(axis=1)


@pytest.mark.parametrize("mod", [E, S, EO], ids=["plain", "sens", "out"])
def test_no_options_and_the_default_options_are_the_same_run(mod):
    """options=None is the call of before; the defaults spelled out (and max_steps <= 0, which means 10 000 000) change no bit"""
    a = mod.solve_ensemble(DECAY, P_DECAY, T_DECAY)
    for o in (dict(), dict(max_steps=0), dict(max_steps=-3, max_error_test_failures=40, min_timestep=1e-13, pi_control_integral=0.5, pi_control_proportional=0.0)):
        b = mod.solve_ensemble(DECAY, P_DECAY, T_DECAY, options=o)
        assert b["failed"] == 0 and np.array_equal(a["stats"], b["stats"]) and np.array_equal(columns(a), columns(b))
    with pytest.raises(KeyError):
        mod.solve_ensemble(DECAY, P_DECAY, T_DECAY, options=dict(max_step=3))


def test_the_blow_up_reaches_the_rejection_branch_with_default_options():
    """explicit_rk.rs:227-239: a rejected attempt multiplies h by the factor, forgets the previous error norm and counts a failure.  Behind the blow-up every attempt
    is rejected until one of error_test_fail's two exits (runge_kutta.rs:843-867) is taken; the columns before it are written, the others NaN"""
    r = E.solve_ensemble(blow_up(), P1, T_BLOW, options=dict(max_steps=100000), **TOL)
    assert r["status"][0] in (1, 2) and r["failed"] == 1 and r["stats"][0, 3] > 0
    assert r["ncols"][0] == 3 and np.isfinite(r["y"][0, :3]).all() and np.isnan(r["y"][0, 3:]).all()
    exact = 1.0 / (1.0 / np.array([1.0, 2.0, 0.5])[None, :] - np.array(T_BLOW[:3])[:, None])
    assert np.abs(r["y"][0, :3] / exact - 1.0).max() < 1e-3


@pytest.mark.parametrize("mod", [E, S, EO], ids=["plain", "sens", "out"])
def test_max_error_test_failures_1_fails_at_the_first_rejection(mod):
    """runge_kutta.rs:852-859: `nattempts >= max_error_test_fails` with nattempts already counted (explicit_rk.rs:228), so a limit of 1 fails at the first rejected
    attempt, with exactly one counted failure (:850).  Up to there the run is the unrestricted one: its columns bit for bit, NaN behind them"""
    mid = blow_up()
    free = mod.solve_ensemble(mid, P1, T_BLOW, options=dict(max_steps=100000), **TOL)
    one = mod.solve_ensemble(mid, P1, T_BLOW, options=dict(max_steps=100000, max_error_test_failures=1), **TOL)
    assert free["stats"][0, 3] > 1
    assert one["status"][0] == 2 and one["failed"] == 1 and one["stats"][0, 3] == 1 and 0 < one["stats"][0, 0] <= free["stats"][0, 0]
    k = int(ncols_of(one)[0])
    assert 0 <= k <= int(ncols_of(free)[0])
    assert np.array_equal(columns(one)[0, :k], columns(free)[0, :k]) and np.isnan(columns(one)[0, k:]).all()
    # the count is per step (explicit_rk.rs:205 starts it at zero in every step()): at loose tolerances a step towards the blow-up is rejected three times in a row,
    # after steps with fewer rejections; a limit of 3 ends there with status 2, a limit of 4 goes on until the step size is too small
    kw = dict(sens_atol=None) if mod is S else {}
    three, four = (mod.solve_ensemble(mid, P1, T_BLOW, rtol=0.1, atol=[1e-2] * 3, options=dict(max_steps=100000, max_error_test_failures=k), **kw) for k in (3, 4))
    assert three["status"][0] == 2 and three["stats"][0, 3] >= 3 and three["stats"][0, 0] >= 1 and four["status"][0] == 1 and four["stats"][0, 3] > three["stats"][0, 3]


@pytest.mark.parametrize("mod", [E, S, EO], ids=["plain", "sens", "out"])
def test_the_failure_count_is_tested_before_the_step_size(mod):
    """runge_kutta.rs:852 comes before :861: with both limits violated at the first rejection the error is TooManyErrorTestFailures (2); the step-size limit alone
    gives StepSizeTooSmall (1) at the same rejection.  min_timestep is read nowhere else: a huge one changes nothing before the first rejection"""
    mid = blow_up()
    both = mod.solve_ensemble(mid, P1, T_BLOW, options=dict(max_steps=100000, max_error_test_failures=1, min_timestep=1e30), **TOL)
    small = mod.solve_ensemble(mid, P1, T_BLOW, options=dict(max_steps=100000, min_timestep=1e30), **TOL)
    assert both["status"][0] == 2 and small["status"][0] == 1
    assert both["stats"][0, 3] == 1 and small["stats"][0, 3] == 1 and np.array_equal(both["stats"], small["stats"])
    assert np.array_equal(columns(both), columns(small), equal_nan=True)


def test_the_stop_time_exits():
    """runge_kutta.rs:436-444 over :752-781: a stop time within the round-off of the current time is StopTimeAtCurrentTime (6), one behind the direction of h
    StopTimeBeforeCurrentTime (5); both before any step.  solve (method.rs:900) has written (t0, y0) by then, solve_dense nothing"""
    for t0 in (0.0, 1.5, -2.0):
        r = E.solve_ensemble(DECAY, P_DECAY, [t0], t0=t0)
        assert (r["status"] == 6).all() and (r["ncols"] == 0).all() and not r["stats"].any() and np.isnan(r["y"]).all() and r["failed"] == 3
        r = E.solve_ensemble(DECAY, P_DECAY, [t0], t0=t0, steps_cap=8)
        assert (r["status"] == 6).all() and (r["ncols"] == 1).all() and not r["stats"].any() and (r["t"][:, 0] == t0).all()
        assert np.array_equal(r["y"][:, 0], np.repeat(P_DECAY[:, 1:2], 2, axis=1)) and np.isnan(r["y"][:, 1:]).all()
        r = E.solve_ensemble(DECAY, P_DECAY, [t0 + 1.0], t0=t0, h0=-1.0)
        assert (r["status"] == 5).all() and (r["ncols"] == 0).all() and not r["stats"].any() and np.isnan(r["y"]).all()
        r = E.solve_ensemble(DECAY, P_DECAY, [t0 + 1.0], t0=t0, h0=-1.0, steps_cap=8)
        assert (r["status"] == 5).all() and (r["ncols"] == 1).all() and (r["t"][:, 0] == t0).all()
    s = S.solve_ensemble(DECAY, P_DECAY, [0.0])
    assert (s["status"] == 6).all() and np.isnan(s["y"]).all() and np.isnan(s["sens"]).all()
    o = EO.solve_ensemble(DECAY, P_DECAY, [1.0], h0=-1.0, steps_cap=4)
    assert (o["status"] == 5).all() and (o["ncols"] == 1).all() and not o["g"][:, 0].any()   # g(t0) = 0


@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("mod", [E, S, EO], ids=["plain", "sens", "out"])
def test_a_run_cut_by_max_steps_has_that_many_steps_and_the_uncut_run_s_columns(mod, group):
    """The device ABI's limit (no counterpart in the reference): one count per step() call, tested before the step, status 99.  A member that needs exactly k steps
    finishes under max_steps = k; one that needs more has k steps and status 99, the columns it reached equal to the uncut run's bit for bit, NaN behind them"""
    free = mod.solve_ensemble(DECAY, P_DECAY, T_DECAY, group=group)
    need = free["stats"][:, 0]
    assert free["failed"] == 0 and (len(set(need.tolist())) > 1 or group == 3)
    for k in (1, int(need.min()), int(need.max()) - 1, int(need.max())):
        cut = mod.solve_ensemble(DECAY, P_DECAY, T_DECAY, group=group, options=dict(max_steps=k))
        over = need > k
        assert np.array_equal(cut["status"], np.where(over, 99, 0)) and cut["failed"] == over.sum()
        assert np.array_equal(cut["stats"][:, 0], np.minimum(need, k)) and np.array_equal(cut["stats"][:, 3], np.where(over, cut["stats"][:, 3], free["stats"][:, 3]))
        nc = ncols_of(cut)
        for b in range(len(P_DECAY)):
            assert np.array_equal(columns(cut)[b, : nc[b]], columns(free)[b, : nc[b]]) and np.isnan(columns(cut)[b, nc[b]:]).all()
            assert nc[b] == len(T_DECAY) if not over[b] else nc[b] < len(T_DECAY)
    if mod is not S:   # every accepted step: column 0 and one column per step
        full = mod.solve_ensemble(DECAY, P_DECAY, [6.0], group=group, steps_cap=64)
        cut = mod.solve_ensemble(DECAY, P_DECAY, [6.0], group=group, steps_cap=64, options=dict(max_steps=2))
        assert (cut["status"] == 99).all() and (cut["ncols"] == 3).all() and (cut["stats"][:, 0] == 2).all()
        assert np.array_equal(columns(cut)[:, :3], columns(full)[:, :3]) and np.array_equal(cut["t"][:, :3], full["t"][:, :3]) and np.isnan(cut["t"][:, 3:]).all()


def test_a_member_that_reaches_its_root_before_the_cap_is_not_cut():
    """the count is tested before a step, never after the last one: a root (or the stop time) found in step k ends the run as a success under max_steps = k"""
    root = ORACLE_MODEL["exponential_decay_with_root"]
    free = E.solve_ensemble(root, P_DECAY, T_DECAY)
    need = free["stats"][:, 0]
    assert (free["root_idx"] == 0).any() and need.min() < need.max()
    k = int(np.sort(need)[1])
    cut = E.solve_ensemble(root, P_DECAY, T_DECAY, options=dict(max_steps=k))
    assert np.array_equal(cut["status"], np.where(need > k, 99, 0)) and (cut["status"] == 0).any() and (cut["status"] == 99).any()
    ok = cut["status"] == 0
    assert np.array_equal(cut["t_root"][ok], free["t_root"][ok], equal_nan=True) and np.isnan(cut["t_root"][~ok]).all() and (cut["root_idx"][~ok] == -1).all()


def test_the_controller_constants_reach_the_factor():
    """runge_kutta.rs:466-495 passes problem.ode_options.pi_control_integral / _proportional to pi_controller_raw (:1313-1336): another pair, another step sequence,
    the same solution within the tolerances"""
    a = E.solve_ensemble(DECAY, P_DECAY, T_DECAY)
    b = E.solve_ensemble(DECAY, P_DECAY, T_DECAY, options=dict(pi_control_integral=0.3, pi_control_proportional=0.4))
    assert b["failed"] == 0 and not np.array_equal(a["stats"][:, 0], b["stats"][:, 0])
    assert np.abs(a["y"] - b["y"]).max() < 1e-4
