"""The group decision the default-options fast lock-step BDF kernel takes by ballot instead of behind a wavefront reduction (newton_first_converged and
ballot_decide_below in dsh_adaptive_kernel.hpp; k_bdf_adaptive<.., FAST, WAVE, DEFOPT>).  The error test by ballot was built and measured slower by itself
(profiles/ballot_decisions.md): it is not in the kernel, and its helper and cases are not here.

1. The helper (tests/ballot_decide_check, compiled with the fast build's flags) against the test it replaces, evaluated beside it on the device: the first Newton
   iteration's `eta08 * sqrt(wave max m) < tol`.  The new decision must equal the old one in EVERY case: random
   wavefronts, the deciding lane at positions 0, 31 and 63, thresholds hit exactly (m = thr2 (1 + k 2^-53) with k inside, on the edge of and outside the band of
   2^-40), zero, a denormal, +inf and a NaN lane, and eta08 = 0, inf, NaN.  The cases inside the band must have gone through the undecided path (the flag the check
   returns): the argument for the band is that the two forms differ by a few units of 2^-53, so a case inside it that did NOT fall back would be decided on rounding.
2. The specialised kernel against the general fast kernel (one option off its default: the reduction-based path), bit for bit: states, five counters and status, on
   ensembles of at most 130 members whose counters show steps that converge in one Newton iteration, steps with three or more, error-test failures and Newton
   failures, on an ensemble whose order goes up and down (a property of the ensemble, asserted on the CPU oracle: the five counters do not hold the order), and on
   Robertson as a DAE (the mass-matrix arm of the peeled update)."""
import numpy as np
import pytest

from bench import robertson_params, T_EVAL
from helpers import ORACLE_MODEL
import test_gpu_default_options as TDO
from test_gpu_wave_uniform import wide_params

pytestmark = pytest.mark.gpu

TOL = 0.2          # nonlinear_solver_tolerance, the default
EPS53 = 2.0 ** -53
KS = [0, 1, 2, 8, 2 ** 10, 2 ** 13, 2 ** 14]


@pytest.fixture(scope="module")
def B():
    import ballot_decide_check
    return ballot_decide_check


def _thr2(eta08):
    q = TOL / np.asarray(eta08, dtype=np.float64)
    return q * q


# ---------------------------------------------------------------- 1. the helper
def test_first_iteration_ballot_makes_the_decision_of_the_reduction_on_random_wavefronts(B):
    rng = np.random.default_rng(11)
    nw = 4096
    eta08 = np.exp(rng.uniform(np.log(1e4 * 2.220446049250313e-16), np.log(320.0), nw))
    m = np.exp2(rng.uniform(-60.0, 20.0, (nw, 64)))
    # half of the wavefronts: every lane well below the threshold but one, which lies within a factor 4 either side of it, at position 0, 31 or 63
    thr2 = _thr2(eta08)
    half = np.arange(nw) % 2 == 0
    m[half] = thr2[half, None] * np.exp2(rng.uniform(-30.0, -3.0, (half.sum(), 64)))
    lane = np.array([0, 31, 63])[np.arange(nw) % 3]
    m[half, lane[half]] = thr2[half] * np.exp2(rng.uniform(-2.0, 2.0, half.sum()))
    new, old, und = B.newton_first(m, eta08, TOL)
    print(f"first iteration, {nw} random wavefronts: converged {int(old.sum())}, undecided {int(und.sum())}")
    assert old.any() and (~old).any(), "the cases were meant to hold both decisions"
    assert np.array_equal(new, old)
    assert und.sum() < nw // 100, "the undecided path is meant to be rare on random values"


@pytest.mark.parametrize("lane", [0, 31, 63])
def test_first_iteration_ballot_at_thresholds_hit_exactly(B, lane):
    rng = np.random.default_rng(12)
    rows, eta, ks = [], [], []
    for e08 in np.concatenate([[1e4 * 2.220446049250313e-16, 320.0, 1.0, 0.2], np.exp(rng.uniform(np.log(1e-11), np.log(320.0), 60))]):
        t2 = float(_thr2(e08))
        for k in [s * k for k in KS for s in (1, -1)]:
            r = t2 * np.exp2(rng.uniform(-30.0, -3.0, 64))
            r[lane] = t2 * (1.0 + k * EPS53)
            rows.append(r); eta.append(e08); ks.append(k)
    ks = np.array(ks)
    new, old, und = B.newton_first(np.array(rows), np.array(eta), TOL)
    assert np.array_equal(new, old), [(k, e) for k, e, a, b in zip(ks, eta, new, old) if a != b][:10]
    inside = np.abs(ks) <= 2 ** 10
    assert und[inside].all(), "a case inside the band was decided by ballot"
    assert not und[np.abs(ks) == 2 ** 14].any(), "a case twice the band away took the reduction"
    assert old[ks == -2 ** 14].all() and not old[ks == 2 ** 14].any()


def test_first_iteration_ballot_with_special_values_in_one_lane_and_special_eta(B):
    rng = np.random.default_rng(13)
    rows, eta = [], []
    for e08 in (1e-9, 0.5, 7.0, 320.0):
        t2 = float(_thr2(e08))
        for scale in (2.0 ** -10, 2.0 ** 3):  # the other lanes all below / one of them above the threshold
            for special in (0.0, 5e-324, 1e-310, np.inf, np.nan):
                for lane in (0, 31, 63):
                    r = t2 * np.exp2(rng.uniform(-30.0, -3.0, 64))
                    r[(lane + 7) % 64] = t2 * scale
                    r[lane] = special
                    rows.append(r); eta.append(e08)
    rows, eta = np.array(rows), np.array(eta)
    new, old, und = B.newton_first(rows, eta, TOL)
    assert np.array_equal(new, old)
    assert und[np.isnan(rows).any(axis=1)].all(), "a wavefront with a NaN lane was decided by ballot"
    assert not old[np.isinf(rows).any(axis=1)].any()
    m = np.exp2(rng.uniform(-60.0, 20.0, (64, 64)))
    m[::4, 5] = 0.0
    for e08 in (0.0, np.inf, np.nan, 5e-324, 1e-170, 1e170):  # (tol / eta08)^2 is not positive, finite and normal: the reduction decides
        new, old, und = B.newton_first(m, e08, TOL)
        assert np.array_equal(new, old), e08
        assert und.all(), e08
    for e08 in (1e-150, 1e150):  # far outside the range eta08 lives in, the threshold still normal: only the equality of the decisions is asked for
        new, old, und = B.newton_first(m, e08, TOL)
        assert np.array_equal(new, old), e08


# ---------------------------------------------------------------- 2. specialised against general fast kernel, bit for bit
def _both(p):
    ys, ss, sts = TDO.solve(p, 2)                                            # every body option at its default: the specialised kernel, decisions by ballot
    yg, sg, stg = TDO.solve(p, 2, max_steps=TDO.default_max_steps() + 1)    # one option off: the general fast kernel, decisions behind the reductions
    assert (sts == 0).all()
    assert np.array_equal(sts, stg) and np.array_equal(ss, sg), "status or counters differ"
    assert np.array_equal(ys.view(np.uint64), yg.view(np.uint64)), "states differ"
    return ss


MAX_ITER = 10  # max_nonlinear_solver_iterations, the default


def _one_iteration_solves(s):
    """Per member: do the counters PROVE a solve that converged in one Newton iteration?  A solve that succeeds (one per accepted step and per error-test failure) takes
    at least one iteration and a failed one (LU failures included) at least none, so fewer than two iterations per successful solve in total leaves one with one."""
    return s[:, 1] < 2 * (s[:, 0] + s[:, 3])


def _three_iteration_solves(s):
    """Per member: do the counters PROVE a successful solve of three or more iterations?  A failed solve takes at most MAX_ITER."""
    return s[:, 1] - MAX_ITER * s[:, 4] > 2 * (s[:, 0] + s[:, 3])


def test_specialised_kernel_has_the_general_kernels_bits_on_groups_that_fail_error_tests_and_newton_solves_and_change_order(O):
    """wide_params() at bench.py's tolerances.  The five counters do not hold the order.  That it goes up and down is a property of the ENSEMBLE, asserted on the
    CPU oracle's first lock-step group stepped by hand, not an observation of the kernel under test (tests/test_gpu_wave_uniform.py holds the exact kernel to that
    group bit for bit, tests/test_gpu_default_options.py the fast kernel's counters to the exact kernel's)."""
    p = wide_params()
    s = _both(p)
    assert (s[:, 3] > 0).any(), "no error-test failure"
    assert (s[:, 4] > 0).any(), "no Newton failure"
    assert _three_iteration_solves(s).any(), "no group whose counters show a solve with three or more Newton iterations"
    O.set_det_pow(True)
    try:
        o = O.OracleSolver(ORACLE_MODEL["robertson_ode"], p[:64], nbatch=64, model_size=1, rtol=TDO.RTOL, atol=TDO.ATOL)
        o.set_stop_time(T_EVAL[-1])
        orders = [o.state()["order"]]
        while True:
            r = o.step()
            orders.append(o.state()["order"])
            if r == 2:
                break
    finally:
        O.set_det_pow(False)
    d = np.diff(orders)
    assert (d > 0).any() and (d < 0).any(), "the order of the first group never went up and down"


@pytest.mark.parametrize("nb", [65, 130])
def test_specialised_kernel_has_the_general_kernels_bits_at_a_tight_tolerance(monkeypatch, nb):
    """robertson_params(130) at rtol = 1e-8.  130 members: three groups (the last one ragged, two live members) that between them show every path the change
    touches, read off the counters: fewer than two Newton iterations per successful solve in one group (some solve converged in ONE iteration: the ballot alone decided, no
    reduction ran), more than two per successful solve in another (some solve took THREE or more: the peeled iterations handed over to the loop), error-test failures
    and Newton failures (a solve is repeated after each: the first iteration's threshold is formed from a reset eta).  65 members: a full group and a group of one live member and 63 shadow lanes."""
    monkeypatch.setattr(TDO, "RTOL", 1e-8)
    s = _both(robertson_params(130)[:nb])
    print(f"rtol 1e-8, nb {nb}: (steps, Newton iterations, error-test failures, Newton failures) per group: {[tuple(int(v) for v in s[g, [0, 1, 3, 4]]) for g in range(0, nb, 64)]}")
    if nb == 130:
        assert _one_iteration_solves(s).any(), "no group whose counters show a solve that converged in one Newton iteration"
        assert _three_iteration_solves(s).any(), "no group whose counters show a solve with three or more Newton iterations"
        assert (s[:, 3] > 0).any() and (s[:, 4] > 0).any(), "no error-test failure or no Newton failure"


def test_specialised_kernel_has_the_general_kernels_bits_on_a_model_with_a_mass_matrix(monkeypatch):
    """The default-options instantiation serves every static model with a fast build, and the peeled update has an arm of its own for a mass matrix (M (x + psi) - c f
    through mass_gemv).  Robertson as a DAE (the third equation algebraic), bench.py's rate constants and tolerances, 65 members: a full group and a ragged one."""
    import diffsol_amd
    monkeypatch.setattr(TDO, "ROBERTSON_ODE", diffsol_amd.MODELS["robertson"])
    s = _both(robertson_params(130)[:65])
    print(f"Robertson DAE, nb 65: (steps, Newton iterations, error-test failures, Newton failures) per group: {[tuple(int(v) for v in s[g, [0, 1, 3, 4]]) for g in (0, 64)]}")
    assert (s[:, 0] > 50).all(), "the run was meant to take a few hundred steps"
