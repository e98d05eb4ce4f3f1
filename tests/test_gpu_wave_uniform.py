"""Wavefront lock-step groups of the device-resident BDF (k_bdf_adaptive<.., WAVE = true>) after its group decisions moved to scalar registers and its group
norm to the one-pass maximum (uniform<WAVE>, group_norm_w<WAVE>, dsh_device.hpp wave_max_nonneg_f64): the exact-arithmetic build against the oracle's
lock-step groups of 64, bit for bit — every member's states and all five counters — at ensemble sizes that give shadow lanes, a group of one live member and
several groups with different step counts in one launch, and on an ensemble whose groups fail Newton solves, fail error tests and change order; and the new
maximum against the two-pass one on 64-lane patterns.  Robertson n = 3 with bench.py's tolerances, save points and parameter distribution."""
import numpy as np
import pytest

from helpers import ORACLE_MODEL
from bench import robertson_params, T_EVAL, RTOL, ATOL

pytestmark = pytest.mark.gpu

TOL = dict(rtol=RTOL, atol=ATOL)


@pytest.fixture(scope="module")
def H():
    import diffsol_amd
    return diffsol_amd


@pytest.fixture
def det_pow(O):
    O.set_det_pow(True)
    yield
    O.set_det_pow(False)


def _oracle_groups(O, p):
    yo, so, failed = O.solve_dense_independent(ORACLE_MODEL["robertson_ode"], np.asarray(p, dtype=float), T_EVAL, model_size=1, nthreads=8, group=64, **TOL)
    assert failed == 0
    return np.transpose(yo, (1, 0, 2)), so


def _device_groups(H, p):
    s = H.Solver("robertson_ode", p, nbatch=len(p), model_size=1, **TOL)
    y, tot, m = s.solve_dense_adaptive(T_EVAL, want_member_stats=True, group=64, deterministic_pow=True)  # the exact kernel, the oracle's pow
    assert (m["status"] == 0).all() and tot["failed_members"] == 0
    return y, m["stats"].T


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
def test_lockstep_groups_are_bit_identical_to_the_oracle_at_ragged_ensemble_sizes(H, O, det_pow, nb):
    """1: a group of one live member and 63 shadow lanes; 63 / 65: one shadow lane, one live member in the second group; 64: none; 130: three groups with
    different step counts in one launch."""
    p = robertson_params(130)[:nb]
    yo, so = _oracle_groups(O, p)
    y, stats = _device_groups(H, p)
    if nb == 130:
        assert len({int(so[g, 0]) for g in (0, 64, 128)}) > 1, "the groups were meant to take different numbers of steps"
    assert np.array_equal(stats, so), "counters differ"
    assert np.array_equal(y, yo, equal_nan=True), "states differ"


def wide_params(nb=128, seed=2, width=30.0):
    """Robertson rate constants log-uniform within a factor `width` either side of (0.04, 1e4, 3e7) — bench.py's distribution is the same with a factor 2:
    chosen on the CPU so that both lock-step groups of 64 take every branch the scalar rewrite touched (asserted on the oracle's own counters below)."""
    rng = np.random.default_rng(seed)
    return np.array([0.04, 1e4, 3e7]) * np.exp(rng.uniform(-np.log(width), np.log(width), (nb, 3)))


def test_lockstep_groups_that_fail_newton_solves_and_error_tests_and_change_order_are_bit_identical_to_the_oracle(H, O, det_pow):
    p = wide_params()
    yo, so = _oracle_groups(O, p)
    assert (so[:, 4] > 0).any(), "no Newton convergence failure in the oracle's run"
    assert (so[:, 3] > 0).any(), "no error-test failure in the oracle's run"
    # the oracle's order after every step of the first group (its lock-step batched solver, stepped by hand)
    o = O.OracleSolver(ORACLE_MODEL["robertson_ode"], p[:64], nbatch=64, model_size=1, **TOL)
    o.set_stop_time(T_EVAL[-1])
    orders = [o.state()["order"]]
    while True:
        r = o.step()
        orders.append(o.state()["order"])
        if r == 2:
            break
    assert len(orders) - 1 == so[0, 0], "the hand-stepped group is the group of the dense solve"
    assert np.count_nonzero(np.diff(orders)) > 0 and (np.diff(orders) < 0).any(), "the order never went up and down in the oracle's run"
    y, stats = _device_groups(H, p)
    assert np.array_equal(stats, so), "counters differ"
    assert np.array_equal(y, yo, equal_nan=True), "states differ"


def test_one_pass_wavefront_maximum_has_the_bits_of_the_two_pass_maximum():
    """wave_max_nonneg_f64(v) == wave_max_u64(d2u(v)) bit for bit on non-negative doubles, +inf and a NaN lane (tests/wave_reduce_check)."""
    import wave_reduce_check as W
    rng = np.random.default_rng(7)
    pats, names = [], []

    def add(name, a):
        names.append(name)
        pats.append(np.asarray(a, dtype=np.float64))

    add("all equal", np.full(64, 0.3))
    add("all zero", np.zeros(64))
    base = rng.uniform(0.0, 1.0, 64)
    for lane in (0, 5, 15, 16, 21, 31, 32, 40, 47, 48, 62, 63):  # the maximum in each of the four rows of 16 lanes, at their ends and inside
        a = base.copy()
        a[lane] = 2.0 + lane
        add(f"maximum in lane {lane}", a)
    hi = np.float64(1.5).view(np.uint64)
    for lane in (3, 17, 35, 60):  # equal high words, different low words: only the low 32 bits decide
        lo = rng.integers(0, 2 ** 31, 64, dtype=np.uint64)
        lo[lane] = np.uint64(2 ** 32 - 1)
        add(f"equal high words, largest low word in lane {lane}", (hi + lo).view(np.float64))
    den = (rng.integers(1, 2 ** 52, 64, dtype=np.uint64)).view(np.float64)  # denormals only
    add("denormals", den)
    a = np.zeros(64)
    a[44] = 5e-324
    add("zeros and the smallest denormal", a)
    a = den.copy()
    a[9] = 2.2250738585072014e-308
    add("denormals and the smallest normal", a)
    for lane in (0, 30, 63):
        a = base * 1e300
        a[lane] = np.inf
        add(f"+inf in lane {lane}", a)
    add("all +inf", np.full(64, np.inf))
    for lane in (0, 18, 63):
        a = base.copy()
        a[(lane + 7) % 64] = np.inf
        a[lane] = np.nan
        add(f"one NaN in lane {lane} beside +inf", a)
    for k in range(8):
        add(f"random magnitudes {k}", 10.0 ** rng.uniform(-300, 300, 64))
    P = np.stack(pats)
    new, old = W.wave_max_both(P)
    # the two-pass maximum itself: the largest bit pattern
    assert np.array_equal(old, P.view(np.uint64).max(axis=1))
    for name, a, b in zip(names, new, old):
        assert a == b, f"{name}: one-pass {int(a):#018x}, two-pass {int(b):#018x}"
