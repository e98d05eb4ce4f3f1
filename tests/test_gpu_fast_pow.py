"""The fixed-exponent powers of the fast BDF build's Newton chain (pow_p08, root_k: dsh_adaptive_kernel.hpp, used under FAST only).

* The helpers themselves (tests/fast_pow_check, compiled with the fast build's flags): inside their domain within 4 ulp (4 x 2^-53 relative) of the power by powl in
  80-bit long double; outside it — zero, denormal, negative, infinite, NaN, beyond the stated bounds, and k other than 2 and 3 — the bits of the plain pow call
  evaluated in the same program.
  The bound is derived, not measured: pow_p08's last division-free Newton step for x^(-1/5) starts from a relative error of some 1e-11 and leaves w within about 1 ulp
  (the residual 1 - x w^5 is one fma of a w^5 that carries three roundings, the correction 0.2 w r is then off by under 0.7 ulp of w, and the final fma rounds once
  more), the product x w adds half an ulp: 2 ulp, doubled.  sqrt is correctly rounded and ocml documents cbrt at 1 ulp.
* Robertson with the bench's tolerances on the first 200 members of the bench's ensemble: in lock-step groups the fast build (deterministic_pow = 2) makes the exact
  kernel's (deterministic_pow = 1) step decisions in the three full groups — they are groups 0 to 2 of the full-size ensemble, where
  tests/test_gpu_adaptive.py requires it — and stays within the solver's tolerance in the ragged fourth group and under per-member control."""
import numpy as np
import pytest

from bench import robertson_params, T_EVAL, RTOL, ATOL

pytestmark = pytest.mark.gpu

TOL = dict(rtol=RTOL, atol=ATOL)
EPS = 2.220446049250313e-16
MIN_ETA = 1e4 * EPS                               # the kernel clamps eta to this from below
ETA_RESET, ETA_RESET_TS = 20.0 ** 1.25, 100.0 ** 1.25  # the two reset constants (convergence.rs:36-42)
P08_LO, P08_HI = 2.0 ** -100, 2.0 ** 100          # pow_p08's domain is the open interval
DBL_MIN, DBL_MAX = np.finfo(np.float64).tiny, np.finfo(np.float64).max
ULP_BOUND = 4.0


@pytest.fixture(scope="module")
def W():
    import fast_pow_check
    return fast_pow_check


@pytest.fixture(scope="module")
def H():
    import diffsol_amd
    return diffsol_amd


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _up(x):
    return np.nextafter(x, np.inf)


def _down(x):
    return np.nextafter(x, -np.inf)


def test_pow_p08_is_within_4_ulp_of_the_long_double_power_inside_its_domain(W):
    x = np.concatenate([
        np.exp(np.linspace(np.log(MIN_ETA), np.log(9.0), 4096)),
        [MIN_ETA, 9.0, _down(ETA_RESET), ETA_RESET, _up(ETA_RESET), _down(ETA_RESET_TS), ETA_RESET_TS, _up(ETA_RESET_TS), _up(P08_LO), _down(P08_HI), 1.0, _down(1.0), _up(1.0)],
    ])
    new, ocml = W.fast_pow_both(x, 0)
    e_new, e_ocml = W.err_ulp(x, new, 4, 5), W.err_ulp(x, ocml, 4, 5)
    print(f"pow_p08: max error {e_new.max():.3f} ulp at x = {x[e_new.argmax()]!r}; ocml pow(x, 0.8) on the same {len(x)} points: {e_ocml.max():.3f} ulp")
    assert np.isfinite(new).all() and e_new.max() <= ULP_BOUND, (e_new.max(), x[e_new.argmax()])


@pytest.mark.parametrize("k", [2, 3])
def test_root_k_is_within_4_ulp_of_the_long_double_root_inside_its_domain(W, k):
    x = np.concatenate([np.exp(np.linspace(np.log(1e-12), np.log(0.9), 4096)), [1e-12, 0.9, DBL_MIN, DBL_MAX, 1.0, _down(1.0), _up(1.0), 0.25, 0.125, 1e-300, 1e300]])
    new, ocml = W.fast_pow_both(x, k)
    e_new, e_ocml = W.err_ulp(x, new, 1, k), W.err_ulp(x, ocml, 1, k)
    print(f"root_k(x, {k}): max error {e_new.max():.3f} ulp at x = {x[e_new.argmax()]!r}; ocml pow(x, 1.0 / {k}) on the same {len(x)} points: {e_ocml.max():.3f} ulp")
    assert np.isfinite(new).all() and e_new.max() <= ULP_BOUND, (e_new.max(), x[e_new.argmax()])


def test_outside_their_domain_the_helpers_return_the_bits_of_the_plain_pow_call(W):
    special = [0.0, -0.0, 5e-324, 1e-310, _down(DBL_MIN), -1.5, -MIN_ETA, -np.inf, np.inf, np.nan]
    x = np.array(special + [P08_LO, _down(P08_LO), P08_HI, _up(P08_HI), 1e-40, 1e40, DBL_MIN, DBL_MAX])
    new, ocml = W.fast_pow_both(x, 0)
    assert np.array_equal(_bits(new), _bits(ocml)), [(a, hex(b), hex(c)) for a, b, c in zip(x, _bits(new), _bits(ocml)) if b != c]
    for k in (2, 3):  # just outside: the largest denormal below, +inf above
        x = np.array(special)
        new, ocml = W.fast_pow_both(x, k)
        assert np.array_equal(_bits(new), _bits(ocml)), (k, [(a, hex(b), hex(c)) for a, b, c in zip(x, _bits(new), _bits(ocml)) if b != c])
    for k in (4, 5, 1, 7):  # every other k is the general call, inside the domain of k = 2, 3 as well
        x = np.array(special + list(np.exp(np.linspace(np.log(1e-12), np.log(0.9), 64))) + [DBL_MIN, DBL_MAX, 1.0, 9.0])
        new, ocml = W.fast_pow_both(x, k)
        assert np.array_equal(_bits(new), _bits(ocml)), (k, [(a, hex(b), hex(c)) for a, b, c in zip(x, _bits(new), _bits(ocml)) if b != c])


@pytest.fixture(scope="module")
def robertson_200(H):
    """The first 200 members of the bench's ensemble: the exact kernel in lock-step groups and per member, computed once."""
    p = robertson_params(100_000)[:200]
    s = H.Solver("robertson_ode", p, nbatch=len(p), model_size=1, **TOL)
    exact = {g: s.solve_dense_adaptive(T_EVAL, group=g, deterministic_pow=1, want_member_stats=True) for g in (64, 1)}
    return s, exact


def test_fast_build_makes_the_exact_kernels_decisions_in_the_first_three_groups_of_the_bench_ensemble(robertson_200):
    s, exact = robertson_200
    ye, tote, me = exact[64]
    yf, totf, mf = s.solve_dense_adaptive(T_EVAL, group=64, deterministic_pow=2, want_member_stats=True)
    assert tote["failed_members"] == 0 and totf["failed_members"] == 0 and (mf["status"] == 0).all()
    full = slice(0, 192)  # groups 0 - 2
    assert np.array_equal(np.asarray(me["stats"])[:, full], np.asarray(mf["stats"])[:, full]), "the five per-member counters differ in a full group"
    assert np.asarray(me["stats"]).shape[0] == 5
    big = np.abs(ye[:, full]) > np.asarray(ATOL)[None, None, :]
    rel = (np.abs(yf[:, full] - ye[:, full])[big] / np.abs(ye[:, full])[big]).max()
    print(f"groups 0-2: max relative difference fast / exact {rel:.3e}")
    assert rel < 1e-9
    # the ragged fourth group (8 live members, 56 shadow lanes): decisions may differ from the full-size run's group 3, the solver's tolerance holds
    assert (np.asarray(mf["status"])[192:] == 0).all()
    assert np.allclose(yf[:, 192:], ye[:, 192:], rtol=5e-3, atol=1e-9)


def test_fast_build_under_per_member_control_stays_within_the_solvers_tolerance_of_the_exact_kernel(robertson_200):
    s, exact = robertson_200
    ye, tote, me = exact[1]
    yf, totf, mf = s.solve_dense_adaptive(T_EVAL, group=1, deterministic_pow=2, want_member_stats=True)
    assert tote["failed_members"] == 0 and totf["failed_members"] == 0 and (mf["status"] == 0).all()
    assert np.allclose(yf, ye, rtol=5e-3, atol=1e-9)
