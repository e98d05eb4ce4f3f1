"""The default-options instantiation of the fast lock-step BDF kernel (k_bdf_adaptive<.., FAST = true, DEFOPT = true>, dsh_adaptive_fast.hip), its dispatch, and the
step-size controller's power without the general pow (inv_root_2k_group, dsh_adaptive_kernel.hpp).  Robertson n = 3 with bench.py's tolerances and save points,
dsh_bdf_solve_adaptive called through ctypes with an explicit dsh_adaptive_options.

1. Specialised against general, bit for bit: the default options (deterministic_pow = 2, group = 64) take the specialised kernel; the same options with
   max_steps = default + 1 take the general fast kernel and change nothing else.  States, all five counters and the status must be equal bit for bit, at
   nb = 1, 65, 130 of robertson_params(130) (a group of one live member, shadow lanes, several groups with different step counts) and on wide_params() of
   tests/test_gpu_wave_uniform.py (Newton failures, error-test failures, order changes).
2. Dispatch: one option at a time away from its default.  The fast build's counters equal the exact build's (deterministic_pow = 1) under the same options, states
   within 1e-9, on the first 130 bench members; and the exact build's counters under the varied option differ from those under the defaults — a fast build that
   ignored the option (a wrong dispatch to the specialised kernel) would then reproduce the defaults' counters and fail the first assertion.
   pi_control_integral away from 0.5 also sends the controller's power back to the pow call.
3. The helper (tests/ctrl_pow_check, compiled with the fast build's flags): inside its domain, 2^-100 < x < 2^100 and k = 1..7, within ULP_BOUND units of 2^-53
   relative of x^(-1/(2k)) by powl in 80-bit long double, the exponent formed in long double.  The bound is derived from the algorithm, not measured.  One unit is the
   largest relative error of ONE rounding.  After the first of the two Newton steps w is within 1e-9 of the root (seed 1e-5 or better: the f32 logarithm's absolute error
   at |log2 x| = 100, halved at least; one step turns e into (2k + 1) / 2 e^2 <= 7.5 e^2), so the last step's own truncation, 7.5 x (1e-9)^2, is below 0.1 unit.
   Its residual 1 - x w^2k is one fma (exact up to a rounding of a number of size 1e-8: nothing) of a w^2k that carries roundings: w^2 one, w^4 three, then
   w^k as a product over the bits of k and its square — k = 1: 1, 2: 3, 3: 5, 4: 7, 5: 9, 6: 11, 7: 13 units.  The correction (w / 2k) x residual scales them by 1 / 2k:
   at most 13 / 14 unit of w.  The final fma rounds once: 1 unit.  1 + 13/14 + 0.1 < 2.1 units; the bound is that sum, not doubled.
   +inf returns +0.  Zero, a denormal, a negative number, NaN, arguments beyond the bounds and k outside 1..7 must give the bits of the pow call evaluated beside it.
4. Fast against exact on a small ensemble (the first 200 bench members): every member's five counters equal, states within 1e-9 relative.  wide_params() is not
   a case here: the fast build is not held to 1e-9 on that ensemble (its groups fail Newton solves and error tests, and the fast arithmetic's rounding differences
   grow through them to the order of the bound); test 1 holds the specialised kernel to the general one on it bit for bit."""
import ctypes as C

import numpy as np
import pytest

from bench import robertson_params, T_EVAL, RTOL, ATOL
from test_gpu_erk import AdaptiveOptions
from test_gpu_wave_uniform import wide_params

pytestmark = pytest.mark.gpu

ROBERTSON_ODE, MODEL_SIZE = 3, 1  # diffsol_amd.MODELS["robertson_ode"]
ULP_BOUND = 2.1
LO, HI = 2.0 ** -100, 2.0 ** 100


def solve(p, deterministic_pow, group=64, **options):
    """dsh_bdf_solve_adaptive on Robertson with bench.py's tolerances and save points, the default options with `options` written over them.
    Returns y [nb, n_eval, 3], stats [nb, 5], status [nb]."""
    from diffsol_amd import _ffi
    dev = _ffi.load_device_lib()
    c = _ffi.vp()
    _ffi.check(dev.dsh_ctx_create(0, None, C.byref(c)))
    bufs = {}
    try:
        p = np.asarray(p, dtype=float)
        nb, n, te = len(p), 3, np.ascontiguousarray(T_EVAL, dtype=float)

        def dmalloc(name, nbytes):
            q = _ffi.vp()
            _ffi.check(dev.dsh_malloc(c, nbytes, 0, C.byref(q)))
            bufs[name] = q
            return q
        for name, arr in (("p", np.ascontiguousarray(p.T)), ("atol", np.ascontiguousarray(ATOL, dtype=float))):
            _ffi.check(dev.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(_ffi.vp), arr.nbytes))
        dmalloc("y", 8 * te.size * n * nb); dmalloc("stats", 4 * 5 * nb); dmalloc("status", 4 * nb)
        o = AdaptiveOptions()
        dev.dsh_adaptive_default_options(C.byref(o))
        o.deterministic_pow, o.group = deterministic_pow, group
        for k, v in options.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        tot = (C.c_int64 * 6)()
        _ffi.check(dev.dsh_bdf_solve_adaptive(c, ROBERTSON_ODE, MODEL_SIZE, nb, bufs["p"], bufs["atol"], 1, RTOL, 0.0, 1.0, C.cast(C.pointer(o), C.c_void_p),
                                              te.ctypes.data_as(_ffi.c_dp), te.size, bufs["y"], bufs["stats"], bufs["status"], None, None, None, tot))

        def fetch(name, shape, dtype):
            a = np.empty(shape, dtype=dtype)
            _ffi.check(dev.dsh_d2h(c, a.ctypes.data_as(_ffi.vp), bufs[name], a.nbytes))
            return a
        return fetch("y", (te.size, n, nb), np.float64).transpose(2, 0, 1), fetch("stats", (5, nb), np.int32).T, fetch("status", (nb,), np.int32)
    finally:
        for q in bufs.values():
            dev.dsh_free(c, q)
        dev.dsh_ctx_destroy(c)


def default_max_steps():
    from diffsol_amd import _ffi
    o = AdaptiveOptions()
    _ffi.load_device_lib().dsh_adaptive_default_options(C.byref(o))
    return o.max_steps


def max_rel(yf, ye):
    big = np.abs(ye) > np.asarray(ATOL)[None, None, :]
    return (np.abs(yf - ye)[big] / np.abs(ye)[big]).max()


# ---------------------------------------------------------------- 1. specialised against general, bit for bit
@pytest.mark.parametrize("which", ["nb1", "nb65", "nb130", "wide"])
def test_default_options_kernel_has_the_bits_of_the_general_fast_kernel(which):
    p = wide_params() if which == "wide" else robertson_params(130)[:int(which[2:])]
    ys, ss, sts = solve(p, 2)                                           # every body option at its default: the specialised kernel
    yg, sg, stg = solve(p, 2, max_steps=default_max_steps() + 1)        # one option off: the general fast kernel, nothing else changes
    assert (sts == 0).all()
    if which == "nb130":
        assert len({int(ss[g, 0]) for g in (0, 64, 128)}) > 1, "the groups were meant to take different numbers of steps"
    if which == "wide":
        assert (ss[:, 4] > 0).any() and (ss[:, 3] > 0).any(), "the ensemble was meant to fail Newton solves and error tests"
    assert np.array_equal(sts, stg) and np.array_equal(ss, sg), "status or counters differ"
    assert np.array_equal(ys.view(np.uint64), yg.view(np.uint64)), "states differ"


# ---------------------------------------------------------------- 2. dispatch
@pytest.fixture(scope="module")
def bench_130():
    p = robertson_params(100_000)[:130]
    return p, solve(p, 1)


VARIED = [("nonlinear_solver_tolerance", 0.05), ("nonlinear_solver_tolerance", 0.1), ("nonlinear_solver_tolerance", 0.4),
          ("max_timestep_growth", 3.0), ("max_timestep_growth", 5.0),  # not 1.5: a growth cap below min_timestep_growth = 2 makes the step size change after every step, and the fast build is not held to the exact one's decisions there
          ("pi_control_integral", 0.4), ("pi_control_integral", 0.6), ("pi_control_integral", 0.7),
          ("max_nonlinear_solver_iterations", 3), ("max_nonlinear_solver_iterations", 4), ("max_nonlinear_solver_iterations", 6)]


@pytest.mark.parametrize("name,value", VARIED)
def test_an_option_away_from_its_default_reaches_the_fast_kernel(bench_130, name, value):
    p, (yd, sd, _) = bench_130
    ye, se, ste = solve(p, 1, **{name: value})
    yf, sf, stf = solve(p, 2, **{name: value})
    assert (ste == 0).all() and (stf == 0).all()
    assert not np.array_equal(se, sd), "the exact build's counters do not depend on this value: the case could not detect a wrong dispatch"
    rel = max_rel(yf, ye)
    print(f"{name} = {value}: steps of group 0 {int(se[0, 0])} (defaults: {int(sd[0, 0])}), max relative difference fast / exact {rel:.3e}")
    assert np.array_equal(sf, se), "the fast build's counters are not the exact build's under this option"
    assert rel < 1e-9


# ---------------------------------------------------------------- 3. the helper
@pytest.fixture(scope="module")
def W():
    import ctrl_pow_check
    return ctrl_pow_check


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7])
def test_controller_power_is_within_its_bound_of_the_long_double_power_inside_its_domain(W, k):
    import fast_pow_check
    up, down = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    x = np.concatenate([np.exp2(np.linspace(-99.99, 99.99, 8192)), np.exp(np.linspace(np.log(1e-6), np.log(1e3), 4096)),  # the whole domain; where error norms live
                        [up(LO), down(HI), 1.0, down(1.0), up(1.0), 0.5, 2.0, 4.0 ** k, 4.0 ** -k]])
    new, ocml = W.ctrl_pow_both(x, k)
    e_new, e_ocml = fast_pow_check.err_ulp(x, new, -1, 2 * k), fast_pow_check.err_ulp(x, ocml, -1, 2 * k)
    print(f"inv_root_2k(x, {k}): max error {e_new.max():.3f} units of 2^-53 at x = {x[e_new.argmax()]!r}; ocml pow(x, -(0.5 / {k})) on the same {len(x)} points: {e_ocml.max():.3f}")
    assert np.isfinite(new).all() and e_new.max() <= ULP_BOUND, (e_new.max(), x[e_new.argmax()])


def test_controller_power_of_plus_infinity_is_plus_zero_and_leaves_its_wavefront_on_the_helper(W):
    x = np.full(64, 3.0)
    x[::3] = np.inf
    k = 1 + np.arange(64) % 7
    new, ocml = W.ctrl_pow_both(x, k)
    alone, _ = W.ctrl_pow_both(np.full(64, 3.0), k)
    assert (_bits(new[::3]) == 0).all() and (_bits(ocml[::3]) == 0).all()
    fin = np.isfinite(x)
    assert np.array_equal(_bits(new[fin]), _bits(alone[fin])), "a +inf lane changed what the other lanes return"


def test_outside_its_domain_the_controller_power_returns_the_bits_of_the_pow_call(W):
    special = [0.0, -0.0, 5e-324, 1e-310, -1.5, -np.inf, np.nan, LO, np.nextafter(LO, 0.0), HI, np.nextafter(HI, np.inf), 1e-40, 1e40]
    for bad in special:  # one bad lane sends the whole wavefront to the call: the in-domain lanes return pow's bits too
        for lane in (0, 37):
            x = np.exp2(np.linspace(-20.0, 20.0, 64))
            x[lane] = bad
            k = 1 + np.arange(64) % 7
            new, ocml = W.ctrl_pow_both(x, k)
            assert np.array_equal(_bits(new), _bits(ocml)), (bad, lane, [(a, hex(b), hex(c)) for a, b, c in zip(x, _bits(new), _bits(ocml)) if b != c])
    for kbad in (0, 8, -1, 15):
        x = np.exp2(np.linspace(-20.0, 20.0, 64))
        k = 1 + np.arange(64) % 7
        k[11] = kbad
        new, ocml = W.ctrl_pow_both(x, k)
        assert np.array_equal(_bits(new), _bits(ocml)), (kbad, [(a, hex(b), hex(c)) for a, b, c in zip(x, _bits(new), _bits(ocml)) if b != c])
    x = np.concatenate([np.array(special), [np.inf]])  # every special at once, +inf among them
    new, ocml = W.ctrl_pow_both(x, 3)
    assert np.array_equal(_bits(new), _bits(ocml))


# ---------------------------------------------------------------- 4. fast against exact on small ensembles
def test_fast_build_makes_the_exact_builds_decisions_on_the_first_200_bench_members():
    which, p = "bench200", robertson_params(100_000)[:200]
    ye, se, ste = solve(p, 1)
    yf, sf, stf = solve(p, 2)
    assert (ste == 0).all() and (stf == 0).all()
    rel = max_rel(yf, ye)
    print(f"{which}: max relative difference fast / exact {rel:.3e}")
    assert np.array_equal(sf, se), "the five per-member counters differ"
    assert rel < 1e-9
