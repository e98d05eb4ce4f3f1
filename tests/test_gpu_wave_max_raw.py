"""The lock-step fast BDF kernel with the default options (k_bdf_adaptive<.., FAST, WAVE, DEFOPT>: the instantiation bench.py times) after its wavefront maxima lost
the maximum that only quiets a NaN (dpp_max_f64_raw, wave_max_nonneg_f64_chain_raw in csrc/dsh_adaptive_kernel.hpp; profiles/wave_max_raw.md), against the general
fast kernel <.., FAST, WAVE, DEFOPT = false>, which keeps wave_max_nonneg_f64 with the compiler's quieting maxima: the same call, bit for bit.  On non-negative values
without a NaN the dropped instruction is the identity, and a wavefront with a NaN lane takes the two-pass maximum in both kernels, so nothing may move.

The call is routed to the general kernel as tests/test_gpu_step_chain.py does it (max_steps = default + 1, nothing else changed).  Compared with array_equal on the
bit patterns: the states at every save point, the five per-member counters, status and ncols.

Cases, Robertson with bench.py's tolerances and its seven save points:
  * 64 members (one full group), 100 (a partial last group), 192 (three groups);
  * 192 members, one of the second group with k2 = 1e308 (finite at the start, overflowing to inf - inf = NaN inside the Newton iterations after a few steps) and one
    of the third with a NaN rate constant: their weighted mean squares are NaN, the groups' maxima take the two-pass path.  Both groups fail in both kernels
    (asserted on the general kernel, as a condition on the input) and the first group does not; everything written must still agree;
  * 64 members whose rate constants are all zero, save points 1e-9 of the bench's: f = 0, so every Newton update and every difference is exactly +0 and +0 goes
    through every stage of every maximum (asserted on the general kernel: the states stay (1, 0, 0) exactly).
Exponential decay (N = 2, the same instantiation for another model) at a loose and at a tight tolerance: the order ends at 4 / climbs to 5 and stays, so the order
selection's bodies with ONE norm (order 1, where every solve's first selection runs, and order 5) run as well as those with two (orders 2 to 4).
That the orders are reached is established on the CPU by the unmarked test below (the oracle's lock-step group stepped by hand).  Robertson's groups above also drop
the order; no smooth solve can be held at order 1 by its tolerance, so "driven to 1" is the first selection of every solve."""
import ctypes as C

import numpy as np
import pytest

from helpers import ORACLE_MODEL
from bench import robertson_params, T_EVAL, RTOL, ATOL
from test_gpu_erk import AdaptiveOptions

gpu = pytest.mark.gpu

DECAY_T_EVAL = [0.5, 2.0, 10.0]
DECAY_ATOL = [1e-12, 1e-12]
DECAY_LOOSE, DECAY_TIGHT = 1e-2, 1e-10


def decay_params(nb=64, seed=5):
    """exponential decay y' = -k y, y(0) = y0 in both components: p = (k, y0)"""
    rng = np.random.default_rng(seed)
    return np.stack([0.1 * 2.0 ** rng.uniform(-1, 1, nb), rng.uniform(0.5, 2.0, nb)], axis=1)


def solve(model, size, n, p, atol, rtol, t_eval, **options):
    """dsh_bdf_solve_adaptive, fast arithmetic, lock-step groups of 64, the default options with `options` written over them; one atol [n] for all members.
    Returns y [n_eval, n, nb], stats [5, nb], status [nb], ncols [nb]."""
    import diffsol_amd
    from diffsol_amd import _ffi
    dev = _ffi.load_device_lib()
    c = _ffi.vp()
    _ffi.check(dev.dsh_ctx_create(0, None, C.byref(c)))
    bufs = {}
    try:
        p = np.asarray(p, dtype=float)
        nb, te = len(p), np.ascontiguousarray(t_eval, dtype=float)
        atol = np.ascontiguousarray(atol, dtype=float)
        assert atol.shape == (n,)

        def dmalloc(name, nbytes):
            q = _ffi.vp()
            _ffi.check(dev.dsh_malloc(c, nbytes, 0, C.byref(q)))
            bufs[name] = q
            return q
        for name, arr in (("p", np.ascontiguousarray(p.T)), ("atol", atol)):
            _ffi.check(dev.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(_ffi.vp), arr.nbytes))
        dmalloc("y", 8 * te.size * n * nb); dmalloc("stats", 4 * 5 * nb); dmalloc("status", 4 * nb); dmalloc("ncols", 4 * nb)
        for name in ("y", "stats", "status", "ncols"):  # a failed member leaves columns unwritten: both runs start from the same bytes
            _ffi.check(dev.dsh_memset_zero(c, bufs[name], {"y": 8 * te.size * n * nb, "stats": 20 * nb, "status": 4 * nb, "ncols": 4 * nb}[name]))
        o = AdaptiveOptions()
        dev.dsh_adaptive_default_options(C.byref(o))
        o.deterministic_pow, o.group = 2, 64
        for k, v in options.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        tot = (C.c_int64 * 6)()
        _ffi.check(dev.dsh_bdf_solve_adaptive(c, diffsol_amd.MODELS[model], size, nb, bufs["p"], bufs["atol"], 1, rtol, 0.0, 1.0, C.cast(C.pointer(o), C.c_void_p),
                                              te.ctypes.data_as(_ffi.c_dp), te.size, bufs["y"], bufs["stats"], bufs["status"], None, None, bufs["ncols"], tot))

        def fetch(name, shape, dtype):
            a = np.empty(shape, dtype=dtype)
            _ffi.check(dev.dsh_d2h(c, a.ctypes.data_as(_ffi.vp), bufs[name], a.nbytes))
            return a
        return fetch("y", (te.size, n, nb), np.float64), fetch("stats", (5, nb), np.int32), fetch("status", (nb,), np.int32), fetch("ncols", (nb,), np.int32)
    finally:
        for q in bufs.values():
            dev.dsh_free(c, q)
        dev.dsh_ctx_destroy(c)


def default_max_steps():
    from diffsol_amd import _ffi
    o = AdaptiveOptions()
    _ffi.load_device_lib().dsh_adaptive_default_options(C.byref(o))
    return o.max_steps


def both(model, size, n, p, atol, rtol, t_eval):
    """The default-options kernel against the general fast kernel on the same call, everything bit for bit.  Returns the GENERAL kernel's (y, stats, status, ncols);
    whether its members succeeded is the caller's to assert."""
    ys, ss, sts, ns = solve(model, size, n, p, atol, rtol, t_eval)                                       # every body option at its default: the default-options kernel
    yg, sg, stg, ng = solve(model, size, n, p, atol, rtol, t_eval, max_steps=default_max_steps() + 1)    # one option off: the general fast kernel
    assert np.array_equal(sts, stg), f"status differs in members {np.nonzero(sts != stg)[0][:8]}"
    assert np.array_equal(ns, ng), f"ncols differs in members {np.nonzero(ns != ng)[0][:8]}"
    assert np.array_equal(ss, sg), f"counters differ in members {np.nonzero((ss != sg).any(axis=0))[0][:8]}"
    assert np.array_equal(ys.view(np.uint64), yg.view(np.uint64)), f"states differ in members {np.nonzero((ys.view(np.uint64) != yg.view(np.uint64)).any(axis=(0, 1)))[0][:8]}"
    return yg, sg, stg, ng


def robertson(p, t_eval=T_EVAL):
    return both("robertson_ode", 1, 3, p, ATOL, RTOL, t_eval)


@gpu
@pytest.mark.parametrize("nb", [64, 100, 192])
def test_bits_of_the_general_kernel_on_a_full_group_a_partial_last_group_and_three_groups(nb):
    y, s, st, nc = robertson(robertson_params(192)[:nb])
    assert (st == 0).all() and (nc == len(T_EVAL)).all() and (s[0] > 50).all(), "the general kernel's run is not the solve the case was meant to be"
    print(f"nb = {nb}: steps per group {[int(s[0, g]) for g in range(0, nb, 64)]}, Newton iterations {[int(s[1, g]) for g in range(0, nb, 64)]}")


@gpu
def test_bits_of_the_general_kernel_when_a_lane_of_a_group_holds_a_nan():
    p = robertson_params(192)
    # second group: one member with k2 = 1e308.  Its first steps succeed (x2 = x3 = 0 at the start); then k2 x2 x3 and the Jacobian's k2 x2, k2 x3 overflow, the solve
    # forms inf - inf, and the member's update and weighted mean square are NaN inside the Newton iterations of a running solve (the oracle's lock-step group takes 3
    # steps and then fails every Newton solve until the step size is too small)
    p[64 + 37, 1] = 1e308
    # third group: one member with a NaN rate constant: NaN from the first right-hand side on
    p[128 + 5, 1] = np.nan
    y, s, st, nc = robertson(p)
    groups = [slice(0, 64), slice(64, 128), slice(128, 192)]
    print("non-finite lanes: per group (status, columns, steps, Newton iterations, Newton failures): "
          f"{[(sorted(set(st[g].tolist())), sorted(set(nc[g].tolist())), int(s[0, g][0]), int(s[1, g][0]), int(s[4, g][0])) for g in groups]}")
    assert (st[groups[0]] == 0).all() and (nc[groups[0]] == len(T_EVAL)).all(), "the group without a non-finite member was meant to succeed"
    assert (st[groups[1]] != 0).all() and (s[0, groups[1]] > 0).all() and (s[4, groups[1]] > 0).all(), \
        "the group with the overflowing member was meant to take steps and then fail Newton solves as a whole: the NaN did not reach the group's maxima"
    assert (st[groups[2]] != 0).all(), "a lock-step group with a NaN member was meant to fail as a whole"


@gpu
def test_bits_of_the_general_kernel_when_every_maximum_is_over_exact_zeros():
    te = (1e-9 * np.asarray(T_EVAL)).tolist()
    y, s, st, nc = robertson(np.zeros((64, 3)), t_eval=te)
    print(f"all-zero updates: status {sorted(set(st.tolist()))}, steps {int(s[0, 0])}, Newton iterations {int(s[1, 0])}")
    assert (st == 0).all() and (nc == len(te)).all()
    assert np.array_equal(y.view(np.uint64), np.broadcast_to(np.array([1.0, 0.0, 0.0]).view(np.uint64)[None, :, None], y.shape)), "the states were meant to stay (1, +0, +0) exactly"
    assert (s[0] > 2).all() and (s[3] == 0).all() and (s[4] == 0).all()


def decay_orders(O, rtol):
    """The oracle's lock-step group of 64 stepped by hand: accepted steps per order [7], the orders at which an order selection ran with n_equal_steps > order."""
    o = O.OracleSolver(ORACLE_MODEL["exponential_decay"], decay_params(), nbatch=64, model_size=0, rtol=rtol, atol=np.asarray(DECAY_ATOL, dtype=float))
    o.set_stop_time(DECAY_T_EVAL[-1])
    hist = np.zeros(7, dtype=int)
    while True:
        before = o.state()["order"]
        r = o.step()
        hist[before] += 1
        if r == 2:
            break
    return hist


def test_the_decay_cases_stay_at_order_one_and_reach_order_five(O):
    """No GPU.  Both: two accepted steps at order 1, so n_equal_steps passes 1 there and the order selection runs at order 1 (its single-norm body; a smooth solve
    leaves order 1 at that selection, at any tolerance: 0.9 was tried).  Loose: the solve ends below order 5, every selection beyond the first has two norms.
    Tight: accepted steps at every order up to 5, many at 5 (n_equal_steps passes 5 again and again: the single-norm body of order 5 runs)."""
    loose, tight = decay_orders(O, DECAY_LOOSE), decay_orders(O, DECAY_TIGHT)
    print(f"decay, accepted steps at order 1..5: rtol {DECAY_LOOSE:g}: {loose[1:6].tolist()}; rtol {DECAY_TIGHT:g}: {tight[1:6].tolist()}")
    assert loose[1] >= 2 and (loose[2:5] > 1).all() and loose[5] == 0
    assert tight[1] >= 2 and (tight[1:6] > 0).all() and tight[5] >= 12


@gpu
@pytest.mark.parametrize("rtol", [DECAY_LOOSE, DECAY_TIGHT])
def test_bits_of_the_general_kernel_on_exponential_decay_at_the_lowest_and_the_highest_order(rtol):
    p = decay_params()
    y, s, st, nc = both("exponential_decay", 0, 2, p, DECAY_ATOL, rtol, DECAY_T_EVAL)
    assert (st == 0).all() and (nc == len(DECAY_T_EVAL)).all()
    exact = p[:, 1] * np.exp(-p[:, 0] * DECAY_T_EVAL[-1])
    assert np.allclose(y[-1, 0], exact, rtol=max(50 * rtol, 1e-6)), "the general kernel's run is not a solve of the model"
    print(f"decay rtol {rtol:g}: {int(s[0, 0])} steps, {int(s[1, 0])} Newton iterations")
