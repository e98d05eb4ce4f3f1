"""The lock-step fast BDF kernel with the default options (k_bdf_adaptive<.., FAST, WAVE, DEFOPT>: the instantiation bench.py times) after its prediction, its update
of the differences and the column pick of its order selection became per-order bodies behind one scalar dispatch on the wavefront-uniform order, with the Bdf::_new
coefficients of that order as compile-time constants (profiles/order_paths.md), against the general fast kernel <.., FAST, WAVE, DEFOPT = false>, which keeps the
per-column guards and reads the tables the host fills: the same call, bit for bit.  Per component the per-order bodies run the guarded form's operations on its
operands in its order, so nothing may move.

The call is routed to the general kernel as tests/test_gpu_step_chain.py does it (max_steps = default + 1, nothing else changed).  Compared bit for bit: the states
at every save point, the five per-member counters, status and ncols.

Cases: nb = 1, 65, 130 of robertson_params(130) at bench.py's tolerances and save points; the same 130 members at rtol = 1e-8; wide_params(); Robertson as a DAE (the
mass-matrix arm); and exponential decay (N = 2, another instantiation dispatch_static_model sends here) with one atol for all members and with per-member atol (both
values of the kernel's BA).

A condition on the inputs, established on the CPU by the unmarked test below: the oracle's lock-step solver (nbatch = 64) stepped by hand on the first group of every
case.  Together the cases take accepted steps at every order 1..5, and the order goes down and goes up.  The histogram per case is printed."""
import ctypes as C

import numpy as np
import pytest

from helpers import ORACLE_MODEL
from bench import robertson_params, T_EVAL, RTOL, ATOL
from test_gpu_erk import AdaptiveOptions
from test_gpu_step_chain import both, default_max_steps
from test_gpu_wave_uniform import wide_params

gpu = pytest.mark.gpu

DECAY_T_EVAL = [0.5, 2.0, 10.0]
DECAY_RTOL = 1e-6


def decay_params(nb=65, seed=5):
    """exponential decay y' = -k y, y(0) = y0 in both components: p = (k, y0)"""
    rng = np.random.default_rng(seed)
    return np.stack([0.1 * 2.0 ** rng.uniform(-1, 1, nb), rng.uniform(0.5, 2.0, nb)], axis=1)


def decay_atol(nb, per_member):
    if not per_member:
        return np.array([1e-8, 1e-8])
    return 1e-8 * 2.0 ** np.random.default_rng(6).uniform(-1, 1, (2, nb))  # [n, nb]: every member its own


# name -> (oracle model, model size, parameters of the first group, rtol, atol [n], stop time)
def cases():
    r130 = robertson_params(130)
    d = decay_params()
    return {
        "robertson nb=1": ("robertson_ode", 1, r130[:1], RTOL, ATOL, T_EVAL[-1]),
        "robertson nb=65/130": ("robertson_ode", 1, r130[:64], RTOL, ATOL, T_EVAL[-1]),
        "robertson rtol=1e-8": ("robertson_ode", 1, r130[:64], 1e-8, ATOL, T_EVAL[-1]),
        "wide": ("robertson_ode", 1, wide_params()[:64], RTOL, ATOL, T_EVAL[-1]),
        "robertson dae": ("robertson", 0, r130[:64], RTOL, ATOL, T_EVAL[-1]),
        # the oracle's batched solver takes one atol for the whole batch: the per-member-atol case of the device has no counterpart here and adds nothing to the count
        "decay, one atol": ("exponential_decay", 0, d[:64], DECAY_RTOL, decay_atol(65, False), DECAY_T_EVAL[-1]),
    }


def test_the_cases_run_every_order_as_the_order_of_an_accepted_step_and_an_order_decrease_and_increase(O):
    """No GPU: the oracle's lock-step group of 64 (its batched solver) stepped by hand on the first group of every case."""
    total = np.zeros(7, dtype=int)
    went_up = went_down = False
    for name, (model, size, p, rtol, atol, t_stop) in cases().items():
        o = O.OracleSolver(ORACLE_MODEL[model], p, nbatch=len(p), model_size=size, rtol=rtol, atol=np.asarray(atol, dtype=float).reshape(-1))
        o.set_stop_time(t_stop)
        hist = np.zeros(7, dtype=int)
        up = down = 0
        while True:
            before = o.state()["order"]   # the order the step that is accepted next runs at
            r = o.step()
            after = o.state()["order"]
            hist[before] += 1
            up += after > before
            down += after < before
            if r == 2:
                break
        print(f"{name}: accepted steps at order 1..5: {hist[1:6].tolist()}, order increases {up}, decreases {down}")
        assert hist[0] == 0 and hist[6] == 0
        total += hist
        went_up, went_down = went_up or up > 0, went_down or down > 0
    print(f"all cases: accepted steps at order 1..5: {total[1:6].tolist()}")
    assert (total[1:6] > 0).all(), f"an order is never the order of an accepted step: {total[1:6].tolist()}"
    assert went_up and went_down


@gpu
@pytest.mark.parametrize("nb", [1, 65, 130])
def test_bits_of_the_general_kernel_on_one_live_lane_a_ragged_group_and_several_groups(nb):
    both(robertson_params(130)[:nb])


@gpu
def test_bits_of_the_general_kernel_at_a_tight_tolerance():
    both(robertson_params(130), rtol=1e-8)


@gpu
def test_bits_of_the_general_kernel_on_the_wide_ensemble():
    s = both(wide_params())
    assert (s[3] > 0).any() and (s[4] > 0).any(), "the ensemble was meant to fail error tests and Newton solves"


@gpu
def test_bits_of_the_general_kernel_on_robertson_as_a_dae():
    import diffsol_amd
    s = both(robertson_params(130)[:65], model=diffsol_amd.MODELS["robertson"])
    assert (s[0] > 50).all()


def solve_decay(p, atol, **options):
    """dsh_bdf_solve_adaptive on exponential decay, fast arithmetic, lock-step groups of 64; atol [2] (one for all members) or [2, nb].
    Returns y [n_eval, 2, nb], stats [5, nb], status [nb], ncols [nb]."""
    import diffsol_amd
    from diffsol_amd import _ffi
    dev = _ffi.load_device_lib()
    c = _ffi.vp()
    _ffi.check(dev.dsh_ctx_create(0, None, C.byref(c)))
    bufs = {}
    try:
        nb, n, te = len(p), 2, np.ascontiguousarray(DECAY_T_EVAL, dtype=float)
        atol = np.ascontiguousarray(atol, dtype=float)
        atol_nb = 1 if atol.ndim == 1 else nb
        assert atol.shape == ((n,) if atol_nb == 1 else (n, nb))

        def dmalloc(name, nbytes):
            q = _ffi.vp()
            _ffi.check(dev.dsh_malloc(c, nbytes, 0, C.byref(q)))
            bufs[name] = q
            return q
        for name, arr in (("p", np.ascontiguousarray(np.asarray(p, dtype=float).T)), ("atol", atol)):
            _ffi.check(dev.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(_ffi.vp), arr.nbytes))
        dmalloc("y", 8 * te.size * n * nb); dmalloc("stats", 4 * 5 * nb); dmalloc("status", 4 * nb); dmalloc("ncols", 4 * nb)
        o = AdaptiveOptions()
        dev.dsh_adaptive_default_options(C.byref(o))
        o.deterministic_pow, o.group = 2, 64
        for k, v in options.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        tot = (C.c_int64 * 6)()
        _ffi.check(dev.dsh_bdf_solve_adaptive(c, diffsol_amd.MODELS["exponential_decay"], 0, nb, bufs["p"], bufs["atol"], atol_nb, DECAY_RTOL, 0.0, 1.0,
                                              C.cast(C.pointer(o), C.c_void_p), te.ctypes.data_as(_ffi.c_dp), te.size, bufs["y"], bufs["stats"], bufs["status"], None, None,
                                              bufs["ncols"], tot))

        def fetch(name, shape, dtype):
            a = np.empty(shape, dtype=dtype)
            _ffi.check(dev.dsh_d2h(c, a.ctypes.data_as(_ffi.vp), bufs[name], a.nbytes))
            return a
        return fetch("y", (te.size, n, nb), np.float64), fetch("stats", (5, nb), np.int32), fetch("status", (nb,), np.int32), fetch("ncols", (nb,), np.int32)
    finally:
        for q in bufs.values():
            dev.dsh_free(c, q)
        dev.dsh_ctx_destroy(c)


@gpu
@pytest.mark.parametrize("per_member_atol", [False, True])
def test_bits_of_the_general_kernel_on_exponential_decay_with_shared_and_per_member_atol(per_member_atol):
    p = decay_params()
    atol = decay_atol(len(p), per_member_atol)
    ys, ss, sts, ns = solve_decay(p, atol)
    yg, sg, stg, ng = solve_decay(p, atol, max_steps=default_max_steps() + 1)
    assert (stg == 0).all() and (ng == len(DECAY_T_EVAL)).all() and (sg[0] > 20).all()
    exact = p[:, 1] * np.exp(-p[:, 0] * DECAY_T_EVAL[-1])
    assert np.allclose(yg[-1, 0], exact, rtol=1e-3), "the general kernel's run is not a solve of the model"
    assert np.array_equal(sts, stg), "status differs"
    assert np.array_equal(ns, ng), "ncols differs"
    assert np.array_equal(ss, sg), f"counters differ in members {np.nonzero((ss != sg).any(axis=0))[0][:8]}"
    assert np.array_equal(ys.view(np.uint64), yg.view(np.uint64)), f"states differ in members {np.nonzero((ys.view(np.uint64) != yg.view(np.uint64)).any(axis=(0, 1)))[0][:8]}"
