"""The lock-step fast BDF kernel with the default options (k_bdf_adaptive<.., FAST, WAVE, DEFOPT>, dsh_adaptive_fast.hip: the instantiation bench.py times) against the
general fast kernel <.., FAST, WAVE, DEFOPT = false>, bit for bit, on the paths that changes to its step chain touch (profiles/step_chain_round_trips.md): the
step-size change in all four of its inlined copies, the order-indexed tables, the save-point test and the output loop, the error-test failure's controller power.
Such changes move data or move an instruction to the block that reads its result; no floating-point operation, operand or order may change, so the specialised
kernel must keep the general kernel's bits.

The same call is routed to the general kernel as tests/test_gpu_default_options.py does it: max_steps = default + 1 and nothing else changed.  Compared bit for bit:
the states at every save point, the five per-member counters, status and ncols.

Cases: nb = 1, 65, 130 of robertson_params(130) (a group of one live lane, a ragged last group, several groups); wide_params(); robertson_params(130) at rtol = 1e-8
(error-test failures and Newton failures, asserted on the GENERAL kernel's counters as a condition on the inputs: with the stop-time clip and the order selection all
four inlined copies of the step-size change then run, and the error-test failure's controller power is taken); Robertson as a DAE (the mass-matrix arm); and three
save-point lists: 40 logarithmically spaced points in [4e-6, 4e5], the single point 0.4, and bench.py's seven points.  The 40 points are there for an output loop that
emits more than one column per step; on these members that is NOT what they give at the start (the general kernel stopped after three steps has written no column:
its first steps end below 4e-6, and the points are a factor 1.9 apart where the kernel's steps average a factor 1.1), so a fourth list makes that case by
construction: 40 points 4e-11 apart ending at the stop time 400, where a step is tens of time units long.  Its premise is asserted on the general kernel: stopped one
step before the end it has written at most 38 of the 40 columns, so the last step alone writes two or more."""
import ctypes as C

import numpy as np
import pytest

from bench import robertson_params, T_EVAL, RTOL, ATOL
from test_gpu_erk import AdaptiveOptions
from test_gpu_wave_uniform import wide_params

pytestmark = pytest.mark.gpu

ROBERTSON_ODE, MODEL_SIZE = 3, 1  # diffsol_amd.MODELS["robertson_ode"]


def solve(p, t_eval, rtol=RTOL, model=ROBERTSON_ODE, **options):
    """dsh_bdf_solve_adaptive, fast arithmetic, lock-step groups of 64, the default options with `options` written over them.
    Returns y [n_eval, 3, nb], stats [5, nb], status [nb], ncols [nb]."""
    from diffsol_amd import _ffi
    dev = _ffi.load_device_lib()
    c = _ffi.vp()
    _ffi.check(dev.dsh_ctx_create(0, None, C.byref(c)))
    bufs = {}
    try:
        p = np.asarray(p, dtype=float)
        nb, n, te = len(p), 3, np.ascontiguousarray(t_eval, dtype=float)

        def dmalloc(name, nbytes):
            q = _ffi.vp()
            _ffi.check(dev.dsh_malloc(c, nbytes, 0, C.byref(q)))
            bufs[name] = q
            return q
        for name, arr in (("p", np.ascontiguousarray(p.T)), ("atol", np.ascontiguousarray(ATOL, dtype=float))):
            _ffi.check(dev.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(_ffi.vp), arr.nbytes))
        dmalloc("y", 8 * te.size * n * nb); dmalloc("stats", 4 * 5 * nb); dmalloc("status", 4 * nb); dmalloc("ncols", 4 * nb)
        o = AdaptiveOptions()
        dev.dsh_adaptive_default_options(C.byref(o))
        o.deterministic_pow, o.group = 2, 64
        for k, v in options.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        tot = (C.c_int64 * 6)()
        _ffi.check(dev.dsh_bdf_solve_adaptive(c, model, MODEL_SIZE, nb, bufs["p"], bufs["atol"], 1, rtol, 0.0, 1.0, C.cast(C.pointer(o), C.c_void_p),
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


def both(p, t_eval=T_EVAL, **kw):
    """The specialised kernel against the general fast kernel on the same call, everything bit for bit.  Returns the GENERAL kernel's counters [5, nb]."""
    ys, ss, sts, ns = solve(p, t_eval, **kw)                                         # every body option at its default: the specialised kernel
    yg, sg, stg, ng = solve(p, t_eval, max_steps=default_max_steps() + 1, **kw)      # one option off: the general fast kernel, nothing else changes
    assert (stg == 0).all(), "the general kernel failed a member: the case is not what it was meant to be"
    assert (ng == len(t_eval)).all()
    assert np.array_equal(sts, stg), "status differs"
    assert np.array_equal(ns, ng), "ncols differs"
    assert np.array_equal(ss, sg), f"counters differ in members {np.nonzero((ss != sg).any(axis=0))[0][:8]}"
    assert np.array_equal(ys.view(np.uint64), yg.view(np.uint64)), f"states differ in members {np.nonzero((ys.view(np.uint64) != yg.view(np.uint64)).any(axis=(0, 1)))[0][:8]}"
    return sg


@pytest.mark.parametrize("nb", [1, 65, 130])
def test_bits_of_the_general_kernel_on_one_live_lane_a_ragged_group_and_several_groups(nb):
    s = both(robertson_params(130)[:nb])
    if nb == 130:
        assert len({int(s[0, g]) for g in (0, 64, 128)}) > 1, "the groups were meant to take different numbers of steps"


def test_bits_of_the_general_kernel_on_the_wide_ensemble():
    s = both(wide_params())
    assert (s[3] > 0).any() and (s[4] > 0).any(), "the ensemble was meant to fail error tests and Newton solves"


def test_bits_of_the_general_kernel_at_a_tight_tolerance_through_every_copy_of_the_step_size_change():
    s = both(robertson_params(130), rtol=1e-8)  # the general kernel's counters: a condition on the inputs
    print(f"rtol 1e-8: (steps, Newton iterations, set-ups, error-test failures, Newton failures) per group: {[tuple(int(v) for v in s[:, g]) for g in (0, 64, 128)]}")
    assert (s[3] > 0).any(), "no error-test failure anywhere in the ensemble"
    assert (s[4] > 0).any(), "no Newton failure anywhere in the ensemble"


def test_bits_of_the_general_kernel_on_robertson_as_a_dae():
    import diffsol_amd
    s = both(robertson_params(130)[:65], model=diffsol_amd.MODELS["robertson"])
    assert (s[0] > 50).all(), "the run was meant to take a few hundred steps"


SAVE_POINTS = {"log40": np.logspace(np.log10(4e-6), np.log10(4e5), 40), "first_bench_point": np.asarray(T_EVAL, dtype=float)[:1], "bench": np.asarray(T_EVAL, dtype=float),
               "dense40": 400.0 - 4e-11 * np.arange(39, -1, -1)}


@pytest.mark.parametrize("which", list(SAVE_POINTS))
def test_bits_of_the_general_kernel_with_other_save_points(which):
    te = SAVE_POINTS[which]
    if which == "first_bench_point":
        assert te.tolist() == [0.4]
    p = robertson_params(130)[:65]
    s = both(p, t_eval=te)
    assert (s[0] > 0).all()
    if which == "dense40":
        # The premise, on the GENERAL kernel (any max_steps other than the default selects it) and the first group alone (groups are independent): stopped one step
        # before the end (MaxStepsExceeded; ncols is what was written by then) it has written at most 38 columns, so the last step writes two or more.
        assert np.all(np.diff(te) > 0) and te[-1] == 400.0
        steps = int(s[0, 0])
        _, sg, stg, ng = solve(p[:64], te, max_steps=steps - 1)
        print(f"dense40: {steps} steps; stopped after {int(sg[0, 0])}: {int(ng[0])} of {len(te)} columns written, status {int(stg[0])}")
        assert (sg[0] == steps - 1).all() and (stg != 0).all() and (ng <= len(te) - 2).all(), "the last step was meant to pass several save points"
