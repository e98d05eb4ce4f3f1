"""The issue-priority policy of the lock-step fast BDF kernel with the default options (k_bdf_adaptive<.., FAST, WAVE, DEFOPT>, DSH_PAIR_PRIO in dsh_adaptive_kernel.hpp:
where a launch has more wavefronts than the device has SIMDs, the wavefronts of the dispatch's second round switch between s_setprio 1 and 0 by the trip count of
their step loop, so that they and the first round's wavefronts they share a SIMD with take turns at being ahead) is timing only: it may not change a value.  The kernel is held to the general fast kernel <.., FAST, WAVE, DEFOPT = false>, which
has no policy, bit for bit: the same call with max_steps = default + 1 and nothing else changed, as tests/test_gpu_step_chain.py routes it.

Compared: the states at every save point, the five per-member counters, status, ncols and the six ensemble totals.  Robertson with bench.py's tolerances and save
points, at
  64 members                 one wavefront: the launch fits on the SIMDs, the policy is off;
  130 members                three wavefronts, the last with shadow lanes, policy off;
  64 * (4 * CUs + 1) members the smallest launch in which a SIMD must hold two wavefronts: the policy is on, the last wavefront runs both of its phases;
  the same with atol per member (BA = false): the other instantiation that carries the policy."""
import ctypes as C

import numpy as np
import pytest

from bench import robertson_params, T_EVAL, RTOL, ATOL
from test_gpu_erk import AdaptiveOptions
from test_gpu_step_chain import default_max_steps

pytestmark = pytest.mark.gpu

ROBERTSON_ODE, MODEL_SIZE, N = 3, 1, 3  # diffsol_amd.MODELS["robertson_ode"]


def simd_count():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def solve(p, per_member_atol, **options):
    """dsh_bdf_solve_adaptive, fast arithmetic, lock-step groups of 64, the default options with `options` written over them; atol broadcast or one row per member.
    Returns y [n_eval, 3, nb], stats [5, nb], status [nb], ncols [nb], totals [6]."""
    from diffsol_amd import _ffi
    dev = _ffi.load_device_lib()
    c = _ffi.vp()
    _ffi.check(dev.dsh_ctx_create(0, None, C.byref(c)))
    bufs = {}
    try:
        p = np.asarray(p, dtype=float)
        nb, te = len(p), np.ascontiguousarray(T_EVAL, dtype=float)
        atol = np.ascontiguousarray(np.tile(np.asarray(ATOL, dtype=float)[:, None], (1, nb))) if per_member_atol else np.ascontiguousarray(ATOL, dtype=float)

        def dmalloc(name, nbytes):
            q = _ffi.vp()
            _ffi.check(dev.dsh_malloc(c, nbytes, 0, C.byref(q)))
            bufs[name] = q
            return q
        for name, arr in (("p", np.ascontiguousarray(p.T)), ("atol", atol)):
            _ffi.check(dev.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(_ffi.vp), arr.nbytes))
        dmalloc("y", 8 * te.size * N * nb); dmalloc("stats", 4 * 5 * nb); dmalloc("status", 4 * nb); dmalloc("ncols", 4 * nb)
        o = AdaptiveOptions()
        dev.dsh_adaptive_default_options(C.byref(o))
        o.deterministic_pow, o.group = 2, 64
        for k, v in options.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        tot = (C.c_int64 * 6)()
        _ffi.check(dev.dsh_bdf_solve_adaptive(c, ROBERTSON_ODE, MODEL_SIZE, nb, bufs["p"], bufs["atol"], nb if per_member_atol else 1, RTOL, 0.0, 1.0,
                                              C.cast(C.pointer(o), C.c_void_p), te.ctypes.data_as(_ffi.c_dp), te.size, bufs["y"], bufs["stats"], bufs["status"], None, None,
                                              bufs["ncols"], tot))

        def fetch(name, shape, dtype):
            a = np.empty(shape, dtype=dtype)
            _ffi.check(dev.dsh_d2h(c, a.ctypes.data_as(_ffi.vp), bufs[name], a.nbytes))
            return a
        return (fetch("y", (te.size, N, nb), np.float64), fetch("stats", (5, nb), np.int32), fetch("status", (nb,), np.int32), fetch("ncols", (nb,), np.int32),
                np.array(list(tot), dtype=np.int64))
    finally:
        for q in bufs.values():
            dev.dsh_free(c, q)
        dev.dsh_ctx_destroy(c)


def both(nb, per_member_atol=False):
    """The kernel with the policy against the general fast kernel on the same call, everything bit for bit.  Returns the GENERAL kernel's counters [5, nb]."""
    p = robertson_params(nb)
    ys, ss, sts, ns, ts = solve(p, per_member_atol)                                         # every body option at its default: the kernel with the policy
    yg, sg, stg, ng, tg = solve(p, per_member_atol, max_steps=default_max_steps() + 1)      # one option off: the general fast kernel, nothing else changes
    assert (stg == 0).all(), "the general kernel failed a member: the case is not what it was meant to be"
    assert (ng == len(T_EVAL)).all()
    assert np.array_equal(sts, stg), "status differs"
    assert np.array_equal(ns, ng), "ncols differs"
    assert np.array_equal(ss, sg), f"counters differ in members {np.nonzero((ss != sg).any(axis=0))[0][:8]}"
    assert np.array_equal(ts, tg), f"totals differ: {ts} against {tg}"
    assert np.array_equal(tg[:5], sg.astype(np.int64).sum(axis=1)) and tg[5] == 0, "the totals are not the sums of the members' counters"
    assert np.array_equal(ys.view(np.uint64), yg.view(np.uint64)), f"states differ in members {np.nonzero((ys.view(np.uint64) != yg.view(np.uint64)).any(axis=(0, 1)))[0][:8]}"
    return sg


def test_one_wavefront_policy_off():
    s = both(64)
    assert (s[0] > 50).all(), "the run was meant to take a few hundred steps"


def test_three_wavefronts_the_last_with_shadow_lanes():
    s = both(130)
    assert len({int(s[0, g]) for g in (0, 64, 128)}) > 1, "the groups were meant to take different numbers of steps"


@pytest.mark.parametrize("per_member_atol", [False, True], ids=["atol_broadcast", "atol_per_member"])
def test_one_wavefront_more_than_simds_both_phases_of_the_policy(per_member_atol):
    simds = simd_count()
    nb = 64 * (simds + 1)
    s = both(nb, per_member_atol)
    # many more trips of the step loop than a period of the policy in every group, so the wavefront of the second round changes its priority many times
    assert (s[0] > 128).all(), "the run was meant to take a few hundred steps"
