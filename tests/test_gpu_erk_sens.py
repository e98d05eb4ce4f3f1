"""Device-resident Tsit45 with forward sensitivities (dsh_erk_solve_resident_sens, k_erk_resident<.., SENS = true>) against the CPU checker (tests/erk_sens_ref):
bitwise parity of states, sensitivities, the five counters and the status with the portable pow on both sides, per member (group 1) and in wavefront lock-step
(group 64: the checker runs each 64-member group as one batched problem); the output-sensitivity and fit entries on top of it; the closed form under the reference's
acceptance bound; members that do not finish; the refusals.

nb = 70 unless a test says otherwise: one full wavefront plus six lanes, so the lanes that shadow the wavefront's first member and the group reductions both take part.
"""
import ctypes as C

import numpy as np
import pytest

import erk_sens_ref as S
import out_fit_models as F
import out_sens_models as M
from helpers import ORACLE_MODEL
from test_erk_sens_ref_golden import BOUND, SWEEP_T, sweep_params, worst_norms
from test_gpu_erk import AdaptiveOptions
from test_gpu_out_sens import Dev, _kernel_on

pytestmark = pytest.mark.gpu

NB = 70
T_EVAL = [0.0, 0.5, 1.0, 2.0, 4.0]   # t0 itself is a save point; the first steps are short, the last ones pass more than one save point
TOL = dict(rtol=1e-6, atol=[1e-6, 1e-6])


@pytest.fixture(scope="module")
def H():
    import diffsol_amd
    return diffsol_amd


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


@pytest.fixture(autouse=True)
def det_pow():
    S.set_det_pow(True)
    yield
    S.set_det_pow(False)


def device_solve(model, size, p, t_eval, rtol, atol, group, sens=True, sens_rtol=1e-6, sens_atol=(1e-6,), max_steps=None, t0=0.0, h0=1.0,
                 options=None):
    """dsh_erk_solve_resident_sens (sens=True) or dsh_erk_solve_resident through the device C ABI: per-member atol and max_steps travel only there.  atol [n] or
    [nb, n]; sens_atol None: out of the error control; options: fields of dsh_adaptive_options to set over the defaults.  Returns dict(y [nb, nt, n], sens [np, nb, nt, n], stats [nb, 5], status [nb], totals)."""
    from diffsol_amd import _ffi
    L = _ffi.load_device_lib()
    c = _ffi.vp()
    _ffi.check(L.dsh_ctx_create(0, None, C.byref(c)))
    bufs = {}
    try:
        nb, npar = p.shape
        info = [C.c_int64(), C.c_int64(), C.c_int(), C.c_int64()]
        _ffi.check(L.dsh_model_info(model, size, C.byref(info[0]), C.byref(info[1]), C.byref(info[2]), C.byref(info[3])))
        n, nt = info[0].value, len(t_eval)
        at = np.asarray(atol, dtype=float)
        a_host = np.ascontiguousarray(at.T if at.ndim == 2 else at)   # device layout: n x nb, batch-fastest
        p_host = np.ascontiguousarray(p.T)

        def dmalloc(name, nbytes):
            q = _ffi.vp()
            _ffi.check(L.dsh_malloc(c, nbytes, 0, C.byref(q)))
            bufs[name] = q
            return q
        for name, arr in (("p", p_host), ("atol", a_host)):
            _ffi.check(L.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(_ffi.vp), arr.nbytes))
        dmalloc("y", 8 * nt * n * nb); dmalloc("sens", 8 * nt * npar * n * nb); dmalloc("stats", 4 * 5 * nb); dmalloc("status", 4 * nb)
        o = AdaptiveOptions()
        L.dsh_adaptive_default_options(C.byref(o))
        o.deterministic_pow, o.group = 1, group
        if max_steps is not None:
            o.max_steps = max_steps
        for k, v in (options or {}).items():
            getattr(o, k)   # an unknown field is an error, not a new attribute
            setattr(o, k, v)
        opts = C.cast(C.pointer(o), C.c_void_p)
        tot = (C.c_int64 * 6)()
        te = np.ascontiguousarray(t_eval, dtype=float)
        if sens:
            sa = np.zeros(1) if sens_atol is None else np.ascontiguousarray(np.asarray(sens_atol, dtype=float).reshape(-1))
            rc = L.dsh_erk_solve_resident_sens(c, 3, model, size, nb, bufs["p"], bufs["atol"], nb if at.ndim == 2 else 1, rtol, t0, h0, opts, te.ctypes.data_as(_ffi.c_dp),
                                               te.size, sens_rtol, sa.ctypes.data_as(_ffi.c_dp), 0 if sens_atol is None else sa.size, bufs["y"], bufs["sens"], bufs["stats"],
                                               bufs["status"], tot)
        else:
            rc = L.dsh_erk_solve_resident(c, 3, model, size, nb, bufs["p"], bufs["atol"], nb if at.ndim == 2 else 1, rtol, t0, h0, opts, te.ctypes.data_as(_ffi.c_dp),
                                          te.size, bufs["y"], bufs["stats"], bufs["status"], None, None, None, tot)
        _ffi.check(rc)

        def fetch(name, shape, dtype):
            a = np.empty(shape, dtype=dtype)
            _ffi.check(L.dsh_d2h(c, a.ctypes.data_as(_ffi.vp), bufs[name], a.nbytes))
            return a
        out = dict(y=fetch("y", (nt, n, nb), np.float64).transpose(2, 0, 1), stats=fetch("stats", (5, nb), np.int32).T, status=fetch("status", (nb,), np.int32),
                   totals=[int(v) for v in tot])
        if sens:
            out["sens"] = fetch("sens", (nt, npar, n, nb), np.float64).transpose(1, 3, 0, 2)   # [col][parameter][state][b] -> [parameter][b][col][state]
        return out
    finally:
        for q in bufs.values():
            L.dsh_free(c, q)
        L.dsh_ctx_destroy(c)


def assert_same(dv, ref):
    assert ref["failed"] == 0 and not dv["status"].any() and not ref["status"].any()
    assert np.array_equal(dv["stats"], ref["stats"]) and np.array_equal(dv["status"], ref["status"])
    assert np.isfinite(dv["y"]).all() and np.isfinite(dv["sens"]).all()
    assert np.array_equal(dv["y"], ref["y"]), f"y: max |diff| {np.abs(dv['y'] - ref['y']).max()}"
    assert np.array_equal(dv["sens"], ref["sens"]), f"sens: max |diff| {np.abs(dv['sens'] - ref['sens']).max()}"
    assert dv["totals"][0] == int(dv["stats"][:, 0].sum()) and dv["totals"][3] == int(dv["stats"][:, 3].sum()) and dv["totals"][5] == 0


def per_member_atol(nb):
    return np.asarray(TOL["atol"])[None, :] * 10.0 ** np.random.default_rng(nb).uniform(-1, 1, (nb, 1))


@pytest.mark.parametrize("error_control", [True, False])
@pytest.mark.parametrize("per_member", [False, True])
@pytest.mark.parametrize("group", [1, 64])
def test_bitwise_parity_with_the_checker_exponential_decay(H, group, per_member, error_control):
    """1. the built-in exponential_decay; nb = 70, and once more a single member (the BA = false form)"""
    for nb in (NB, 1):
        p = sweep_params(nb, seed=3 + nb)
        atol = per_member_atol(nb) if per_member else TOL["atol"]
        sa = (1e-6,) if error_control else None
        dv = device_solve(H.MODELS["exponential_decay"], 0, p, T_EVAL, TOL["rtol"], atol, group, sens_atol=sa)
        ref = S.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, T_EVAL, rtol=TOL["rtol"], atol=atol, sens_atol=sa, group=group)
        assert_same(dv, ref)
        assert np.array_equal(dv["sens"][1, :, 0], np.ones((nb, 2))) and not dv["sens"][0, :, 0].any()   # the column at t0: dy0/dy0 = 1, dy0/dk = 0
        if group == 1 and nb > 64:
            assert dv["stats"][:, 0].min() < dv["stats"][:, 0].max()
    if error_control and not per_member:  # the sensitivities in the error test cost steps: the control is not a no-op
        off = device_solve(H.MODELS["exponential_decay"], 0, p, T_EVAL, TOL["rtol"], atol, group, sens_atol=None)
        assert off["totals"][0] <= dv["totals"][0]


_compiled = {}


def _diffsl(name):
    """(DiffslModel, HostTwin, the checker's id of the host twin of the equations) of a text of out_sens_models, compiled once per session"""
    import diffsl_models as DM
    from diffsol_amd import diffsl
    if name not in _compiled:
        code = {"transcendental": M.TRANSCENDENTAL, "decay": M.DECAY}[name]
        so, _ = DM.host_model_so(code)
        _compiled[name] = (diffsl.DiffslModel(code), M.HostTwin(code), S.load_external_model(so))
    return _compiled[name]


@pytest.mark.parametrize("error_control", [True, False])
@pytest.mark.parametrize("group", [1, 64])
def test_bitwise_parity_with_the_checker_diffsl_model(H, group, error_control):
    """2. TRANSCENDENTAL of out_sens_models (x(0) = y0 is a parameter: init_sens_mul is not zero) through the run-time-compiled kernel, its host twin in the checker"""
    m, _, ref_id = _diffsl("transcendental")
    assert (m.n, m.nparams) == (2, 2)
    p = np.random.default_rng(5).uniform(0.5, 2.0, (NB, 2))
    atol, sa = [1e-8, 1e-8], ((1e-7,) if error_control else None)
    dv = device_solve(m.model_id, 0, p, T_EVAL, 1e-6, atol, group, sens_atol=sa)
    ref = S.solve_ensemble(ref_id, p, T_EVAL, rtol=1e-6, atol=atol, sens_atol=sa, group=group)
    assert_same(dv, ref)
    assert np.array_equal(dv["sens"][1, :, 0, 0], np.ones(NB)) and not dv["sens"][1, :, 0, 1].any()   # x(0) = y0, y(0) = 1


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("name", ["decay", "transcendental"])
def test_outputs_and_fit_on_the_resident_buffers(H, dev, name, group):
    """3. solve_dense_sens_outputs and solve_dense_sens_fit with Tsit45: the states and sensitivities are those of solve_dense_adaptive_sens, out / dout the kernel
    applied to them, loss / grad / gn the numpy restatement on out / dout — shared and per-member data, a missing observation, weights"""
    m, tw, _ = _diffsl(name)
    p = np.random.default_rng(8).uniform(0.5, 2.0, (NB, 2)) * ([0.2, 1.0] if name == "decay" else [1.0, 1.0])
    te = T_EVAL
    s = H.Solver(m, p, nbatch=NB, method=H.METHOD_TSIT45, sens=True, sens_rtol=1e-6, sens_atol=[1e-6], **TOL)
    out, dout, tot, ys, ss = s.solve_dense_sens_outputs(te, group=group, want_states=True)
    y, sens, tot2 = s.solve_dense_adaptive_sens(te, group=group)
    assert tot["failed_members"] == 0 and tot == tot2 and tot["number_of_steps"] > 0 and tot["number_of_linear_solver_setups"] == 0
    assert np.array_equal(ys, y) and np.array_equal(ss, sens) and np.isfinite(sens).all()
    ko, kd = _kernel_on(dev, m, tw, te, y, sens, p)
    assert np.array_equal(out, ko) and np.array_equal(dout, kd) and np.abs(dout).max() > 0
    rng = np.random.default_rng(3)
    pm = out * rng.uniform(0.9, 1.1, out.shape)          # per-member data [nt, nb, nout]
    holed = pm.copy()
    holed[2, 5, 0] = np.nan                              # one missing observation
    w = rng.uniform(0.5, 2.0, (len(te), out.shape[2]))
    for data, wt in ((pm[:, 17, :], None), (pm[:, 17, :], w), (pm, None), (pm, w), (holed, w)):
        loss, grad, tot3, gn, mem = s.solve_dense_sens_fit(te, data, weights=wt, gauss_newton=True, group=group, want_member_stats=True)
        assert tot3 == tot and not mem["status"].any()
        want = F.from_solver_outputs(out, dout, data, wt, gn=True)
        for got, ref in zip((loss, grad, gn), want):
            assert np.array_equal(got, ref), (name, group, np.abs(got - ref).max())
        assert np.isfinite(gn).all() and (loss > 0).all()


@pytest.mark.parametrize("group", [1, 64])
def test_4096_members_against_the_closed_form_under_the_reference_bound(H, group):
    """4. every member: states and both sensitivities under the bound of the CPU tier (tests/test_erk_sens_ref_golden.py), the state tolerances as weights"""
    nb = 4096
    p = sweep_params(nb)
    s = H.Solver("exponential_decay", p, nbatch=nb, method=H.METHOD_TSIT45, sens=True, sens_rtol=1e-6, sens_atol=[1e-6], rtol=1e-6, atol=[1e-6])
    y, sens, tot, mem = s.solve_dense_adaptive_sens(SWEEP_T, group=group, want_member_stats=True)
    assert tot["failed_members"] == 0 and not mem["status"].any()
    norms = worst_norms(np.transpose(y, (1, 0, 2)), np.transpose(sens, (0, 2, 1, 3)), p, SWEEP_T, 1e-6, 1e-6)
    print("tsit45 + sensitivities, 4096 members, group", group, ": worst weighted error norms (y, dy/dk, dy/dy0)", norms, "steps per member", tot["number_of_steps"] / nb)
    assert max(norms) < BOUND


@pytest.mark.parametrize("group", [1, 64])
def test_members_that_do_not_finish(H, group):
    """5. max_steps = 3.  With the sensitivities out of the error control the step sequence is the plain solver's: status, counters and states equal the plain
    Tsit45 launch with the same options bit for bit.  With them in it, too: the status equals the plain solver's (nobody reaches t = 4 in three steps), the columns from
    the first one a member did not reach are NaN in y and in sens alike, the ones before equal the unrestricted run's bit for bit."""
    model = H.MODELS["exponential_decay"]
    p = sweep_params(NB, seed=21)
    plain = device_solve(model, 0, p, T_EVAL, TOL["rtol"], TOL["atol"], group, sens=False, max_steps=3)
    assert (plain["status"] == 99).all()   # MaxStepsExceeded
    for sa in (None, (1e-6,)):
        full = device_solve(model, 0, p, T_EVAL, TOL["rtol"], TOL["atol"], group, sens_atol=sa)
        cut = device_solve(model, 0, p, T_EVAL, TOL["rtol"], TOL["atol"], group, sens_atol=sa, max_steps=3)
        assert np.array_equal(cut["status"], plain["status"]) and cut["totals"][5] == NB and not full["status"].any()
        assert (cut["stats"][:, 0] == 3).all()
        reached = np.isfinite(cut["y"][:, :, 0]).sum(axis=1)   # columns a member wrote
        assert (reached >= 1).all() and (reached < len(T_EVAL)).all()
        for b in range(NB):
            r = reached[b]
            assert np.isnan(cut["y"][b, r:]).all() and np.isnan(cut["sens"][:, b, r:]).all()
            assert np.array_equal(cut["y"][b, :r], full["y"][b, :r]) and np.array_equal(cut["sens"][:, b, :r], full["sens"][:, b, :r])
        if sa is None:
            assert np.array_equal(cut["stats"], plain["stats"]) and np.array_equal(cut["y"], plain["y"], equal_nan=True)


OVER_THE_BOUND = "in = [a, b]\nu_i { x = 1, y = b, z = 0.5 }\nF_i { -a * x, -b * y, a * x - z }\nout_i { x + y + z }\n"   # 3 states, 2 parameters: 3 (14 + 24) = 114 doubles


def test_refusals_name_the_reason_and_the_alternative(H):
    """6. code -6 at creation; what keeps working"""
    from diffsol_amd import diffsl as fe
    p = [[0.1, 1.0]] * 4

    def refused(model, *needles, **kw):
        with pytest.raises(H.DiffsolHipError) as e:
            H.Solver(model, p, nbatch=4, method=H.METHOD_TSIT45, sens=True, **kw)
        msg = str(e.value)
        assert e.value.code == -6 and all(x in msg for x in needles) and all(x in msg for x in ("BDF", "TR-BDF2", "ESDIRK34")), msg

    over = fe.DiffslModel(OVER_THE_BOUND)
    assert (over.n, over.nparams) == (3, 2)
    refused(over, "sensitivities", "14 + 12", "3 states, 2 parameters (114)", rtol=1e-6, atol=[1e-6])
    H.Solver(over, p, nbatch=4, method=H.METHOD_TSIT45, rtol=1e-6, atol=[1e-6])   # without sensitivities the model is taken (n <= 8)
    stopping = fe.DiffslModel(M.DECAY + "stop_i { x - 0.5 }\n")
    refused(stopping, "sensitivities", "stop conditions", "1 root functions", **TOL)
    hybrid = fe.DiffslModel(M.DECAY + "stop_i { x - 0.5 }\nreset_i { 1.0, 1.0 }\n")
    refused(hybrid, "reset operator", **TOL)
    # an admitted model: every accepted step still comes without sensitivities, and the host-driven entries stay refused
    m, _, _ = _diffsl("decay")
    s = H.Solver(m, p, nbatch=4, method=H.METHOD_TSIT45, sens=True, sens_rtol=1e-6, sens_atol=[1e-6], **TOL)
    plain = H.Solver(m, p, nbatch=4, method=H.METHOD_TSIT45, **TOL)
    got, want = s.solve_adaptive(4.0, max_cols=64), plain.solve_adaptive(4.0, max_cols=64)
    assert len(got) == 4 and np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1], equal_nan=True) and (got[2]["ncols"] > 2).all()
    for call in (lambda: s.step(), lambda: s.interpolate_sens(1.0), lambda: s.solve(1.0), lambda: s.set_ensemble_mode(H.ENSEMBLE_LOCKSTEP)):
        with pytest.raises(H.DiffsolHipError) as e:
            call()
        assert e.value.code == -6 and "dshs_solve_dense" in str(e.value), str(e.value)
