"""Device-resident Tsit45 (dsh_erk_solve_resident) against the CPU checker (tests/erk_ref): bitwise parity — states at t_eval, every per-member counter, status,
t_root, root_idx, ncols — with the portable pow on both sides (deterministic_pow), per member (group 1) and in wavefront lock-step (group 64: the checker runs each
64-member group as one batched problem); every accepted step (solve_adaptive); tstop cases; a 100 000-member ensemble against the closed form under the reference's
acceptance bound (ode_solver/mod.rs:164-167); the refusals.

dydt_y2 and gaussian_decay are run-time-sized models of the registry: neither has a static form at any size, and the Tsit45 kernel takes register-resident static
models only.  dydt_y2's right-hand side (dy/dt = a y^2) is run through a static DiffSL text of 3 states; gaussian_decay has no static size <= 4 and appears in the
refusal test only.
"""
import ctypes as C

import numpy as np
import pytest

import erk_ref as E
from helpers import ORACLE_MODEL, weighted_error_norm

pytestmark = pytest.mark.gpu

LOGISTIC = """
in = [r, k]
r { 1 } k { 1 }
u_i { y = 0.1 }
F_i { r * y * (1 - y / k) }
"""
DYDT_Y2 = """
in = [a]
a { 1 }
u_i { x = 1, z = 2, w = 0.5 }
F_i { a * x * x, a * z * z, a * w * w }
"""
OSC6 = """
in = [w]
w { 1 }
u_i { a = 1, b = 0, c = 0.5, d = 0, e = 0.25, f = 0 }
F_i { w * b, -w * a, 2 * w * d, -2 * w * c, 3 * w * f, -3 * w * e }
"""
SIZES = [1, 63, 65, 4099]


@pytest.fixture(scope="module")
def H():
    import diffsol_amd
    return diffsol_amd


@pytest.fixture(autouse=True)
def det_pow():
    E.set_det_pow(True)
    yield
    E.set_det_pow(False)


def params(model, nb, seed=3):
    rng = np.random.default_rng(seed + nb)
    if model in ("exponential_decay", "exponential_decay_with_root"):
        return np.stack([rng.uniform(0.05, 2.0, nb), rng.uniform(0.5, 5.0, nb)], axis=1)
    if model == "robertson_ode":
        return np.stack([0.04 * 2 ** rng.uniform(-1, 1, nb), 1e4 * 2 ** rng.uniform(-1, 1, nb), 3e7 * 2 ** rng.uniform(-1, 1, nb)], axis=1)
    raise KeyError(model)


CASES = {
    "exponential_decay": dict(t_eval=[0.5, 1.0, 2.5, 6.0], size=0, rtol=1e-6, atol=[1e-6, 1e-6]),
    "exponential_decay_with_root": dict(t_eval=[0.5, 1.0, 2.5, 6.0], size=0, rtol=1e-6, atol=[1e-6, 1e-6]),   # members stop when y = 0.6: at different times
    "robertson_ode": dict(t_eval=[1e-4, 1e-3, 4e-3], size=1, rtol=1e-4, atol=[1e-8, 1e-14, 1e-6]),        # short span: before the stiffness bites
}


def device_solve(H, model, size, p, t_eval, rtol, atol, group, steps_cap=0, t0=0.0, h0=1.0, options=None):
    """dsh_erk_solve_resident[_steps] through the device C ABI (per-member atol travels only there).  atol [n] or [nb, n]; options: fields of dsh_adaptive_options
    to set over the defaults."""
    from diffsol_amd import _ffi
    dev = _ffi.load_device_lib()
    c = _ffi.vp()
    _ffi.check(dev.dsh_ctx_create(0, None, C.byref(c)))
    bufs = {}
    try:
        nb, npar = p.shape
        info = [C.c_int64(), C.c_int64(), C.c_int(), C.c_int64()]
        _ffi.check(dev.dsh_model_info(model, size, C.byref(info[0]), C.byref(info[1]), C.byref(info[2]), C.byref(info[3])))
        n = info[0].value
        at = np.asarray(atol, dtype=float)
        atol_nb = nb if at.ndim == 2 else 1
        a_host = np.ascontiguousarray(at.T if at.ndim == 2 else at)   # device layout: n x nb, batch-fastest
        p_host = np.ascontiguousarray(p.T)
        cols = steps_cap if steps_cap else len(t_eval)

        def dmalloc(name, nbytes):
            q = _ffi.vp()
            _ffi.check(dev.dsh_malloc(c, nbytes, 0, C.byref(q)))
            bufs[name] = q
            return q
        for name, arr in (("p", p_host), ("atol", a_host)):
            _ffi.check(dev.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(_ffi.vp), arr.nbytes))
        dmalloc("y", 8 * cols * n * nb); dmalloc("t", 8 * max(cols, 1) * nb); dmalloc("stats", 4 * 5 * nb); dmalloc("status", 4 * nb)
        dmalloc("troot", 8 * nb); dmalloc("ridx", 4 * nb); dmalloc("ncols", 4 * nb)
        o = AdaptiveOptions()
        dev.dsh_adaptive_default_options(C.byref(o))
        o.deterministic_pow, o.group = 1, group
        for k, v in (options or {}).items():
            getattr(o, k)   # an unknown field is an error, not a new attribute
            setattr(o, k, v)
        opts = C.cast(C.pointer(o), C.c_void_p)
        tot = (C.c_int64 * 6)()
        te = np.ascontiguousarray(t_eval, dtype=float)
        if steps_cap:
            rc = dev.dsh_erk_solve_resident_steps(c, 3, model, size, nb, bufs["p"], bufs["atol"], atol_nb, rtol, t0, h0, opts, float(te[-1]), steps_cap, bufs["y"], bufs["t"],
                                                  bufs["stats"], bufs["status"], bufs["troot"], bufs["ridx"], bufs["ncols"], tot)
        else:
            rc = dev.dsh_erk_solve_resident(c, 3, model, size, nb, bufs["p"], bufs["atol"], atol_nb, rtol, t0, h0, opts, te.ctypes.data_as(_ffi.c_dp), te.size, bufs["y"],
                                            bufs["stats"], bufs["status"], bufs["troot"], bufs["ridx"], bufs["ncols"], tot)
        _ffi.check(rc)

        def fetch(name, shape, dtype):
            a = np.empty(shape, dtype=dtype)
            _ffi.check(dev.dsh_d2h(c, a.ctypes.data_as(_ffi.vp), bufs[name], a.nbytes))
            return a
        y = fetch("y", (cols, n, nb), np.float64).transpose(2, 0, 1)   # -> [nb, cols, n]
        out = dict(y=y, stats=fetch("stats", (5, nb), np.int32).T, status=fetch("status", (nb,), np.int32), t_root=fetch("troot", (nb,), np.float64),
                   root_idx=fetch("ridx", (nb,), np.int32), ncols=fetch("ncols", (nb,), np.int32), totals=[int(v) for v in tot])
        if steps_cap:  # only the first ncols[b] columns of member b are written (the buffers are not initialised): blank the rest like the checker's
            out["t"] = fetch("t", (cols, nb), np.float64).T.copy()
            out["y"] = y = y.copy()
            for b in range(nb):
                y[b, out["ncols"][b]:] = np.nan
                out["t"][b, out["ncols"][b]:] = np.nan
        return out
    finally:
        for q in bufs.values():
            dev.dsh_free(c, q)
        dev.dsh_ctx_destroy(c)


class AdaptiveOptions(C.Structure):
    """dsh_adaptive_options (include/diffsol_hip.h)"""
    _fields_ = ([(k, C.c_int) for k in ("max_nonlinear_solver_iterations", "max_error_test_failures", "max_nonlinear_solver_failures")] +
                [(k, C.c_double) for k in ("nonlinear_solver_tolerance", "min_timestep", "max_timestep_growth", "min_timestep_growth", "max_timestep_shrink", "min_timestep_shrink")] +
                [(k, C.c_int) for k in ("update_jacobian_after_steps", "update_rhs_jacobian_after_steps")] +
                [(k, C.c_double) for k in ("threshold_to_update_jacobian", "threshold_to_update_rhs_jacobian", "pi_control_proportional", "pi_control_integral")] +
                [(k, C.c_int) for k in ("ic_use_linesearch", "ic_max_linesearch_iterations", "ic_max_linear_solver_setups", "ic_max_newton_iterations")] +
                [(k, C.c_double) for k in ("ic_step_reduction_factor", "ic_armijo_constant")] + [("max_steps", C.c_int64), ("deterministic_pow", C.c_int), ("group", C.c_int)])


def assert_same(dev, ref, steps=False):
    assert ref["failed"] == 0 and (dev["status"] == 0).all() and (ref["status"] == 0).all()
    assert np.array_equal(dev["stats"], ref["stats"])
    assert np.array_equal(dev["ncols"], ref["ncols"]) and np.array_equal(dev["root_idx"], ref["root_idx"])
    assert np.array_equal(dev["t_root"], ref["t_root"], equal_nan=True)
    assert np.array_equal(dev["y"], ref["y"], equal_nan=True), f"max |diff| {np.nanmax(np.abs(dev['y'] - ref['y']))}"
    if steps:
        assert np.array_equal(dev["t"], ref["t"], equal_nan=True)
    assert dev["totals"][0] == int(dev["stats"][:, 0].sum()) and dev["totals"][3] == int(dev["stats"][:, 3].sum()) and dev["totals"][5] == 0


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("per_member_atol", [False, True])
@pytest.mark.parametrize("nb", SIZES)
@pytest.mark.parametrize("model", list(CASES))
def test_bitwise_parity_with_the_checker(H, model, nb, per_member_atol, group):
    cs = CASES[model]
    if model == "exponential_decay_with_root" and group == 64:
        # the members of a wavefront must agree on the crossing (status 20 otherwise): one parameter set per group
        p = np.repeat(params(model, (nb + 63) // 64), 64, axis=0)[:nb]
    else:
        p = params(model, nb)
    atol = np.asarray(cs["atol"])
    if per_member_atol:
        f = 10.0 ** np.random.default_rng(nb).uniform(-1, 1, (nb, 1))
        if group == 64 and model == "exponential_decay_with_root":
            f = np.repeat(f[: (nb + 63) // 64], 64, axis=0)[:nb]
        atol = atol[None, :] * f
    dev = device_solve(H, H.MODELS[model], cs["size"], p, cs["t_eval"], cs["rtol"], atol, group)
    ref = E.solve_ensemble(ORACLE_MODEL[model], p, cs["t_eval"], model_size=cs["size"], rtol=cs["rtol"], atol=atol, group=group)
    assert_same(dev, ref)
    if model == "exponential_decay_with_root" and nb > 1 and group == 1:
        assert (dev["root_idx"] == 0).any() and len(np.unique(dev["t_root"][dev["root_idx"] == 0])) > 1   # per-member events: different stop times
    if group == 1 and nb > 64:
        assert dev["stats"][:, 0].min() < dev["stats"][:, 0].max()


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("name,code,nparam,t_eval", [("logistic", LOGISTIC, 2, [0.5, 2.0, 8.0]), ("dydt_y2", DYDT_Y2, 1, [0.05, 0.1, 0.2]), ("oscillators6", OSC6, 1, [0.5, 3.0])])
@pytest.mark.parametrize("nb", [1, 65, 4099])
def test_diffsl_models_through_the_runtime_compiled_kernel(H, name, code, nparam, t_eval, nb, group):
    """static DiffSL models through jit_launch: n = 1 (logistic), n = 3 (dydt_y2's right-hand side) and n = 6 (5 <= n <= 8 stays register-resident)"""
    import diffsl_models as DM
    from diffsol_amd import diffsl
    m = diffsl.DiffslModel(code)
    so, _ = DM.host_model_so(code)
    ref_id = E.load_external_model(so)
    rng = np.random.default_rng(nb)
    p = rng.uniform(0.5, 1.5, (nb, nparam)) if name != "logistic" else np.stack([rng.uniform(0.5, 2.0, nb), rng.uniform(0.5, 3.0, nb)], axis=1)
    atol = [1e-8] * m.n
    dev = device_solve(H, m.model_id, 0, p, t_eval, 1e-6, atol, group)
    ref = E.solve_ensemble(ref_id, p, t_eval, rtol=1e-6, atol=atol, group=group)
    assert_same(dev, ref)


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("model", ["exponential_decay", "exponential_decay_with_root"])
def test_solve_adaptive_every_accepted_step_and_the_max_cols_protocol(H, model, group):
    nb = 200
    p = params(model, nb) if group == 1 else np.repeat(params(model, 4), 64, axis=0)[:nb]
    cs = CASES[model]
    dev = device_solve(H, H.MODELS[model], 0, p, [6.0], cs["rtol"], cs["atol"], group, steps_cap=64)
    ref = E.solve_ensemble(ORACLE_MODEL[model], p, [6.0], rtol=cs["rtol"], atol=cs["atol"], group=group, steps_cap=64)
    assert_same(dev, ref, steps=True)
    assert (dev["ncols"] == dev["stats"][:, 0] + 1).all() and dev["ncols"].max() <= 64   # (t0, y0) + one column per accepted step (the last one moved back to the root)
    # ncols > max_cols: counted, not stored — as for SDIRK
    small = device_solve(H, H.MODELS[model], 0, p, [6.0], cs["rtol"], cs["atol"], group, steps_cap=3)
    assert np.array_equal(small["ncols"], dev["ncols"]) and (small["ncols"] > 3).any()
    assert np.array_equal(small["y"], dev["y"][:, :3], equal_nan=True) and np.array_equal(small["t"], dev["t"][:, :3], equal_nan=True)
    # the Python surface gives the same columns
    s = H.Solver(model, p, nbatch=nb, method=H.METHOD_TSIT45, rtol=cs["rtol"], atol=cs["atol"])
    y, t, mem, tot = s.solve_adaptive(6.0, max_cols=64, group=group)
    for b in range(nb):  # member b's solution is y[:ncols[b], b], t[:ncols[b], b]
        y[mem["ncols"][b]:, b] = np.nan
        t[mem["ncols"][b]:, b] = np.nan
    assert np.array_equal(mem["ncols"], dev["ncols"]) and np.array_equal(np.transpose(y, (1, 0, 2)), dev["y"], equal_nan=True) and np.array_equal(t.T, dev["t"], equal_nan=True)


def test_tstop_inside_a_step_and_at_a_step_boundary(H):
    """test_tstop_tsit45's situations: a stop time the controller's step would overshoot (the step is cut: handle_tstop), and one that coincides with the end of an
    accepted step (found from the step times of a first run): the last column is state.y at tstop in both, equal to the checker's bit for bit"""
    p = np.array([[0.1, 1.0]])
    kw = dict(rtol=1e-6, atol=[1e-6, 1e-6])
    free = device_solve(H, H.MODELS["exponential_decay"], 0, p, [10.0], group=1, steps_cap=64, **kw)
    ts = free["t"][0, : free["ncols"][0]]
    for tstop in (0.5 * (ts[3] + ts[4]), float(ts[4])):
        dev = device_solve(H, H.MODELS["exponential_decay"], 0, p, [tstop], group=1, steps_cap=64, **kw)
        ref = E.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, [tstop], group=1, steps_cap=64, **kw)
        assert_same(dev, ref, steps=True)
        assert dev["t"][0, dev["ncols"][0] - 1] == tstop
        dense = device_solve(H, H.MODELS["exponential_decay"], 0, p, [tstop], group=1, **kw)
        assert_same(dense, E.solve_ensemble(ORACLE_MODEL["exponential_decay"], p, [tstop], group=1, **kw))  # solve_dense interpolates at tstop (theta = 1): the checker's bits
        assert weighted_error_norm(dense["y"][0, 0], np.full(2, np.exp(-0.1 * tstop)), [1e-6], 1e-6) < 20.0


def test_100000_members_against_the_closed_form_under_the_reference_bound(H):
    """every member of a 100 000-member exponential-decay sweep, none left out: weighted error norm below 20 (test_ode_solver's bound) at every save point"""
    nb = 100_000
    rng = np.random.default_rng(7)
    p = np.stack([rng.uniform(0.05, 2.0, nb), rng.uniform(0.5, 5.0, nb)], axis=1)
    t = np.array([0.5, 1.0, 2.0, 4.0])
    s = H.Solver("exponential_decay", p, nbatch=nb, method=H.METHOD_TSIT45, rtol=1e-6, atol=[1e-6])
    y, reason = s.solve_dense(t)                       # ensemble mode auto -> wavefront groups, [nt, nb, n]
    mode, tot = s.last_solve_info()
    assert mode == H.ENSEMBLE_WAVEFRONT and tot["failed_members"] == 0 and reason == 2
    exact = p[None, :, 1:2] * np.exp(-p[None, :, 0:1] * t[:, None, None]) * np.ones((1, 1, 2))
    e = (y - exact) / (np.abs(exact) * 1e-6 + 1e-6)
    norms = np.sqrt(np.mean(e * e, axis=2))
    print("tsit45, 100000 members, wavefront groups: max weighted error norm", norms.max())
    assert norms.max() < 20.0
    y1, tot1, mem = s.solve_dense_adaptive(t, want_member_stats=True, group=1)
    n1 = np.sqrt(np.mean(((y1 - exact) / (np.abs(exact) * 1e-6 + 1e-6)) ** 2, axis=2))
    print("tsit45, 100000 members, per member: max weighted error norm", n1.max(), "steps per member", tot1["number_of_steps"] / nb)
    assert (mem["status"] == 0).all() and n1.max() < 20.0


def test_refusals_say_what_to_use_instead(H):
    from diffsol_amd import _ffi
    dev = _ffi.load_device_lib()

    def nparams(model, size):
        n, npar, hm, nr = C.c_int64(), C.c_int64(), C.c_int(), C.c_int64()
        _ffi.check(dev.dsh_model_info(H.MODELS[model], size, C.byref(n), C.byref(npar), C.byref(hm), C.byref(nr)))
        return int(npar.value)
    for model, size, extra, needle in (("robertson", 0, {}, "MassMatrixNotSupported"), ("spm", 20, {}, "n > 8"),("heat1d", 20, {}, "n > 8"),
                                       ("robertson_ode", 4, {}, "n > 8"), ("robertson_ode", 1, dict(sens=True), "sensitivities")):
        with pytest.raises(H.DiffsolHipError) as e:
            H.Solver(model, [[1.0] * nparams(model, size)], nbatch=1, model_size=size, method=H.METHOD_TSIT45, **extra)
        assert e.value.code == -6 and needle in str(e.value) and "BDF" in str(e.value), str(e.value)
    import diffsl_models as DM
    from diffsol_amd import diffsl
    dae = diffsl.DiffslModel(DM.spm_dae(20))   # the battery model as a DAE (the built-in spm is its 42-state ODE form)
    with pytest.raises(H.DiffsolHipError) as e:
        H.Solver(dae, None, nbatch=1, method=H.METHOD_TSIT45)
    assert e.value.code == -6 and "MassMatrixNotSupported" in str(e.value) and "BDF" in str(e.value), str(e.value)
    s = H.Solver("exponential_decay", [[0.1, 1.0]], nbatch=1, method=H.METHOD_TSIT45)
    for call in (lambda: s.step(), lambda: s.solve(1.0), lambda: s.set_ensemble_mode(H.ENSEMBLE_LOCKSTEP), lambda: s.solve_to_points([1.0])):
        with pytest.raises(H.DiffsolHipError) as e:
            call()
        assert e.value.code == -6 and "dshs_solve_dense" in str(e.value) and "dshs_solve_adaptive" in str(e.value)
    y, _ = s.solve_dense([1.0])   # and the modes that work, work
    assert weighted_error_norm(y[0, 0], np.full(2, np.exp(-0.1)), [1e-6], 1e-6) < 20.0
    assert dev.dsh_model_has_resident(3, H.MODELS["gaussian_decay"], 4) == 0   # run-time sized: no static form
