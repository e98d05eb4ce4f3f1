"""Device-resident Tsit45 with the output equations integrated (dsh_erk_solve_resident_out / _steps_out, Solver(integrate_out=True)) against the CPU checker
(tests/erk_out_ref): g = integral of out(y, t) at t_eval and after every accepted step, every per-member counter, status, t_root, root_idx and ncols bit for bit, with the
portable pow on both sides, per member (group 1) and in wavefront lock-step (group 64), shared and per-member atol, output tolerances off and on; the Python surface;
the refusals."""
import ctypes as C

import numpy as np
import pytest

import erk_out_ref as EO
from helpers import ORACLE_MODEL
from test_gpu_erk import AdaptiveOptions

pytestmark = pytest.mark.gpu

# 3 states, one nonlinear output that reads the time: a wrong stage time or stage point shows in g
OSC_OUT = """
in = [w]
w { 1 }
u_i { x = 1, y = 0, z = 0.5 }
F_i { w * y, -w * x, -0.3 * z + 0.1 * x }
out_i { x * y + t }
"""
# more outputs than states
TWO_THREE = """
in = [k, c]
k { 1 } c { 1 }
u_i { x = 1, y = 0 }
F_i { -k * x, k * x - c * y }
out_i { x, y, x * y + c }
"""
EIGHT = """
in = [w]
w { 1 }
u_i { a = 1, b = 0, c = 0.5, d = 0, e = 0.25, f = 0, g = 1, h = 2 }
F_i { w * b, -w * a, 2 * w * d, -2 * w * c, 3 * w * f, -3 * w * e, -g, -h }
out_i { a }
"""
T_EVAL = [0.0, 0.5, 1.0, 2.5, 6.0]
RTOL = 1e-6
OUT_RTOL, OUT_ATOL = 1e-9, 1e-11


@pytest.fixture(scope="module")
def H():
    import diffsol_amd
    return diffsol_amd


@pytest.fixture(autouse=True)
def det_pow():
    EO.set_det_pow(True)
    yield
    EO.set_det_pow(False)


_models = {}


def model_of(H, name):
    """(device model id, size, checker model id, n, nout, number of parameters); DiffSL texts are compiled once per session"""
    if name in ("exponential_decay", "exponential_decay_with_root"):
        return H.MODELS[name], 0, ORACLE_MODEL[name], 2, 2, 2
    if name not in _models:
        import diffsl_models as DM
        from diffsol_amd import diffsl
        code = {"osc_out": OSC_OUT, "two_three": TWO_THREE}[name]
        m = diffsl.DiffslModel(code)
        so, _ = DM.host_model_so(code)
        _models[name] = (m, EO.load_external_model(so))
    m, ref = _models[name]
    return m.model_id, 0, ref, m.n, EO.model_dims(ref)["nout"], {"osc_out": 1, "two_three": 2}[name]


def params(name, nb, group):
    def draw(k):
        rng = np.random.default_rng(17 + k)
        if name.startswith("exponential_decay"):
            return np.stack([rng.uniform(0.05, 2.0, k), rng.uniform(0.5, 5.0, k)], axis=1)
        if name == "osc_out":
            return rng.uniform(0.5, 1.5, (k, 1))
        return np.stack([rng.uniform(0.3, 2.0, k), rng.uniform(0.3, 2.0, k)], axis=1)
    if name == "exponential_decay_with_root" and group == 64:   # the members of a wavefront must agree on the crossing (status 20 otherwise): one parameter set per group
        return np.repeat(draw((nb + 63) // 64), 64, axis=0)[:nb]
    return draw(nb)


def device_solve(model, size, nout, p, t_eval, rtol, atol, group, out_rtol=0.0, out_atol=None, steps_cap=0, expect=None, t0=0.0, h0=1.0, options=None):
    """dsh_erk_solve_resident_out / _steps_out through the device C ABI.  atol [n] or [nb, n]; out_atol None (outside the error test) or a list.  expect: the error code
    the call must return (the message comes back instead of the arrays).  options: fields of dsh_adaptive_options to set over the defaults."""
    from diffsol_amd import _ffi
    dev = _ffi.load_device_lib()
    c = _ffi.vp()
    _ffi.check(dev.dsh_ctx_create(0, None, C.byref(c)))
    bufs = {}
    try:
        nb = p.shape[0]
        at = np.asarray(atol, dtype=float)
        atol_nb = nb if at.ndim == 2 else 1
        a_host = np.ascontiguousarray(at.T if at.ndim == 2 else at)
        p_host = np.ascontiguousarray(p.T)
        cols = steps_cap if steps_cap else len(t_eval)

        def dmalloc(name, nbytes):
            q = _ffi.vp()
            _ffi.check(dev.dsh_malloc(c, nbytes, 0, C.byref(q)))
            bufs[name] = q
            return q
        for name, arr in (("p", p_host), ("atol", a_host)):
            _ffi.check(dev.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(_ffi.vp), arr.nbytes))
        dmalloc("y", 8 * cols * max(nout, 1) * nb); dmalloc("t", 8 * max(cols, 1) * nb); dmalloc("stats", 4 * 5 * nb); dmalloc("status", 4 * nb)
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
        oa = np.ascontiguousarray(np.zeros(1) if out_atol is None else np.asarray(out_atol, dtype=float).reshape(-1))
        noa = 0 if out_atol is None else oa.size
        if steps_cap:
            rc = dev.dsh_erk_solve_resident_steps_out(c, 3, model, size, nb, bufs["p"], bufs["atol"], atol_nb, rtol, t0, h0, opts, float(te[-1]), steps_cap, out_rtol,
                                                      oa.ctypes.data_as(_ffi.c_dp), noa, bufs["y"], bufs["t"], bufs["stats"], bufs["status"], bufs["troot"], bufs["ridx"],
                                                      bufs["ncols"], tot)
        else:
            rc = dev.dsh_erk_solve_resident_out(c, 3, model, size, nb, bufs["p"], bufs["atol"], atol_nb, rtol, t0, h0, opts, te.ctypes.data_as(_ffi.c_dp), te.size, out_rtol,
                                                oa.ctypes.data_as(_ffi.c_dp), noa, bufs["y"], bufs["stats"], bufs["status"], bufs["troot"], bufs["ridx"], bufs["ncols"], tot)
        if expect is not None:
            assert rc == expect, (rc, dev.dsh_last_error())
            return (dev.dsh_last_error() or b"").decode()
        _ffi.check(rc)

        def fetch(name, shape, dtype):
            a = np.empty(shape, dtype=dtype)
            _ffi.check(dev.dsh_d2h(c, a.ctypes.data_as(_ffi.vp), bufs[name], a.nbytes))
            return a
        g = fetch("y", (cols, nout, nb), np.float64).transpose(2, 0, 1).copy()   # -> [nb, cols, nout]
        out = dict(g=g, stats=fetch("stats", (5, nb), np.int32).T, status=fetch("status", (nb,), np.int32), t_root=fetch("troot", (nb,), np.float64),
                   root_idx=fetch("ridx", (nb,), np.int32), ncols=fetch("ncols", (nb,), np.int32), totals=[int(v) for v in tot])
        if steps_cap:  # only the first ncols[b] columns of member b are written: blank the rest like the checker's
            out["t"] = fetch("t", (cols, nb), np.float64).T.copy()
            for b in range(nb):
                g[b, out["ncols"][b]:] = np.nan
                out["t"][b, out["ncols"][b]:] = np.nan
        return out
    finally:
        for q in bufs.values():
            dev.dsh_free(c, q)
        dev.dsh_ctx_destroy(c)


def assert_same(dev, ref, steps=False):
    assert ref["failed"] == 0 and (dev["status"] == 0).all() and (ref["status"] == 0).all()
    assert np.array_equal(dev["stats"], ref["stats"])
    assert np.array_equal(dev["ncols"], ref["ncols"]) and np.array_equal(dev["root_idx"], ref["root_idx"])
    assert np.array_equal(dev["t_root"], ref["t_root"], equal_nan=True)
    assert np.array_equal(dev["g"], ref["g"], equal_nan=True), f"max |diff| {np.nanmax(np.abs(dev['g'] - ref['g']))}"
    if steps:
        assert np.array_equal(dev["t"], ref["t"], equal_nan=True)
    assert dev["totals"][0] == int(dev["stats"][:, 0].sum()) and dev["totals"][3] == int(dev["stats"][:, 3].sum()) and dev["totals"][5] == 0


def atol_of(n, nb, per_member, name, group):
    base = np.full(n, 1e-8) if name in ("osc_out", "two_three") else np.full(n, 1e-6)
    if not per_member:
        return base
    f = 10.0 ** np.random.default_rng(nb).uniform(-1, 1, (nb, 1))
    if group == 64 and name == "exponential_decay_with_root":
        f = np.repeat(f[: (nb + 63) // 64], 64, axis=0)[:nb]
    return base[None, :] * f


@pytest.mark.parametrize("out_tol", [False, True], ids=["no_out_tol", "out_tol"])
@pytest.mark.parametrize("per_member_atol", [False, True], ids=["shared_atol", "member_atol"])
@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("nb", [1, 65, 130])
@pytest.mark.parametrize("name", ["exponential_decay", "exponential_decay_with_root", "osc_out", "two_three"])
def test_bitwise_parity_with_the_checker(H, name, nb, group, per_member_atol, out_tol):
    model, size, ref_id, n, nout, _ = model_of(H, name)
    p = params(name, nb, group)
    atol = atol_of(n, nb, per_member_atol, name, group)
    kw = dict(out_rtol=OUT_RTOL, out_atol=([OUT_ATOL] if nout != 3 else [OUT_ATOL, 2 * OUT_ATOL, 5 * OUT_ATOL])) if out_tol else {}
    dev = device_solve(model, size, nout, p, T_EVAL, RTOL, atol, group, **kw)
    ref = EO.solve_ensemble(ref_id, p, T_EVAL, rtol=RTOL, atol=atol, group=group, **kw)
    assert_same(dev, ref)
    assert np.array_equal(dev["g"][:, 0], np.zeros((nb, nout)))   # t_eval[0] = t0: the integral starts at zero
    if name == "exponential_decay_with_root":
        assert (dev["root_idx"] == 0).any() and np.array_equal(dev["ncols"] < len(T_EVAL), dev["t_root"] < T_EVAL[-2])
        for b in range(nb):
            assert np.isnan(dev["g"][b, dev["ncols"][b]:]).all() and not np.isnan(dev["g"][b, : dev["ncols"][b]]).any()
    if out_tol:   # the output tolerances decide the step size: more steps than the plain run
        plain = EO.solve_ensemble(ref_id, p, T_EVAL, rtol=RTOL, atol=atol, group=group)
        assert dev["stats"][:, 0].sum() > plain["stats"][:, 0].sum()


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("name", ["exponential_decay", "exponential_decay_with_root", "osc_out"])
def test_every_accepted_step_the_zero_first_column_and_the_max_cols_protocol(H, name, group):
    model, size, ref_id, n, nout, _ = model_of(H, name)
    nb = 130
    p = params(name, nb, group)
    atol = atol_of(n, nb, False, name, group)
    dev = device_solve(model, size, nout, p, [6.0], RTOL, atol, group, steps_cap=96)
    ref = EO.solve_ensemble(ref_id, p, [6.0], rtol=RTOL, atol=atol, group=group, steps_cap=96)
    assert_same(dev, ref, steps=True)
    assert (dev["ncols"] == dev["stats"][:, 0] + 1).all() and dev["ncols"].max() <= 96
    assert np.array_equal(dev["g"][:, 0], np.zeros((nb, nout))) and (dev["t"][:, 0] == 0.0).all()   # write_out before the first step: g(t0) = 0
    if name == "exponential_decay_with_root":   # the last column is g at the root
        hit, last = dev["root_idx"] == 0, dev["ncols"] - 1
        assert hit.any() and np.array_equal(dev["t"][hit, last[hit]], dev["t_root"][hit])
        dense = device_solve(model, size, nout, p, [0.0, 6.0], RTOL, atol, group)   # the same steps; no save point between t0 and the root: column 1 is the root's
        assert np.array_equal(dense["g"][hit, 1], dev["g"][hit, last[hit]]) and (dense["ncols"] == 2).all() and np.array_equal(dense["t_root"], dev["t_root"], equal_nan=True)
    small = device_solve(model, size, nout, p, [6.0], RTOL, atol, group, steps_cap=3)   # ncols > max_cols: counted, not stored
    assert np.array_equal(small["ncols"], dev["ncols"]) and (small["ncols"] > 3).any()
    assert np.array_equal(small["g"], dev["g"][:, :3], equal_nan=True) and np.array_equal(small["t"], dev["t"][:, :3], equal_nan=True)


@pytest.mark.parametrize("name", ["exponential_decay", "two_three"])
def test_the_python_surface_returns_the_c_entry_arrays_and_leaves_the_plain_solver_alone(H, name):
    model, size, ref_id, n, nout, _ = model_of(H, name)
    nb = 130
    p = params(name, nb, 1)
    atol = atol_of(n, nb, False, name, 1)
    what = name if name in H.MODELS else _models[name][0]
    before = H.Solver(what, p, nbatch=nb, method=H.METHOD_TSIT45, rtol=RTOL, atol=atol)
    y0, _, m0 = before.solve_dense_adaptive(T_EVAL, want_member_stats=True, group=1)
    for out_atol in (None, [OUT_ATOL]):
        kw = {} if out_atol is None else dict(out_rtol=OUT_RTOL, out_atol=out_atol)
        dev = device_solve(model, size, nout, p, T_EVAL, RTOL, atol, 1, **kw)
        s = H.Solver(what, p, nbatch=nb, method=H.METHOD_TSIT45, rtol=RTOL, atol=atol, integrate_out=True, **kw)
        assert s.nout == nout and s.n == n
        g, tot, mem = s.solve_dense_adaptive(T_EVAL, want_member_stats=True, group=1)
        assert g.shape == (len(T_EVAL), nb, nout)
        assert np.array_equal(np.transpose(g, (1, 0, 2)), dev["g"], equal_nan=True) and np.array_equal(mem["stats"].T, dev["stats"]) and np.array_equal(mem["ncols"], dev["ncols"])
        if out_atol is None:   # no output tolerances: the step sequence is the plain solve's
            assert np.array_equal(mem["stats"], m0["stats"])
        steps = device_solve(model, size, nout, p, [6.0], RTOL, atol, 1, steps_cap=96, **kw)
        gs, ts, ms, _ = s.solve_adaptive(6.0, max_cols=96, group=1)
        for b in range(nb):
            gs[ms["ncols"][b]:, b] = np.nan
            ts[ms["ncols"][b]:, b] = np.nan
        assert np.array_equal(np.transpose(gs, (1, 0, 2)), steps["g"], equal_nan=True) and np.array_equal(ts.T, steps["t"], equal_nan=True)
        gd, reason = s.solve_dense(T_EVAL)   # auto mode: wavefront groups
        wave = device_solve(model, size, nout, p, T_EVAL, RTOL, atol, 64, **kw)
        assert reason == 2 and np.array_equal(np.transpose(gd, (1, 0, 2)), wave["g"], equal_nan=True)
    # the builder spells the same solver
    b = H.OdeBuilder().model(what).p(p).nbatch(nb).rtol(RTOL).atol(atol).integrate_out(True).out_rtol(OUT_RTOL).out_atol(OUT_ATOL).tsit45()
    gb, _ = b.solve_dense_adaptive(T_EVAL, group=1)
    assert np.array_equal(gb, g)
    # a second solver of the same model with the flag off, and the first after the flag solvers ran: the states as before
    after = H.Solver(what, p, nbatch=nb, method=H.METHOD_TSIT45, rtol=RTOL, atol=atol)
    y1, _, m1 = after.solve_dense_adaptive(T_EVAL, want_member_stats=True, group=1)
    y2, _ = before.solve_dense_adaptive(T_EVAL, group=1)
    assert after.nout == n and np.array_equal(y1, y0) and np.array_equal(y2, y0) and np.array_equal(m1["stats"], m0["stats"])
    s.set_integrate_out(False)
    y3, _ = s.solve_dense_adaptive(T_EVAL, group=1)
    assert s.nout == n and np.array_equal(y3, y0)


def test_refusals_name_what_is_supported(H):
    from diffsol_amd import _ffi, diffsl
    dev = _ffi.load_device_lib()
    p = [[0.1, 1.0]]
    with pytest.raises(H.DiffsolHipError) as e:   # a BDF solver
        H.Solver("exponential_decay", p, nbatch=1, method=H.METHOD_BDF, integrate_out=True)
    assert e.value.code == -6 and "BDF" in str(e.value) and "Tsit45" in str(e.value) and "append the integral as a state" in str(e.value), str(e.value)
    with pytest.raises(H.DiffsolHipError) as e:   # Tsit45 with forward sensitivities
        H.Solver("exponential_decay", p, nbatch=1, method=H.METHOD_TSIT45, sens=True, integrate_out=True)
    assert e.value.code == -6 and "sensitivities" in str(e.value) and "not combined" in str(e.value), str(e.value)
    eight = diffsl.DiffslModel(EIGHT)                # 14 * 8 + 12 * 1 = 124 > 112
    assert dev.dsh_model_has_resident(3, eight.model_id, 0) == 1 and dev.dsh_erk_model_has_out_integral(eight.model_id, 0) == 0 and dev.dsh_erk_model_nout(eight.model_id, 0) == 1
    with pytest.raises(H.DiffsolHipError) as e:
        H.Solver(eight, None, nbatch=1, method=H.METHOD_TSIT45, integrate_out=True)
    assert e.value.code == -6 and "8 states and 1 outputs (124 doubles" in str(e.value) and "<= 112" in str(e.value) and "BDF" in str(e.value), str(e.value)
    msg = device_solve(eight.model_id, 0, 1, np.array([[1.0]]), [1.0], RTOL, [1e-8] * 8, 1, expect=-6)
    assert "8 states and 1 outputs (124 doubles)" in msg and "<= 112" in msg and "BDF" in msg, msg
    H.Solver(eight, None, nbatch=1, method=H.METHOD_TSIT45).solve_dense([1.0])   # the plain solve takes it
    with pytest.raises(H.DiffsolHipError) as e:   # out_atol of a wrong length
        H.Solver("exponential_decay", p, nbatch=1, method=H.METHOD_TSIT45, integrate_out=True, out_rtol=1e-8, out_atol=[1e-8, 1e-8, 1e-8])
    assert e.value.code == -1 and "out_atol must have length 1 or nout (2 for this model)" in str(e.value) and "got 3" in str(e.value), str(e.value)
    msg = device_solve(H.MODELS["exponential_decay"], 0, 2, np.array(p), [1.0], RTOL, [1e-6, 1e-6], 1, out_rtol=1e-8, out_atol=[1e-8] * 3, expect=-1)
    assert "out_atol must have length 1 or nout (2 for this model)" in msg and "got 3" in msg, msg
    assert dev.dsh_erk_model_has_out_integral(H.MODELS["exponential_decay_with_root"], 0) == 1   # root functions are allowed
    assert dev.dsh_erk_model_has_out_integral(H.MODELS["robertson"], 0) == 0                      # mass matrix: no Tsit45 at all
