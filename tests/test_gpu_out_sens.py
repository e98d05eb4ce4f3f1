"""Output sensitivities on the device (csrc/dsh_out_sens_kernel.hpp, dsh_model_out_sens, dshs_solve_dense_sens_out, Solver.solve_dense_sens_outputs): out_i and
d(out_i)/dp_j at every save point of every member from one launch — the reference's solve_dense_sensitivities for a model with an out_i
(crates/diffsol/src/ode_solver/sensitivities.rs:360-397: out.jac_mul(y, s_j) + out.sens_mul(y, e_j)).

The kernel is held bit for bit to the front end's own host twin (out_sens_models.HostTwin: the same expression roots, added once, no contraction on either side); the
solver entry is held bit for bit to that kernel applied to the states and sensitivities the existing entry points return (which tests/test_gpu_resident_sens.py holds
to the oracle), and to closed forms."""
import ctypes as C

import numpy as np
import pytest

import diffsl_models as D
import out_sens_models as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import diffsol_amd
    return diffsol_amd


class Dev:
    """a context of the device library with a few buffers (ctypes)"""

    def __init__(self):
        from diffsol_amd import _ffi
        self.f, self.L = _ffi, _ffi.load_device_lib()
        self.c = _ffi.vp()
        _ffi.check(self.L.dsh_ctx_create(0, None, C.byref(self.c)))
        self.bufs = []

    def up(self, a):
        a = np.ascontiguousarray(a)
        q = self.f.vp()
        self.f.check(self.L.dsh_malloc(self.c, max(a.nbytes, 8), 0, C.byref(q)))
        self.bufs.append(q)
        if a.nbytes:
            self.f.check(self.L.dsh_h2d(self.c, q, a.ctypes.data_as(self.f.vp), a.nbytes))
        return q

    def down(self, q, shape):
        a = np.empty(shape)
        self.f.check(self.L.dsh_d2h(self.c, a.ctypes.data_as(self.f.vp), q, a.nbytes))
        return a

    def out_sens(self, model_id, nout, t_cols, y, sens, p, member_cols=None):
        """dsh_model_out_sens on host arrays in the device layouts: y [ncols, n, nb], sens [np, ncols, n, nb], p [np, nb]"""
        ncols, n, nb = y.shape
        npar = p.shape[0]
        t = np.ascontiguousarray(t_cols, dtype=float)
        out, dout = self.up(np.zeros((ncols, nout, nb))), self.up(np.zeros((npar, ncols, nout, nb)))
        mc = self.up(np.ascontiguousarray(member_cols, dtype=np.int32)) if member_cols is not None else None
        self.f.check(self.L.dsh_model_out_sens(self.c, model_id, nb, ncols, t.ctypes.data_as(self.f.c_dp), self.up(y), self.up(sens), self.up(p), mc, out, dout))
        r = self.down(out, (ncols, nout, nb)), self.down(dout, (npar, ncols, nout, nb))
        self.release()
        return r

    def release(self):
        for q in self.bufs:
            self.L.dsh_free(self.c, q)
        self.bufs = []

    def close(self):
        self.release()
        self.L.dsh_ctx_destroy(self.c)


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


_models = {}


def _model(name):
    """(DiffslModel, HostTwin) of a named text, compiled once per session"""
    from diffsol_amd import diffsl as fe
    if name not in _models:
        code = {"rational": M.RATIONAL, "transcendental": M.TRANSCENDENTAL, "spm": M.spm_out(), "robertson_dae": M.ROBERTSON_DAE_OUT, "decay": M.DECAY}[name]
        _models[name] = (fe.DiffslModel(code), M.HostTwin(code))
    return _models[name]


def _inputs(name, tw, nb, ncols, seed):
    rng = np.random.default_rng(seed)
    # the battery outputs take sqrt(sn (1 - sn)) of the SURFACE value sn = 1.5 cn[m-1] - 0.5 cn[m-2]: concentrations in (0.35, 0.65) keep it in (0.2, 0.8), so the
    # root stays real (drawn in (0.2, 0.8) themselves the extrapolation leaves (0, 1): 1.5 * 0.2 - 0.5 * 0.8 < 0)
    lo, hi = (0.35, 0.65) if name == "spm" else (0.5, 2.0)
    y = rng.uniform(lo, hi, (ncols, tw.n, nb))
    sens = rng.uniform(-1.0, 1.0, (tw.np, ncols, tw.n, nb))
    p = rng.uniform(0.5, 2.0, (tw.np, nb))
    return np.linspace(0.0, 1.0, ncols), y, sens, p


@pytest.mark.parametrize("name,dims", [("rational", (2, 2, 3)), ("transcendental", (2, 2, 3)), ("spm", (42, 1, 2)), ("robertson_dae", (3, 3, 2))])
def test_kernel_equals_the_host_twin_bit_for_bit(dev, name, dims):
    """no integration involved: random states, sensitivities and parameters; one member, partial wavefronts, one past a wavefront, more than one workgroup row
    (4099 > 16 x 256); one and three columns"""
    m, tw = _model(name)
    assert (tw.n, tw.np, tw.nout) == dims and m.has_out_sens and dev.L.dsh_model_has_out_sens(m.model_id) == 1
    for nb in (1, 63, 65, 4099):
        for ncols in (1, 3):
            t, y, sens, p = _inputs(name, tw, nb, ncols, seed=nb + ncols)
            out, dout = dev.out_sens(m.model_id, tw.nout, t, y, sens, p)
            ro, rd = tw.evaluate(t, y, sens, p)
            assert np.isfinite(ro).all() and np.isfinite(rd).all() and np.abs(rd).max() > 0
            assert np.array_equal(out, ro), (name, nb, ncols, np.abs(out - ro).max())
            assert np.array_equal(dout, rd), (name, nb, ncols, np.abs(dout - rd).max())


def test_member_cols_blank_exactly_the_columns_a_member_never_produced(dev):
    m, tw = _model("rational")
    nb, ncols = 65, 3
    t, y, sens, p = _inputs("rational", tw, nb, ncols, seed=9)
    mc = np.array([3, 1, 0, 2] * 17, dtype=np.int32)[:nb]
    full_out, full_dout = dev.out_sens(m.model_id, tw.nout, t, y, sens, p)
    behind = np.arange(ncols)[:, None] >= mc[None, :]  # [ncols, nb]
    yn, sn = y.copy(), sens.copy()
    yn[np.broadcast_to(behind[:, None, :], yn.shape)] = np.nan  # what lies behind the count is not read into a surviving output
    sn[np.broadcast_to(behind[None, :, None, :], sn.shape)] = np.nan
    out, dout = dev.out_sens(m.model_id, tw.nout, t, yn, sn, p, member_cols=mc)
    assert np.array_equal(np.isnan(out), np.broadcast_to(behind[:, None, :], out.shape))
    assert np.array_equal(np.isnan(dout), np.broadcast_to(behind[None, :, None, :], dout.shape))
    keep = ~np.isnan(out)
    assert np.array_equal(out[keep], full_out[keep]) and np.array_equal(dout[~np.isnan(dout)], full_dout[~np.isnan(dout)])
    ro, rd = tw.evaluate(t, yn, sn, p, member_cols=mc)
    assert np.array_equal(out, ro, equal_nan=True) and np.array_equal(dout, rd, equal_nan=True)


def _kernel_on(dev, m, tw, te, y, sens, p):
    """dsh_model_out_sens on host results of the solver entry points: y [nt, nb, n], sens [np, nt, nb, n], p [nb, np] -> out [nt, nb, nout], dout [np, nt, nb, nout]"""
    out, dout = dev.out_sens(m.model_id, tw.nout, te, np.transpose(y, (0, 2, 1)), np.transpose(sens, (0, 1, 3, 2)), np.ascontiguousarray(np.asarray(p, dtype=float).T))
    return np.transpose(out, (0, 2, 1)), np.transpose(dout, (0, 1, 3, 2))


@pytest.mark.parametrize("group", [1, 64])
@pytest.mark.parametrize("method", ["bdf", "tr_bdf2", "esdirk34"])
def test_resident_route_end_to_end(H, dev, method, group):
    """y' = -k y, y(0) = y0 twice, out_i { x + y, k x }: 130 members, t = 0 .. 10, rtol = atol = 1e-6 with the sensitivities in the error control (the problem of
    test_gpu_resident_sens.py).  (i) out / dout are bitwise the kernel applied to what solve_dense_adaptive_sens of the same solver returns; (ii) the closed forms
    d(x+y)/dk = -2 t y0 e^{-kt}, d(x+y)/dy0 = 2 e^{-kt}, d(kx)/dk = y0 e^{-kt} (1 - kt), d(kx)/dy0 = k e^{-kt}, with twice the tolerance the existing tests grant one
    sensitivity of this problem (each output is a sum of at most two such terms with coefficients <= 1); (iii) want_states returns that solver's y and sens."""
    m, tw = _model("decay")
    k = 0.1 * (1 + np.arange(130) % 7)
    y0 = 1.0 + 0.25 * (np.arange(130) % 5)
    p = np.stack([k, y0], axis=1)
    te = [float(i) for i in range(0, 11)]
    hm = {"bdf": H.METHOD_BDF, "tr_bdf2": H.METHOD_TR_BDF2, "esdirk34": H.METHOD_ESDIRK34}[method]
    s = H.Solver(m, p, nbatch=130, method=hm, sens=True, sens_rtol=1e-6, sens_atol=[1e-6], rtol=1e-6, atol=[1e-6, 1e-6])
    out, dout, tot, ys, ss = s.solve_dense_sens_outputs(te, group=group, want_states=True)
    y, sens, tot2 = s.solve_dense_adaptive_sens(te, group=group)
    assert tot["failed_members"] == 0 and tot == tot2
    assert np.array_equal(ys, y) and np.array_equal(ss, sens)  # (iii)
    ko, kd = _kernel_on(dev, m, tw, te, y, sens, p)
    assert np.array_equal(out, ko) and np.array_equal(dout, kd)  # (i)
    out2, dout2, _ = s.solve_dense_sens_outputs(te, group=group)  # without the states: the same numbers
    assert np.array_equal(out2, out) and np.array_equal(dout2, dout)
    t = np.asarray(te)[:, None]
    e = np.exp(-k[None, :] * t)
    rtol, atol = (2e-3, 6e-5) if method == "bdf" else (4e-3, 4e-4)
    want = {(0, 0): -2 * t * y0[None, :] * e, (1, 0): 2 * e, (0, 1): y0[None, :] * e * (1 - k[None, :] * t), (1, 1): k[None, :] * e}
    for (j, o), w in want.items():
        print(method, group, "d out_%d / d p_%d: max abs error" % (o, j), np.abs(dout[j, :, :, o] - w).max())
        assert np.allclose(dout[j, :, :, o], w, rtol=rtol, atol=atol), (j, o)
    assert np.allclose(out[:, :, 0], 2 * y0[None, :] * e, rtol=rtol, atol=atol) and np.allclose(out[:, :, 1], k[None, :] * y0[None, :] * e, rtol=rtol, atol=atol)


def test_host_driven_route_end_to_end(H, dev):
    """A DAE has no device-resident integrator with sensitivities: the host-driven BDF is stepped and interpolated at the save points, the columns stay on the
    device and go through the same kernel.  Bitwise the kernel applied to states and sensitivities obtained by stepping the same solver by hand."""
    m, tw = _model("robertson_dae")
    assert m.has_mass
    p = np.array([[0.04, 1e4, 3e7]] * 4) * np.array([1.0, 1.1, 0.9, 1.2])[:, None]
    te = [0.4, 4.0, 40.0]
    kw = dict(nbatch=4, sens=True, rtol=1e-4, atol=[1e-8, 1e-6, 1e-6])
    s = H.Solver(m, p, **kw)
    out, dout, tot, ys, ss = s.solve_dense_sens_outputs(te, want_states=True)
    assert tot["failed_members"] == 0 and tot["number_of_steps"] > 0
    ref = H.Solver(m, p, **kw)
    y, sens, col = np.empty((3, 4, 3)), np.empty((3, 3, 4, 3)), 0
    ref.set_stop_time(te[-1])
    while col < 3:
        reason = ref.step()
        while col < 3 and te[col] <= ref.scalars()[0]:
            y[col], sens[:, col] = ref.interpolate(te[col]), ref.interpolate_sens(te[col])
            col += 1
        if reason == H.solver.STOP_TSTOP_REACHED:
            break
    assert col == 3
    assert np.array_equal(ys, y) and np.array_equal(ss, sens)
    ko, kd = _kernel_on(dev, m, tw, te, y, sens, p)
    assert np.array_equal(out, ko) and np.array_equal(dout, kd)
    print("|d(x + y + z)/dk_j| max:", np.abs(dout[:, :, :, 0]).max(axis=(1, 2)))  # the algebraic constraint keeps x + y + z = 1: small, its size depends on the tolerances
    assert np.abs(dout[0, :, :, 1]).max() > 0  # d(k1 x)/dk1 = x + k1 dx/dk1


def test_banded_lane_route(H, dev):
    """the battery model (n = 42) runs its sensitivities in the banded lane-per-member form; same identity as above"""
    m, tw = _model("spm")
    assert m.lane_model_id is not None
    p = np.random.default_rng(5).uniform(0.6, 1.4, (70, 1))
    # save points inside the range where the output is real: at the largest current the surface value sn = 1.5 cn[19] - 0.5 cn[18] falls from 0.72 at 360 s to 0.13 at
    # 1800 s (CPU oracle on the host twin) and is negative from about 2200 s on, where sqrt(sn (1 - sn)) is NaN
    te = [360.0, 1200.0, 1800.0]
    s = H.Solver(m, p, nbatch=70, sens=True, rtol=1e-6, atol=[1e-6])
    out, dout, tot = s.solve_dense_sens_outputs(te, group=1)
    y, sens, _ = s.solve_dense_adaptive_sens(te, group=1)
    assert tot["failed_members"] == 0
    ko, kd = _kernel_on(dev, m, tw, te, y, sens, p)
    assert np.isfinite(out).all() and np.abs(dout).max() > 0
    assert np.array_equal(out, ko) and np.array_equal(dout, kd)


def test_refusals_name_their_reason(H):
    from diffsol_amd._ffi import DiffsolHipError
    m, _ = _model("decay")
    p = [[0.1, 1.0]] * 4
    tol = dict(rtol=1e-6, atol=[1e-6, 1e-6])

    def refused(solver, pattern, te=(1.0,)):
        with pytest.raises(DiffsolHipError, match=pattern) as e:
            solver.solve_dense_sens_outputs(list(te))
        assert e.value.code == -6, e.value

    refused(H.Solver(m, p, nbatch=4, **tol), "dshs_create_sens")  # no sens=True
    refused(H.Solver("robertson_ode", [[0.04, 1e4, 3e7]] * 4, nbatch=4, model_size=1, sens=True, rtol=1e-4, atol=[1e-8, 1e-14, 1e-6]), "no out_i")  # registry model
    refused(H.Solver(m, p, nbatch=4, method=H.METHOD_TSIT45, **tol), "Tsit45")
    from diffsol_amd import diffsl as fe
    stopping = fe.DiffslModel(M.DECAY + "stop_i { x - 0.5 }\n")  # x = e^{-0.1 t} crosses 0.5 at t = 6.9
    refused(H.Solver(stopping, p, nbatch=4, sens=True, **tol), "stop condition", te=(1.0, 10.0))
