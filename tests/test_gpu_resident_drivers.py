"""The host drivers of the device-resident integrators (dsh_bdf_solve_adaptive, dsh_sdirk_solve_resident, dsh_erk_solve_resident) through the device C ABI: what
the drivers decide between the arguments and the launch, held to properties that need no stored numbers.

  * the constants cache of the BDF driver: a repeated call (cache hit after miss) gives the same bits, a call with another rtol in between gives others and the first
    call repeated gives the first bits again (miss, miss); save points kept in the context's block (n_eval = 3) against save points uploaded per call (n_eval = 513:
    more than 4096 bytes) agree bit for bit in the columns they share;
  * both BA forms: atol broadcast against the same atol given per member, bit for bit, for BDF, TR-BDF2, ESDIRK34 and Tsit45, at 65 members (one full wavefront plus
    one lane: the grid's tail) and at 1;
  * a call the host refuses — DSH_E_INVALID for decreasing save points, DSH_E_UNSUPPORTED for Tsit45 on a model with a mass matrix — leaves the context usable and
    the next solve unchanged.  These are argument errors returned by the host: nothing is launched.

Robertson (n = 3, register-resident); Tsit45 over a short span, before the stiffness bites (as tests/test_gpu_erk.py)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_erk import AdaptiveOptions

pytestmark = pytest.mark.gpu

ROBERTSON_ODE, ROBERTSON_DAE, MODEL_SIZE, N = 3, 4, 1, 3  # diffsol_amd.MODELS["robertson_ode"], ["robertson"] (the same system with a mass matrix)
BDF, TR_BDF2, ESDIRK34, TSIT45 = 0, 1, 2, 3
RTOL, ATOL = 1e-4, [1e-8, 1e-14, 1e-6]
T_STIFF, T_SHORT = [0.4, 4.0, 40.0], [1e-4, 1e-3, 4e-3]
DSH_E_INVALID, DSH_E_UNSUPPORTED = -1, -6
NB = 65
KEYS = ("y", "stats", "status", "t_root", "root_idx", "ncols", "totals")


def params(nb):
    rng = np.random.default_rng(2024 + nb)
    return np.stack([0.04 * 2 ** rng.uniform(-1, 1, nb), 1e4 * 2 ** rng.uniform(-1, 1, nb), 3e7 * 2 ** rng.uniform(-1, 1, nb)], axis=1)


def t_eval_of(method):
    return T_SHORT if method == TSIT45 else T_STIFF


class Device:
    """one context for a sequence of solves: what one call leaves behind (the cached constants, the parked blocks) is what the next one meets"""

    def __init__(self):
        from diffsol_amd import _ffi
        self.ffi, self.dev, self.c = _ffi, _ffi.load_device_lib(), _ffi.vp()
        _ffi.check(self.dev.dsh_ctx_create(0, None, C.byref(self.c)))

    def close(self):
        self.dev.dsh_ctx_destroy(self.c)

    def solve(self, method, p, t_eval, rtol=RTOL, per_member_atol=False, group=1, model=ROBERTSON_ODE):
        """returns (return code, dict of y [n_eval, N, nb], stats [5, nb], status, t_root, root_idx, ncols [nb], totals [6]); the dict is None for a refused call"""
        ffi, dev, c = self.ffi, self.dev, self.c
        p = np.asarray(p, dtype=float)
        nb, te = len(p), np.ascontiguousarray(t_eval, dtype=float)
        atol = np.ascontiguousarray(np.tile(np.asarray(ATOL, dtype=float)[:, None], (1, nb))) if per_member_atol else np.ascontiguousarray(ATOL, dtype=float)
        bufs = {}

        def dmalloc(name, nbytes):
            q = ffi.vp()
            ffi.check(dev.dsh_malloc(c, nbytes, 0, C.byref(q)))
            bufs[name] = q
            return q
        try:
            for name, arr in (("p", np.ascontiguousarray(p.T)), ("atol", atol)):
                ffi.check(dev.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(ffi.vp), arr.nbytes))
            shapes = dict(y=((te.size, N, nb), np.float64), stats=((5, nb), np.int32), status=((nb,), np.int32), t_root=((nb,), np.float64), root_idx=((nb,), np.int32),
                          ncols=((nb,), np.int32))
            for name, (shape, dtype) in shapes.items():
                dmalloc(name, int(np.prod(shape)) * np.dtype(dtype).itemsize)
            o = AdaptiveOptions()
            dev.dsh_adaptive_default_options(C.byref(o))
            o.group = group
            tot = (C.c_int64 * 6)()
            common = (model, MODEL_SIZE, nb, bufs["p"], bufs["atol"], nb if per_member_atol else 1, rtol, 0.0, 1.0, C.cast(C.pointer(o), C.c_void_p),
                      te.ctypes.data_as(ffi.c_dp), te.size, bufs["y"], bufs["stats"], bufs["status"], bufs["t_root"], bufs["root_idx"], bufs["ncols"], tot)
            if method == BDF:
                rc = dev.dsh_bdf_solve_adaptive(c, *common)
            elif method == TSIT45:
                rc = dev.dsh_erk_solve_resident(c, method, *common)
            else:
                rc = dev.dsh_sdirk_solve_resident(c, method, *common)
            if rc != 0:
                return rc, None
            out = {}
            for name, (shape, dtype) in shapes.items():
                out[name] = np.empty(shape, dtype=dtype)
                ffi.check(dev.dsh_d2h(c, out[name].ctypes.data_as(ffi.vp), bufs[name], out[name].nbytes))
            out["totals"] = np.array(list(tot), dtype=np.int64)
            return rc, out
        finally:
            for q in bufs.values():
                dev.dsh_free(c, q)


@pytest.fixture
def device():
    d = Device()
    yield d
    d.close()


def bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b, keys=KEYS):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def solved(device, *args, **kw):
    rc, out = device.solve(*args, **kw)
    assert rc == 0, device.dev.dsh_last_error()
    assert (out["status"] == 0).all() and (out["ncols"] == out["y"].shape[0]).all() and out["totals"][5] == 0, "the case was meant to run through"
    assert np.array_equal(out["totals"][:5], out["stats"].astype(np.int64).sum(axis=1)), "the totals are not the sums of the members' counters"
    return out


@pytest.mark.parametrize("group", [1, 64])
def test_bdf_constants_cache_hit_and_miss(device, group):
    p = params(NB)
    first = solved(device, BDF, p, T_STIFF, group=group)                 # miss: the context has no constants yet
    again = solved(device, BDF, p, T_STIFF, group=group)                 # hit: nothing uploaded
    assert same(first, again), "the repeated call differs from the first"
    other = solved(device, BDF, p, T_STIFF, rtol=RTOL / 10, group=group)  # miss: other constants
    assert not np.array_equal(bits(other["y"]), bits(first["y"])) and not np.array_equal(other["stats"], first["stats"]), "another rtol gave the same run"
    back = solved(device, BDF, p, T_STIFF, group=group)                  # miss again: the first constants return
    assert same(first, back), "the first call repeated after another one differs from the first"
    assert first["stats"][0].min() > 20, "the run was meant to take some tens of steps"


@pytest.mark.parametrize("group", [1, 64])
def test_bdf_cached_and_uploaded_save_points_agree(device, group):
    p = params(NB)
    dense = np.unique(np.concatenate([np.linspace(0.05, 39.95, 510), T_STIFF]))
    assert dense.size == 513 and dense.nbytes > 4096 and dense[-1] == T_STIFF[-1]
    at = [int(np.nonzero(dense == t)[0][0]) for t in T_STIFF]
    few = solved(device, BDF, p, T_STIFF, group=group)    # 24 bytes of save points: kept in the context's block
    many = solved(device, BDF, p, dense, group=group)     # 4104 bytes: blocks of the call
    # the save points are interpolated behind the steps and the integration stops at the last of them in both calls: the same steps, the same three columns
    assert np.array_equal(few["stats"], many["stats"]) and np.array_equal(few["totals"], many["totals"])
    assert np.array_equal(bits(few["y"]), bits(many["y"][at]))
    assert same(few, solved(device, BDF, p, T_STIFF, group=group)), "the cached call after the uploaded one differs"


@pytest.mark.parametrize("nb", [NB, 1])
@pytest.mark.parametrize("method", [BDF, TR_BDF2, ESDIRK34, TSIT45], ids=["bdf", "tr_bdf2", "esdirk34", "tsit45"])
@pytest.mark.parametrize("group", [1, 64])
def test_broadcast_atol_equals_the_same_atol_per_member(device, method, nb, group):
    p = params(nb)
    broadcast = solved(device, method, p, t_eval_of(method), group=group)
    per_member = solved(device, method, p, t_eval_of(method), group=group, per_member_atol=True)
    assert same(broadcast, per_member)
    assert broadcast["stats"][0].min() > 3


@pytest.mark.parametrize("method", [BDF, TR_BDF2, ESDIRK34, TSIT45], ids=["bdf", "tr_bdf2", "esdirk34", "tsit45"])
def test_refused_calls_leave_the_context_usable(device, method):
    p = params(NB)
    before = solved(device, method, p, t_eval_of(method))
    rc, _ = device.solve(method, p, t_eval_of(method)[::-1])
    assert rc == DSH_E_INVALID and "increasing" in device.dev.dsh_last_error().decode()
    rc, _ = device.solve(TSIT45, p, T_SHORT, model=ROBERTSON_DAE)
    assert rc == DSH_E_UNSUPPORTED and "MassMatrixNotSupported" in device.dev.dsh_last_error().decode()
    assert same(before, solved(device, method, p, t_eval_of(method))), "the solve after two refused calls differs from the one before them"
