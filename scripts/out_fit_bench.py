"""The measurements of profiles/out_fit.md (needs an MI355X): the fit-objective kernels k_out_fit / k_out_fit_gn (csrc/dsh_out_fit_kernel.hpp) on the workload of
profiles/out_sens.md — battery model with two outputs, 262 144 members, 8 save points.

    python scripts/out_fit_bench.py kernel      # HIP events: 3 warm-up + 50 timed calls of dsh_model_out_fit (both forms, shared and per-member data) and of dsh_model_out_sens
    python scripts/out_fit_bench.py wall        # solve_dense_sens_fit against solve_dense_sens_outputs + the numpy reduction of tests/out_fit_models.py, alternating
    python scripts/out_fit_bench.py footprint fit|outputs    # device memory the context holds after one call of one route (a fresh process: the pool keeps every block)
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import out_fit_models as F  # noqa: E402
import out_sens_models as M  # noqa: E402

NB, NCOLS = 262144, 8
TE = [360.0 * (k + 1) for k in range(NCOLS)]


def kernel():
    from diffsol_amd import _ffi, diffsl as fe
    m = fe.DiffslModel(M.spm_out())
    n, npar, nout = m.n, m.nparams, m.nout
    L = _ffi.load_device_lib()
    c = _ffi.vp()
    _ffi.check(L.dsh_ctx_create(0, None, C.byref(c)))

    def up(a):
        a = np.ascontiguousarray(a)
        q = _ffi.vp()
        _ffi.check(L.dsh_malloc(c, a.nbytes, 0, C.byref(q)))
        _ffi.check(L.dsh_h2d(c, q, a.ctypes.data_as(_ffi.vp), a.nbytes))
        return q

    rng = np.random.default_rng(1)
    t = np.ascontiguousarray(np.linspace(0.0, 1.0, NCOLS))
    y, sens = up(rng.uniform(0.35, 0.65, (NCOLS, n, NB))), up(rng.uniform(-1.0, 1.0, (npar, NCOLS, n, NB)))
    p = up(rng.uniform(0.5, 2.0, (npar, NB)))
    shared, per_member, w = up(rng.uniform(-1.0, 1.0, (NCOLS, nout))), up(rng.uniform(-1.0, 1.0, (NCOLS, nout, NB))), up(rng.uniform(0.5, 2.0, (NCOLS, nout)))
    nq = npar * (npar + 1) // 2
    loss, grad, gn = up(np.zeros(NB)), up(np.zeros((npar, NB))), up(np.zeros((nq, NB)))
    out, dout = up(np.zeros((NCOLS, nout, NB))), up(np.zeros((npar, NCOLS, nout, NB)))
    tp = t.ctypes.data_as(_ffi.c_dp)
    rows = 4  # state rows the two outputs name (profiles/out_sens.md)
    reads = (rows * (1 + npar) * NCOLS + npar) * NB * 8

    def timed(label, nbytes, call):
        for _ in range(3):
            _ffi.check(call())
        _ffi.check(L.dsh_ctx_set_timing(c, 1))
        for _ in range(50):
            _ffi.check(call())
        k, ms = C.c_int64(0), C.c_double(0.0)
        _ffi.check(L.dsh_ctx_get_timing(c, C.byref(k), C.byref(ms)))
        _ffi.check(L.dsh_ctx_set_timing(c, 0))
        assert k.value == 50, k.value
        mean = ms.value / 50
        print(f"{label}: mean of 50 = {mean:.4f} ms, byte model {nbytes / 1e6:.1f} MB = {nbytes / 8e12 * 1e3:.4f} ms at 8 TB/s, achieved {nbytes / mean / 1e9:.2f} TB/s")

    fit = lambda data, pm, wt, g: L.dsh_model_out_fit(c, m.model_id, NB, NCOLS, tp, y, sens, NCOLS * n * NB, n * NB, p, None, data, pm, wt, loss, grad, g)
    timed("k_out_sens", reads + (1 + npar) * NCOLS * nout * NB * 8, lambda: L.dsh_model_out_sens(c, m.model_id, NB, NCOLS, tp, y, sens, p, None, out, dout))
    for form, g, res in (("k_out_fit", None, 1 + npar), ("k_out_fit_gn", gn, 1 + npar + nq)):
        timed(form + ", shared data, no weights", reads + res * NB * 8, lambda: fit(shared, 0, None, g))
        timed(form + ", shared data, weights", reads + res * NB * 8, lambda: fit(shared, 0, w, g))
        timed(form + ", per-member data, weights", reads + (NCOLS * nout + res) * NB * 8, lambda: fit(per_member, 1, w, g))
    timed("k_out_sens (again)", reads + (1 + npar) * NCOLS * nout * NB * 8, lambda: L.dsh_model_out_sens(c, m.model_id, NB, NCOLS, tp, y, sens, p, None, out, dout))
    L.dsh_ctx_destroy(c)


def _solver():
    import diffsol_amd as H
    from diffsol_amd import diffsl as fe
    m = fe.DiffslModel(M.spm_out())
    p = np.random.default_rng(5).uniform(0.6, 1.4, (NB, 1))
    return H.Solver(m, p, nbatch=NB, sens=True, rtol=1e-6, atol=[1e-6]), m


def _data(m):
    # shared data: plausible observations of the two outputs (what is timed does not depend on the values)
    return np.stack([np.linspace(3.9, 3.5, NCOLS), np.linspace(0.7, 0.2, NCOLS)], axis=1)


def wall():
    s, m = _solver()
    data = _data(m)
    rows = []
    for it in range(4):
        t0 = time.perf_counter()
        loss, grad, tot, gn = s.solve_dense_sens_fit(TE, data, gauss_newton=True, group=1)
        t1 = time.perf_counter()
        out, dout, tot2 = s.solve_dense_sens_outputs(TE, group=1)
        t2 = time.perf_counter()
        r = F.from_solver_outputs(out, dout, data, gn=True)
        t3 = time.perf_counter()
        assert tot == tot2
        same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip((loss, grad, gn), r))
        rows.append((t1 - t0, t2 - t1, t3 - t2))
        print(f"pair {it}{' (dropped)' if it == 0 else ''}: solve_dense_sens_fit {t1 - t0:.4f} s | solve_dense_sens_outputs {t2 - t1:.4f} s + numpy reduction {t3 - t2:.4f} s = {t3 - t1:.4f} s"
              f" | bitwise equal: {same} | failed members {tot['failed_members']}, members with a NaN loss {int(np.isnan(loss).sum())}")
    npar, nout = m.nparams, m.nout
    print(f"copied to the host: fit {(1 + npar + npar * npar) * NB * 8 / 1e6:.1f} MB (loss, grad, gn packed {(1 + npar + npar * (npar + 1) // 2) * NB * 8 / 1e6:.1f} MB)"
          f" + data to the device {data.nbytes} B; outputs {(1 + npar) * NCOLS * nout * NB * 8 / 1e6:.1f} MB")


def footprint(which):
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)

    def used():
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return total.value - free.value

    s, m = _solver()
    before = used()
    if which == "fit":
        s.solve_dense_sens_fit(TE, _data(m), gauss_newton=True, group=1)
    else:
        s.solve_dense_sens_outputs(TE, group=1)
    print(f"footprint {which}: device memory in use grew by {(used() - before) / 1e6:.1f} MB over the call (the context's pool keeps every block the call used)")


if __name__ == "__main__":
    {"kernel": kernel, "wall": wall, "footprint": lambda: footprint(sys.argv[2])}[sys.argv[1]]()
