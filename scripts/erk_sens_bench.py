"""Tsit45 with forward sensitivities on the fit objective, and the plain Tsit45 path against another build of the device library (profiles/erk_tsit45_sens.md).

    python scripts/erk_sens_bench.py [--reps 7] [--out results.json] [--plain-against /path/to/other/libdiffsol_hip.so]

* Solver.solve_dense_sens_fit with Tsit45 against the same call with BDF on the same solver settings, both solvers alive in this process, called alternately (the order changes every round) after two
  warm-up rounds: the 4096 starts of examples/fit_decay (11 save points, tolerances 1e-8) and 100 000 members of the same model with 8 save points (tolerances 1e-6),
  per member and in wavefront groups.  Host clock around the call; the call returns after its results are on the host.
* --plain-against: the 100 000-member exponential-decay run of tests/test_gpu_erk.py through dsh_erk_solve_resident, this tree's library and the given one loaded
  side by side (each with local symbol scope) and called alternately, the order inside a round changing every round; the states are compared bit for bit.  Runs INSTEAD of the fit comparison."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diffsol_amd as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--plain-against", default=None)
args = ap.parse_args()
REPS = args.reps
res = {}


def stats(v):
    v = np.asarray(v) * 1e3
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), reps=len(v))


DECAY = "in_i { k = 0.1, y0 = 1.0 }\nu_i { x = y0, y = y0 }\nF_i { -k * u_i }\nout_i { x + y, k * x }\n"
model = None   # compiled below
true = np.array([0.1, 1.0])


def fit_case(name, nb, t_eval, tol, group):
    e = np.exp(-true[0] * t_eval)
    data = np.stack([2 * true[1] * e, true[0] * true[1] * e], axis=1)
    p = true * np.random.default_rng(0).uniform(0.8, 1.2, (nb, 2))
    kw = dict(nbatch=nb, sens=True, sens_rtol=tol, sens_atol=[tol], rtol=tol, atol=[tol, tol])
    solvers = {"bdf": H.Solver(model, p, method=H.METHOD_BDF, **kw), "tsit45": H.Solver(model, p, method=H.METHOD_TSIT45, **kw)}
    times = {k: [] for k in solvers}
    info = {}
    for rep in range(REPS + 2):  # two warm-up rounds (module load, allocations), then alternate
        for k, s in (list(solvers.items())[::-1] if rep % 2 else solvers.items()):   # who goes first changes every round
            t0 = time.perf_counter()
            loss, grad, tot, gn = s.solve_dense_sens_fit(t_eval, data, gauss_newton=True, group=group)   # returns after the results are on the host: synchronised
            dt = time.perf_counter() - t0
            if rep >= 2:
                times[k].append(dt)
            info[k] = dict(steps=tot["number_of_steps"], failed=tot["failed_members"], loss_max=float(loss.max()))
    lb, gb, _, _ = solvers["bdf"].solve_dense_sens_fit(t_eval, data, gauss_newton=True, group=group)
    lt, gt, _, _ = solvers["tsit45"].solve_dense_sens_fit(t_eval, data, gauss_newton=True, group=group)
    res[name] = dict(nb=nb, nt=len(t_eval), tol=tol, group=group, bdf=dict(**stats(times["bdf"]), **info["bdf"]), tsit45=dict(**stats(times["tsit45"]), **info["tsit45"]),
                     max_rel_grad_diff=float(np.abs(gt - gb).max() / np.abs(gb).max()), max_rel_loss_diff=float(np.abs(lt - lb).max() / np.abs(lb).max()))
    print(name, json.dumps(res[name]), flush=True)


def plain_runner(lib_path):
    from diffsol_amd import _ffi
    from test_gpu_erk import AdaptiveOptions
    L = C.CDLL(lib_path, mode=C.RTLD_LOCAL)
    for name, (restype, argtypes) in _ffi.DEVICE_ABI.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    c = _ffi.vp()
    assert L.dsh_ctx_create(0, None, C.byref(c)) == 0
    nb = 100_000
    rng = np.random.default_rng(7)
    p = np.ascontiguousarray(np.stack([rng.uniform(0.05, 2.0, nb), rng.uniform(0.5, 5.0, nb)], axis=1).T)
    atol = np.array([1e-6, 1e-6])
    te = np.array([0.5, 1.0, 2.0, 4.0])
    bufs = {}

    def dmalloc(name, nbytes):
        q = _ffi.vp()
        assert L.dsh_malloc(c, nbytes, 0, C.byref(q)) == 0
        bufs[name] = q
        return q
    for name, arr in (("p", p), ("atol", atol)):
        assert L.dsh_h2d(c, dmalloc(name, arr.nbytes), arr.ctypes.data_as(_ffi.vp), arr.nbytes) == 0
    dmalloc("y", 8 * 4 * 2 * nb); dmalloc("stats", 20 * nb); dmalloc("status", 4 * nb)
    o = AdaptiveOptions()
    L.dsh_adaptive_default_options(C.byref(o))
    o.deterministic_pow, o.group = 1, 64
    opts = C.cast(C.pointer(o), C.c_void_p)
    tot = (C.c_int64 * 6)()

    def run():
        t0 = time.perf_counter()
        rc = L.dsh_erk_solve_resident(c, 3, H.MODELS["exponential_decay"], 0, nb, bufs["p"], bufs["atol"], 1, 1e-6, 0.0, 1.0, opts, te.ctypes.data_as(_ffi.c_dp), 4, bufs["y"],
                                      bufs["stats"], bufs["status"], None, None, None, tot)   # synchronises the stream before it returns
        dt = time.perf_counter() - t0
        assert rc == 0
        y = np.empty((4, 2, nb))
        assert L.dsh_d2h(c, y.ctypes.data_as(_ffi.vp), bufs["y"], y.nbytes) == 0
        return dt, y, int(tot[0])
    return run


if args.plain_against:
    runs = {"this": plain_runner(os.path.join(ROOT, "diffsol_amd", "lib", "libdiffsol_hip.so")), "other": plain_runner(args.plain_against)}
    times = {k: [] for k in runs}
    ys = {}
    for rep in range(REPS + 2):
        for k, r in (list(runs.items())[::-1] if rep % 2 else runs.items()):   # who goes first changes every round
            dt, y, steps = r()
            if rep >= 2:
                times[k].append(dt)
            ys[k] = (y, steps)
    res["plain_tsit45_100000_members_group64"] = dict(this=stats(times["this"]), other=stats(times["other"]), steps=ys["this"][1],
                                                      same_bits=bool(np.array_equal(ys["this"][0], ys["other"][0]) and ys["this"][1] == ys["other"][1]))
    print("plain", json.dumps(res["plain_tsit45_100000_members_group64"]), flush=True)
else:
    from diffsol_amd import diffsl  # noqa: E402
    model = diffsl.DiffslModel(DECAY)
    for group in (1, 64):
        fit_case(f"fit_decay_4096_starts_group{group}", 4096, np.linspace(0.0, 10.0, 11), 1e-8, group)
        fit_case(f"decay_100000_members_8_points_group{group}", 100_000, np.linspace(0.0, 10.0, 8), 1e-6, group)


if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
