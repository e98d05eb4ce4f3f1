"""The op queue (dsh_ctx_set_op_queue, diffsol_amd/csrc/dsh_opq.hip): element-wise entry points record instead of launching and the recorded run is launched as
one chain kernel.  The immediate kernels are pinned to numpy and the oracle by test_gpu_la.py; here they are the yardstick, and the queue must reproduce them
BIT FOR BIT (uint64 equality) — on random programs, for every call that hands data to the host, and for whole trait-mode solves."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NVEC = 6    # vectors the programs write
NPRIS = 3   # vectors the programs only read (they keep the data from degenerating into NaN everywhere)
NCOL = 8    # columns of the matrix
NBC = 3     # broadcast operands (n doubles each)


@pytest.fixture(scope="module")
def L():
    from diffsol_amd import _ffi
    return _ffi.load_device_lib()


def chk(L, rc):
    assert rc == 0, (rc, L.dsh_last_error())


class Ctx:
    def __init__(self, L, queue):
        self.L = L
        self.h = C.c_void_p()
        chk(L, L.dsh_ctx_create(0, None, C.byref(self.h)))
        chk(L, L.dsh_ctx_set_op_queue(self.h, 1 if queue else 0))
        assert L.dsh_ctx_get_op_queue(self.h) == (1 if queue else 0)

    def malloc(self, nbytes, zero=0):
        p = C.c_void_p()
        chk(self.L, self.L.dsh_malloc(self.h, nbytes, zero, C.byref(p)))
        return p.value

    def stats(self):
        out = (C.c_int64 * 4)()
        chk(self.L, self.L.dsh_ctx_op_queue_stats(self.h, out))
        return [int(v) for v in out]

    def close(self):
        if self.h:
            self.L.dsh_ctx_destroy(self.h)
            self.h = None


class Arena:
    """One device allocation: NVEC + NPRIS vectors, an n x NCOL matrix and NBC broadcast operands, back to back (so that a shifted view of one vector runs into the
    next).  Offsets are in doubles."""

    def __init__(self, n, nb):
        self.n, self.nb, self.total = n, nb, n * nb
        t = self.total
        self.vec = [k * t for k in range(NVEC)]
        self.pris = [(NVEC + k) * t for k in range(NPRIS)]
        self.mat = (NVEC + NPRIS) * t
        self.bc = [(NVEC + NPRIS + NCOL) * t + k * n for k in range(NBC)]
        self.size = (NVEC + NPRIS + NCOL) * t + NBC * n

    def col(self, j):
        return self.mat + j * self.total


KINDS = ("add", "sub", "add_assign", "sub_assign", "mul_assign", "div_assign", "mul_scalar", "mul_assign_scalar", "axpy", "axpy_beta0", "axpby_to", "axpby_to_copy",
         "copy", "copy_bcast", "d2d", "fill", "fill_special", "div_by_zero", "set_index_all", "set_column", "set_column_bcast", "column_axpy", "ladder", "scale_add_assign",
         "scale_add_assign_mat", "shifted_read", "bcast_inside", "refresh")


def make_program(n, nb, seed, ncalls=200):
    """A list of (entry point name, argument tuple with device offsets in doubles as ('p', off)).  No single call races with itself: the operands of one call are
    either the identical range or disjoint from what it writes (the immediate kernels are only a yardstick where they are deterministic); hazards are BETWEEN calls."""
    rng = np.random.default_rng(seed)
    A = Arena(n, nb)
    t = A.total
    P = lambda off: ("p", int(off))
    prog, kinds = [], []

    def rv(k=1, exclude=()):
        pool = [v for v in range(NVEC) if v not in exclude]
        return [int(x) for x in rng.choice(pool, size=k, replace=False)]

    def src():  # a full-batch source: a pristine vector or a pool vector
        return A.pris[int(rng.integers(NPRIS))] if rng.random() < 0.4 else A.vec[int(rng.integers(NVEC))]

    def scalar():
        return float(rng.choice([0.5, -1.25, 2.0, 1.0, -0.75, 3.0]))

    while len(prog) < ncalls:
        # every kind once, then at random; one call in six restores a vector from the read-only data
        kind = KINDS[len(kinds)] if len(kinds) < len(KINDS) else ("refresh" if rng.random() < 1 / 6 else KINDS[int(rng.integers(len(KINDS)))])
        kinds.append(kind)
        bc = rng.random() < 0.3 and nb != 1
        if kind in ("add", "sub"):
            (d,) = rv()
            a, b = src(), src()
            if bc:
                prog.append(("dsh_vec_" + kind, (n, nb, P(a), nb, P(A.bc[int(rng.integers(NBC))]), 1, P(A.vec[d]))))
            else:
                prog.append(("dsh_vec_" + kind, (n, nb, P(a), nb, P(b), nb, P(A.vec[d]))))
        elif kind in ("add_assign", "sub_assign", "mul_assign"):
            (d,) = rv()
            if bc:
                prog.append(("dsh_vec_" + kind, (n, nb, P(A.vec[d]), P(A.bc[int(rng.integers(NBC))]), 1)))
            else:
                prog.append(("dsh_vec_" + kind, (n, nb, P(A.vec[d]), P(src()), nb)))  # the source may be the destination itself: dst == src
        elif kind == "div_assign":
            (d,) = rv()
            prog.append(("dsh_vec_div_assign", (n, nb, P(A.vec[d]), P(A.pris[int(rng.integers(NPRIS))]), nb)))
        elif kind == "div_by_zero":
            d, z = rv(2)
            prog.append(("dsh_vec_fill", (n, nb, P(A.vec[z]), 0.0)))
            prog.append(("dsh_vec_div_assign", (n, nb, P(A.vec[d]), P(A.vec[z]), nb)))
        elif kind == "mul_scalar":
            (d,) = rv()
            prog.append(("dsh_vec_mul_scalar", (n, nb, P(src()), scalar(), P(A.vec[d]))))
        elif kind == "mul_assign_scalar":
            (d,) = rv()
            prog.append(("dsh_vec_mul_assign_scalar", (n, nb, P(A.vec[d]), scalar())))
        elif kind in ("axpy", "axpy_beta0"):
            (d,) = rv()
            beta = 0.0 if kind == "axpy_beta0" else scalar()
            if bc:
                prog.append(("dsh_vec_axpy", (n, nb, scalar(), P(A.bc[int(rng.integers(NBC))]), 1, beta, P(A.vec[d]))))
            else:
                prog.append(("dsh_vec_axpy", (n, nb, scalar(), P(src()), nb, beta, P(A.vec[d]))))
        elif kind in ("axpby_to", "axpby_to_copy"):
            x, out, cp = rv(3)
            y0 = A.vec[out] if rng.random() < 0.5 else A.pris[int(rng.integers(NPRIS))]  # out may be y0
            prog.append(("dsh_vec_axpby_to", (n, nb, scalar(), P(A.vec[x]), scalar(), P(y0), P(A.vec[out]), P(A.vec[cp]) if kind == "axpby_to_copy" else None)))
        elif kind == "copy":
            (d,) = rv()
            prog.append(("dsh_vec_copy", (n, nb, P(src()), nb, P(A.vec[d]))))
        elif kind == "copy_bcast":
            (d,) = rv()
            prog.append(("dsh_vec_copy", (n, nb, P(A.bc[int(rng.integers(NBC))]), 1, P(A.vec[d]))))
        elif kind == "d2d":
            (d,) = rv()
            prog.append(("dsh_d2d", (P(A.vec[d]), P(src()), 8 * t)))
        elif kind == "fill":
            (d,) = rv()
            prog.append(("dsh_vec_fill", (n, nb, P(A.vec[d]), scalar())))
        elif kind == "fill_special":
            (d,) = rv()
            prog.append(("dsh_vec_fill", (n, nb, P(A.vec[d]), float(rng.choice([np.nan, np.inf, -np.inf])))))
        elif kind == "set_index_all":
            (d,) = rv()
            prog.append(("dsh_vec_set_index_all", (nb, P(A.vec[d]), int(rng.integers(n)), scalar())))
        elif kind == "set_column":
            prog.append(("dsh_mat_set_column", (n, NCOL, nb, P(A.mat), int(rng.integers(NCOL)), P(src()), nb)))
        elif kind == "set_column_bcast":
            prog.append(("dsh_mat_set_column", (n, NCOL, nb, P(A.mat), int(rng.integers(NCOL)), P(A.bc[int(rng.integers(NBC))]), 1 if nb != 1 else nb)))
        elif kind == "column_axpy":
            j, i = [int(x) for x in rng.choice(NCOL, size=2, replace=False)]
            prog.append(("dsh_mat_column_axpy", (n, nb, P(A.mat), scalar(), j, i)))
        elif kind == "ladder":  # the Nordsieck update: D[:, i] += D[:, i + 1] for i = k .. 0, then a vector takes column 0
            k = int(rng.integers(1, NCOL - 1))
            for i in range(k, -1, -1):
                prog.append(("dsh_mat_column_axpy", (n, nb, P(A.mat), 1.0, i + 1, i)))
            (d,) = rv()
            prog.append(("dsh_vec_add_assign", (n, nb, P(A.vec[d]), P(A.col(0)), nb)))
        elif kind == "scale_add_assign":
            (d,) = rv()
            x = A.bc[int(rng.integers(NBC))] if bc else src()
            prog.append(("dsh_mat_scale_add_assign", (n, nb, P(A.vec[d]), P(x), 1 if bc else nb, scalar(), P(src()), nb)))
        elif kind == "scale_add_assign_mat":  # over the whole matrix: another total than the vector operations
            prog.append(("dsh_mat_scale_add_assign", (n * 2, nb, P(A.col(0)), P(A.col(2)), nb, scalar(), P(A.col(4)), nb)))
        elif kind == "shifted_read":  # a view that starts inside vector s and runs into vector s + 1, read right after s was written
            s = int(rng.integers(NVEC - 1))
            (d,) = rv(exclude=(s, s + 1))
            shift = int(rng.choice([1, t - 1, max(1, t // 2)]))
            prog.append(("dsh_vec_mul_assign_scalar", (n, nb, P(A.vec[s]), scalar())))
            prog.append(("dsh_vec_add_assign", (n, nb, P(A.vec[d]), P(A.vec[s] + shift), nb)))
        elif kind == "bcast_inside":  # a broadcast operand that lives inside a vector written just before
            s, d = rv(2)
            prog.append(("dsh_vec_axpy", (n, nb, scalar(), P(src()), nb, 1.0, P(A.vec[s]))))
            if nb != 1:
                prog.append(("dsh_vec_sub_assign", (n, nb, P(A.vec[d]), P(A.vec[s] + int(rng.integers(t - n + 1))), 1)))
        elif kind == "refresh":
            (d,) = rv()
            prog.append(("dsh_vec_copy", (n, nb, P(A.pris[int(rng.integers(NPRIS))]), nb, P(A.vec[d]))))
    return A, prog, set(kinds)


def initial_data(A, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 2.0, A.size) * rng.choice([-1.0, 1.0], A.size)
    return np.ascontiguousarray(x)


def run_program(L, ctx, A, prog, init, lo=0, hi=None):
    """Runs prog[lo:hi] on a fresh arena of `ctx`; returns the arena's final contents as uint64."""
    base = ctx.malloc(8 * A.size)
    chk(L, L.dsh_h2d(ctx.h, base, init.ctypes.data_as(C.c_void_p), 8 * A.size))
    for name, args in prog[lo:hi]:
        a = [C.c_void_p(base + 8 * x[1]) if isinstance(x, tuple) else x for x in args]
        chk(L, getattr(L, name)(ctx.h, *a))
    out = np.empty(A.size)
    chk(L, L.dsh_d2h(ctx.h, out.ctypes.data_as(C.c_void_p), base, 8 * A.size))  # no explicit flush: the download launches what is queued
    chk(L, L.dsh_free(ctx.h, base))
    return out.view(np.uint64)


@pytest.fixture(scope="module")
def ctxs(L):
    off, on = Ctx(L, False), Ctx(L, True)
    yield off, on
    off.close()
    on.close()


# (5, 209716): total = 1 048 580, just past the 4096 x 256 grid cap — the grid-stride loop of the chain kernel runs a second pass
@pytest.mark.parametrize("n,nb", [(3, 1), (3, 63), (3, 65), (7, 4099), (5, 209716)])
def test_random_programs_queue_on_equals_off_bit_for_bit(L, ctxs, n, nb):
    off, on = ctxs
    for seed in ((1, 2, 3) if n * nb < 100000 else (1,)):
        A, prog, kinds = make_program(n, nb, 1000 * seed + n)
        assert kinds == set(KINDS), "every kind of call must appear in the program"
        names = {name for name, _ in prog}
        assert names >= {"dsh_vec_add", "dsh_vec_sub", "dsh_vec_add_assign", "dsh_vec_sub_assign", "dsh_vec_mul_assign", "dsh_vec_div_assign", "dsh_vec_mul_scalar",
                         "dsh_vec_mul_assign_scalar", "dsh_vec_axpy", "dsh_vec_axpby_to", "dsh_vec_copy", "dsh_d2d", "dsh_vec_fill", "dsh_mat_set_column",
                         "dsh_mat_column_axpy", "dsh_mat_scale_add_assign"}
        init = initial_data(A, seed)
        s0 = on.stats()
        want = run_program(L, off, A, prog, init)
        got = run_program(L, on, A, prog, init)
        s1 = on.stats()
        bad = np.flatnonzero(want != got)
        assert bad.size == 0, f"n={n} nb={nb} seed={seed}: {bad.size} of {want.size} words differ, first at {bad[:5]}: {want[bad[:5]]} vs {got[bad[:5]]}"
        written = want.view(np.float64)[:A.pris[0]]
        assert np.isfinite(written).mean() > 0.1, "the program degenerated: nothing left to compare"
        assert s1[0] - s0[0] == len(prog), "every call of the program is an enqueuing call"
        assert s1[1] - s0[1] < len(prog), "the queue must have merged launches"
        assert off.stats() == [0, 0, 0, 0]


def test_host_never_sees_stale_data(L, ctxs):
    """Without an explicit flush, every call that hands results to the host (or to another kernel) sees the queued writes."""
    n, nb = 3, 67
    t = n * nb
    rng = np.random.default_rng(7)
    x0 = np.ascontiguousarray(rng.uniform(0.5, 2.0, t))
    amat = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (n, n, nb)) + 4.0 * np.eye(n)[:, :, None])  # [col][row][b]: diagonally dominant
    pars = np.ascontiguousarray(np.stack([np.full(nb, 0.04), np.full(nb, 1e4), np.full(nb, 3e7)]) * rng.uniform(0.9, 1.1, (3, nb)))
    results = []
    for ctx in ctxs:
        h = ctx.h
        r = {}
        x, y, z = (ctx.malloc(8 * t) for _ in range(3))
        a, p = ctx.malloc(8 * n * t), ctx.malloc(8 * 3 * nb)
        chk(L, L.dsh_h2d(h, x, x0.ctypes.data_as(C.c_void_p), 8 * t))
        chk(L, L.dsh_h2d(h, a, amat.ctypes.data_as(C.c_void_p), 8 * n * t))
        chk(L, L.dsh_h2d(h, p, pars.ctypes.data_as(C.c_void_p), 8 * 3 * nb))
        # d2h after queued writes
        chk(L, L.dsh_vec_mul_scalar(h, n, nb, x, 1.5, y))
        chk(L, L.dsh_vec_add_assign(h, n, nb, y, x, nb))
        out = np.empty(t)
        chk(L, L.dsh_d2h(h, out.ctypes.data_as(C.c_void_p), y, 8 * t))
        r["d2h"] = out.copy()
        assert np.array_equal(out, x0 * 1.5 + x0)
        # vec_download (transposing)
        chk(L, L.dsh_vec_axpy(h, n, nb, 2.0, x, nb, -1.0, y))
        out = np.empty((nb, n))
        chk(L, L.dsh_vec_download(h, n, nb, y, out.ctypes.data_as(C.POINTER(C.c_double))))
        r["download"] = out.copy()
        assert np.array_equal(out, (2.0 * x0 + -1.0 * (x0 * 1.5 + x0)).reshape(n, nb).T)
        # norms
        chk(L, L.dsh_vec_sub(h, n, nb, y, nb, x, nb, z))
        v = C.c_double()
        chk(L, L.dsh_vec_norm(h, n, nb, z, 2, C.byref(v)))
        r["norm"] = v.value
        chk(L, L.dsh_vec_fill(h, n, nb, y, 1e-3))
        chk(L, L.dsh_vec_mul_assign_scalar(h, n, nb, z, 3.0))
        chk(L, L.dsh_vec_squared_norm(h, n, nb, z, x, nb, y, nb, 1e-2, C.byref(v), None))
        r["squared_norm"] = v.value
        assert v.value > 0.0
        # root finding: g0 = x0 - 1, g1 = -(x0 - 1) member-independent rows would be needed for equal results across members: use broadcast-built rows
        row = np.ascontiguousarray(np.repeat(np.array([0.5, -0.25, 2.0]), nb))
        chk(L, L.dsh_h2d(h, y, row.ctypes.data_as(C.c_void_p), 8 * t))
        chk(L, L.dsh_vec_mul_scalar(h, n, nb, y, -2.0, z))
        chk(L, L.dsh_vec_set_index_all(h, nb, z, 2, 4.0))  # component 2 keeps its sign: sign changes in components 0 and 1
        found, idx, frac = C.c_int(), C.c_int(), C.c_double()
        chk(L, L.dsh_vec_root_finding(h, n, nb, y, z, C.byref(found), C.byref(frac), C.byref(idx)))
        r["root"] = (found.value, idx.value, frac.value)
        assert found.value == 0 and idx.value in (0, 1) and frac.value == 2.0 / 3.0
        # LU: the matrix and the right-hand side are finished by queued operations
        lu = C.c_void_p()
        chk(L, L.dsh_lu_create(h, n, nb, C.byref(lu)))
        chk(L, L.dsh_vec_mul_assign_scalar(h, n * n, nb, a, 2.0))
        chk(L, L.dsh_lu_factor(lu, a))
        chk(L, L.dsh_vec_fill(h, n, nb, z, 1.0))
        chk(L, L.dsh_vec_add_assign(h, n, nb, z, x, nb))
        chk(L, L.dsh_lu_solve(lu, z))
        out = np.empty(t)
        chk(L, L.dsh_d2h(h, out.ctypes.data_as(C.c_void_p), z, 8 * t))
        r["lu"] = out.copy()
        sol = np.stack([np.linalg.solve(2.0 * amat[:, :, b].T, 1.0 + x0.reshape(n, nb)[:, b]) for b in range(nb)], axis=1)
        assert np.allclose(out.reshape(n, nb), sol, rtol=1e-12, atol=0)
        L.dsh_lu_destroy(lu)
        # model right-hand side of a queued state
        chk(L, L.dsh_vec_copy(h, n, nb, x, nb, y))
        chk(L, L.dsh_vec_mul_assign_scalar(h, n, nb, y, 0.5))
        chk(L, L.dsh_model_rhs(h, 3, 1, nb, 0.0, y, p, z))
        out = np.empty(t)
        chk(L, L.dsh_d2h(h, out.ctypes.data_as(C.c_void_p), z, 8 * t))
        r["rhs"] = out.copy()
        yy, pp = (0.5 * x0).reshape(n, nb), pars
        assert np.allclose(out.reshape(n, nb)[0], -pp[0] * yy[0] + pp[1] * yy[1] * yy[2], rtol=1e-13)
        # dsh_malloc(zero = 1) of a block just freed by a queued operand's owner
        odd = 8 * t + 8 * 977  # a size nothing else in this context uses: the zeroed block below is the one freed here
        blk, res = ctx.malloc(odd), ctx.malloc(8 * t)
        chk(L, L.dsh_vec_fill(h, n, nb, blk, 3.0))
        chk(L, L.dsh_vec_add(h, n, nb, blk, nb, blk, nb, res))
        chk(L, L.dsh_free(h, blk))
        again = ctx.malloc(odd, zero=1)
        assert again == blk, "the allocation cache must hand the parked block back (the scenario under test)"
        out = np.empty(t)
        chk(L, L.dsh_d2h(h, out.ctypes.data_as(C.c_void_p), res, 8 * t))
        assert np.array_equal(out, np.full(t, 6.0)), "the zeroing of the recycled block overtook the queued operation that read it"
        chk(L, L.dsh_d2h(h, out.ctypes.data_as(C.c_void_p), again, 8 * t))
        assert np.array_equal(out, np.zeros(t))
        for q in (x, y, z, a, p, res, again):
            chk(L, L.dsh_free(h, q))
        results.append(r)
    off, on = results
    for k in off:
        a, b = np.asarray(off[k], dtype=np.float64), np.asarray(on[k], dtype=np.float64)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), k


def test_stats_mean_what_they_say(L, ctxs):
    off, on = ctxs
    n, nb = 3, 65
    t = n * nb
    for ctx in (off, on):
        chk(L, L.dsh_ctx_set_op_queue(ctx.h, 1 if ctx is on else 0))  # resets the counters
        assert ctx.stats() == [0, 0, 0, 0]
        d, y = ctx.malloc(8 * NCOL * t, zero=1), ctx.malloc(8 * t, zero=1)
        # the ladder: 7 column updates and the vector update are one launch
        for i in range(6, -1, -1):
            chk(L, L.dsh_mat_column_axpy(ctx.h, n, nb, d, 1.0, i + 1, i))
        chk(L, L.dsh_vec_add_assign(ctx.h, n, nb, y, d, nb))
        if ctx is on:
            assert ctx.stats() == [8, 0, 0, 0], "nothing may be launched before a result is needed"
        chk(L, L.dsh_ctx_sync(ctx.h))
        if ctx is off:
            assert ctx.stats() == [0, 0, 0, 0]
            for q in (d, y):
                chk(L, L.dsh_free(ctx.h, q))
            continue
        assert ctx.stats() == [8, 1, 0, 1]
        # a shifted-overlap pair: exactly one hazard flush
        chk(L, L.dsh_vec_fill(ctx.h, n, nb, d, 1.0))
        chk(L, L.dsh_vec_copy(ctx.h, n, nb, C.c_void_p(d + 8), nb, y))  # reads d[1 .. t + 1): overlaps what the fill writes, shifted by one element
        assert ctx.stats() == [10, 2, 1, 1]
        chk(L, L.dsh_ctx_flush(ctx.h))  # explicit: neither a hazard nor a non-queuing call
        assert ctx.stats() == [10, 3, 1, 1]
        chk(L, L.dsh_ctx_flush(ctx.h))  # nothing queued: no launch
        assert ctx.stats() == [10, 3, 1, 1]
        # another shape and a full chain are booked as forced by the operation too
        chk(L, L.dsh_vec_fill(ctx.h, n, nb, y, 2.0))
        chk(L, L.dsh_vec_fill(ctx.h, n * 2, nb, d, 2.0))
        assert ctx.stats() == [12, 4, 2, 1]
        for _ in range(40):
            chk(L, L.dsh_vec_mul_assign_scalar(ctx.h, n * 2, nb, d, 1.0))
        assert ctx.stats() == [52, 5, 3, 1]  # 1 + 31 joined, the 33rd operation of the chain forced a launch
        # argument validation is the immediate mode's: same error from the same call, nothing recorded
        assert L.dsh_vec_add_assign(ctx.h, n, nb, y, d, 2) == -5 and b"nbatch" in L.dsh_last_error()
        assert L.dsh_mat_column_axpy(ctx.h, n, nb, d, 1.0, 1, 1) == -1
        assert ctx.stats()[0] == 52
        chk(L, L.dsh_ctx_set_op_queue(ctx.h, 0))  # switching off launches what is queued
        out = np.empty(2 * t)
        chk(L, L.dsh_d2h(ctx.h, out.ctypes.data_as(C.c_void_p), d, 8 * 2 * t))
        assert np.array_equal(out, np.full(2 * t, 2.0))
        assert ctx.stats() == [0, 0, 0, 0]
        chk(L, L.dsh_ctx_set_op_queue(ctx.h, 1))
        for q in (d, y):
            chk(L, L.dsh_free(ctx.h, q))


SOLVE_CASES = [("robertson_ode", 1, 1), ("robertson_ode", 1, 67), ("robertson_ode", 1, 1000), ("robertson", 0, 67), ("exponential_decay_with_root", 0, 8), ("heat1d", 20, 8)]


def _problem(model, nb):
    from helpers import robertson_params
    if model in ("robertson_ode", "robertson"):
        return robertson_params(nb), dict(rtol=1e-4, atol=[1e-8, 1e-14, 1e-6]), [0.4, 4.0, 40.0], 40.0
    if model == "exponential_decay_with_root":  # lock-step: every member must meet the event in the same step
        return np.tile([0.1, 1.0], (nb, 1)), dict(rtol=1e-6, atol=[1e-6, 1e-6]), [1.0, 3.0, 10.0], 10.0
    return np.linspace(0.5, 2.0, nb)[:, None], dict(rtol=1e-6, atol=[1e-6]), [0.01, 0.05, 0.1], 0.1


@pytest.mark.parametrize("method", [0, 1, 2], ids=["bdf", "tr_bdf2", "esdirk34"])
@pytest.mark.parametrize("model,size,nb", SOLVE_CASES, ids=[f"{m}-{nb}" for m, _, nb in SOLVE_CASES])
def test_trait_mode_solves_are_unchanged(model, size, nb, method):
    """The host-driven lock-step integrators over the 1:1 trait operations (fused=False) with the queue on and off: outputs, times, counters and stop reasons are
    bit-identical, and the queue did merge launches."""
    import diffsol_amd as H
    p, tol, t_eval, t_final = _problem(model, nb)
    got = {}
    for on in (False, True):
        s = H.Solver(model, p, nbatch=nb, model_size=size, method=method, fused=False, ensemble_mode=H.ENSEMBLE_LOCKSTEP, op_queue=on, **tol)
        s.set_op_queue(on)  # explicitly off for the yardstick too: DSH_OP_QUEUE=1 in the environment switches every new context on
        assert not s.fused
        y_dense, reason_dense = s.solve_dense(t_eval)
        st_dense, q_dense = s.stats(), s.op_queue_stats()
        s.reset()
        y, ncols, reason, ts, ys = s.solve(t_final, keep_trajectory=True)
        got[on] = dict(y_dense=y_dense, reason_dense=reason_dense, st_dense=st_dense, y=y, ncols=ncols, reason=reason, ts=ts, ys=ys, st=s.stats(), q=s.op_queue_stats(),
                       q_dense=q_dense)
        del s
    a, b = got[False], got[True]
    for k in ("y_dense", "y", "ts", "ys"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    for k in ("reason_dense", "st_dense", "ncols", "reason", "st"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["st"]["number_of_steps"] > 3
    assert a["q"] == dict(ops_enqueued=0, chain_launches=0, hazard_flushes=0, entry_flushes=0)
    for q in (b["q_dense"], b["q"]):
        assert q["ops_enqueued"] > 0 and q["chain_launches"] < q["ops_enqueued"], q
        assert q["hazard_flushes"] + q["entry_flushes"] <= q["chain_launches"]


def test_two_host_threads_share_one_context_with_the_queue_on(L):
    """Each thread runs its own program on its own arena of the SAME context; the calls interleave under the context lock and the planner keeps them apart."""
    n, nb = 3, 65
    progs = [make_program(n, nb, 50 + k) for k in range(2)]
    inits = [initial_data(progs[k][0], 60 + k) for k in range(2)]
    off = Ctx(L, False)
    want = [run_program(L, off, progs[k][0], progs[k][1], inits[k]) for k in range(2)]
    off.close()
    on = Ctx(L, True)
    got, errs = [None, None], []

    def work(k):
        try:
            got[k] = run_program(L, on, progs[k][0], progs[k][1], inits[k])
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    st = on.stats()
    on.close()
    for k in range(2):
        assert np.array_equal(want[k], got[k]), f"thread {k}"
    assert st[0] == len(progs[0][1]) + len(progs[1][1])
