"""Inputs of the pivot-facts tests (tests/test_pivot_facts.py on the CPU, tests/test_gpu_pivot_facts.py on the GPU; profiles/pivot_facts.md) and the CPU side of their conditions: which row permutation first-max partial pivoting of M - c J takes in every lane of a lock-step
group, along the accepted steps of the oracle's lock-step group (c = h alpha_order after the step: the matrix the next factorisation of that step size would form).

The Jacobians are written out here in numpy for the whole group at once; tests/test_pivot_facts.py holds them to the oracle's jac_mul."""
import functools

import numpy as np

from helpers import ORACLE_MODEL
from bench import robertson_params, T_EVAL, RTOL, ATOL

# Bdf::_new: alpha_k = 1 / ((1 - kappa_k) gamma_k), gamma_k = sum_{j <= k} 1 / j
KAPPA = np.array([0.0, -0.1850, -1.0 / 9.0, -0.0823, -0.0415, 0.0])
GAMMA = np.concatenate([[0.0], np.cumsum(1.0 / np.arange(1, 6))])
ALPHA = np.concatenate([[0.0], 1.0 / ((1.0 - KAPPA[1:]) * GAMMA[1:])])

IDENTITY = (0, 1, 2)

# lanes of one group disagree: linear members (only the first rate constant is not zero: y0' = -k1 y0, y1' = k1 y0), the second group with k1 of both signs.
# Column 0 of I - c J is (1 + c k1, -c k1, 0): for k1 < 0 row 1 wins once c |k1| > 1/2, for k1 > 0 row 0 always does.  The tolerance is loose enough for the step size
# to double up to that (|y| <= e^12 stays below atol), and the span short enough for the growing members.
MIXED_ATOL, MIXED_RTOL, MIXED_T_EVAL = [1e6, 1e6, 1e6], 1e-4, [1.5, 3.0, 6.0]


def mixed_params():
    rng = np.random.default_rng(7)
    p = np.zeros((192, 3))
    p[:, 0] = 2.0 ** rng.uniform(-1, 1, 192)
    p[64:128:2, 0] *= -1.0
    return p


def nan_params():
    """tests/test_gpu_wave_max_raw.py's members: k2 = 1e308 in the second group (NaN inside the Newton iterations after a few steps), a NaN rate constant in the third"""
    p = robertson_params(192)
    p[64 + 37, 1] = 1e308
    p[128 + 5, 1] = np.nan
    return p


def jacobian(model, y, p):
    """[nb, 3, 3]: df/dy of robertson_ode / robertson (the DAE) at y [nb, 3], p [nb, 3]"""
    nb = len(y)
    J = np.zeros((nb, 3, 3))
    J[:, 0, 0], J[:, 0, 1], J[:, 0, 2] = -p[:, 0], p[:, 1] * y[:, 2], p[:, 1] * y[:, 1]
    J[:, 1, 0], J[:, 1, 1], J[:, 1, 2] = p[:, 0], -p[:, 1] * y[:, 2] - 2.0 * p[:, 2] * y[:, 1], -p[:, 1] * y[:, 1]
    if model == "robertson_ode":
        J[:, 2, 1] = 2.0 * p[:, 2] * y[:, 1]
    else:
        J[:, 2, :] = 1.0
    return J


def mass(model):
    return np.diag([1.0, 1.0, 1.0 if model == "robertson_ode" else 0.0])


def pivot_rows(A):
    """First-max partial pivoting (lu_factor_reg, csrc/dsh_lu_dev.hpp) of A [nb, n, n]: the pivot rows [nb, n] and whether a pivot was exactly zero [nb]."""
    A = np.array(A, dtype=float)
    nb, n, _ = A.shape
    P = np.zeros((nb, n), dtype=int)
    zero = np.zeros(nb, dtype=bool)
    idx = np.arange(nb)
    for i in range(n):
        best, p = np.abs(A[:, i, i]), np.full(nb, i)
        for r in range(i + 1, n):  # `v > best`: the first maximum stays; false with a NaN on either side, so a NaN on the diagonal stays and one below never wins
            v = np.abs(A[:, r, i])
            with np.errstate(invalid="ignore"):
                win = v > best
            best, p = np.where(win, v, best), np.where(win, r, p)
        piv = A[idx, p, i]
        z = piv == 0.0
        zero |= z
        p = np.where(z, i, p)
        P[:, i] = p
        rows_i, rows_p = A[idx, i, :].copy(), A[idx, p, :].copy()
        A[idx, i, :], A[idx, p, :] = rows_p, rows_i
        with np.errstate(all="ignore"):
            l = np.where(z[:, None], 0.0, A[:, i + 1:, i] / np.where(z, 1.0, A[:, i, i])[:, None])
            A[:, i + 1:, i] = l
            A[:, i + 1:, i + 1:] -= l[:, :, None] * A[:, i, None, i + 1:]
    return P, zero


@functools.lru_cache(maxsize=None)
def _walk(model, size, pbytes, nb, rtol, atol, t_end):
    from oracle import oracle as O
    O.build()
    p = np.frombuffer(pbytes).reshape(nb, 3)
    o = O.OracleSolver(ORACLE_MODEL[model], p, nbatch=nb, model_size=size, rtol=rtol, atol=np.asarray(atol, dtype=float))
    o.set_stop_time(t_end)
    M = mass(model)
    out = []
    while True:
        r = o.step()
        s = o.state()
        c = s["h"] * ALPHA[s["order"]]
        P, zero = pivot_rows(M[None] - c * jacobian(model, s["y"], p))
        out.append((c, tuple(sorted(set(map(tuple, P.tolist())))), bool(zero.any())))
        if r == 2:
            return tuple(out)


def walk(model, size, p, rtol, atol, t_end):
    """One lock-step group stepped by the oracle to t_end: per accepted step (c, the set of permutations among its lanes, any exactly zero pivot)."""
    p = np.ascontiguousarray(p, dtype=float)
    return _walk(model, size, p.tobytes(), len(p), float(rtol), tuple(float(a) for a in atol), float(t_end))


def groups(p):
    return [p[g:g + 64] for g in range(0, len(p), 64)]


# ---- the conditions, asserted by the CPU test and again, as conditions on their inputs, by the GPU cases
def identity_condition(nb):
    """Robertson ODE at bench.py's tolerances and save points: identity pivots in every lane at every step, no zero pivot."""
    for g, pg in enumerate(groups(robertson_params(192)[:nb])):
        w = walk("robertson_ode", 1, pg, RTOL, ATOL, T_EVAL[-1])
        assert len(w) > 50 and all(perms == (IDENTITY,) and not z for _, perms, z in w), f"group {g}: {sorted(set(q for _, perms, _ in w for q in perms))}"
    return True


def dae_condition(nb):
    """The Robertson DAE: column 0 of M - c J is (1 + c k1, -c k1, -c), so row 2 wins once c (1 - k1) > 1.  Every step's permutation is the same in all lanes
    of the group, the solve starts with the identity and leaves it for good, and steps on either side have distinct c (so each side is factorised)."""
    for g, pg in enumerate(groups(robertson_params(192)[:nb])):
        w = walk("robertson", 0, pg, RTOL, ATOL, T_EVAL[-1])
        assert all(len(perms) == 1 and not z for _, perms, z in w), f"group {g}: lanes disagree"
        ident = [perms == (IDENTITY,) for _, perms, _ in w]
        first = ident.index(False)
        assert first > 50 and not any(ident[first:]) and len(ident) - first > 50, (g, first, len(ident))
        assert {perms for _, perms, _ in w[first:]} == {((2, 1, 2),)}
        k1 = pg[:, 0]
        for c, perms, _ in w:
            if (c * (1.0 - k1) > 1.0 + 1e-9).all():
                assert perms == ((2, 1, 2),), (g, c)
            if (c * (1.0 - k1) < 1.0 - 1e-9).all():
                assert perms == (IDENTITY,), (g, c)
        assert len({c for c, _, _ in w[:first]}) > 5 and len({c for c, _, _ in w[first:]}) > 5
    return True


def mixed_condition():
    """Linear members, the second group with k1 of both signs: its lanes disagree (identity and (1, 1, 2)) over steps with several distinct c, after steps on which
    all of them have the identity; the first and the third group have the identity everywhere."""
    g0, g1, g2 = groups(mixed_params())
    for pg in (g0, g2):
        w = walk("robertson_ode", 1, pg, MIXED_RTOL, MIXED_ATOL, MIXED_T_EVAL[-1])
        assert len(w) > 10 and all(perms == (IDENTITY,) and not z for _, perms, z in w)
    w = walk("robertson_ode", 1, g1, MIXED_RTOL, MIXED_ATOL, MIXED_T_EVAL[-1])
    mixed = [c for c, perms, z in w if len(perms) > 1]
    assert not any(z for _, _, z in w)
    assert all(set(perms) <= {IDENTITY, (1, 1, 2)} for _, perms, _ in w)
    assert len(w[0][1]) == 1 and len(mixed) >= 4 and len(set(mixed)) >= 3, (len(w), mixed)
    return True
