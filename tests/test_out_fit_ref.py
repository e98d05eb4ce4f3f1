"""The CPU restatement of the fit-objective kernel (tests/out_fit_models.py) anchored without the kernel: on the rational test model with closed-form states and
sensitivities its gradient is the derivative of its own loss, its Gauss-Newton matrix is 2 J^T W J, and a missing observation is an observation of weight zero."""
import numpy as np
import pytest

import out_fit_models as F
import out_sens_models as M

NB, NCOLS = 7, 5
T = np.linspace(0.25, 2.0, NCOLS)


@pytest.fixture(scope="module")
def tw():
    return M.HostTwin(M.RATIONAL)


def _closed_form(p):
    """RATIONAL: x' = -k x, x(0) = y0; y' = -y, y(0) = 1  ->  y [ncols, 2, nb], sens [2, ncols, 2, nb] for p [2, nb] = (k, y0)"""
    k, y0 = p[0][None, :], p[1][None, :]
    t = T[:, None]
    e = np.exp(-k * t)
    y = np.stack([y0 * e, np.exp(-t) * np.ones_like(e)], axis=1)
    z = np.zeros_like(e)
    sens = np.stack([np.stack([-t * y0 * e, z], axis=1), np.stack([e, z], axis=1)], axis=0)
    return y, sens


def _problem(tw):
    rng = np.random.default_rng(11)
    p = np.stack([rng.uniform(0.5, 1.5, NB), rng.uniform(0.8, 2.0, NB)])
    out_true, _ = tw.evaluate(T, *_closed_form(p * rng.uniform(0.8, 1.2, p.shape)), p)
    data = out_true[:, :, 0] + rng.uniform(-0.05, 0.05, (NCOLS, tw.nout))  # shared: the first member's outputs at nearby parameters, with noise
    per_member = out_true + rng.uniform(-0.05, 0.05, out_true.shape)
    w = rng.uniform(0.5, 2.0, (NCOLS, tw.nout))
    return p, data, per_member, w


def _fit(tw, p, data, w=None, gn=False):
    y, sens = _closed_form(p)
    return F.restate(tw, T, y, sens, p, data, w, gn=gn)


@pytest.mark.parametrize("per_member", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_the_gradient_is_the_derivative_of_the_loss(tw, per_member, weighted):
    """Central differences of the restatement's own loss in (k, y0), step 1e-6 |p|, against its gradient.  Observed here on the CPU: the largest disagreement is
    1.25e-10 of the member's largest gradient component (0.72e-10 ... 1.25e-10 over the four cases) - the cancellation error of the difference quotient, of the
    order of 2^-53 L / h for losses of order 0.1 ... 1; the truncation error, of order h^2, is far below it.  Asserted: 10 times the observed maximum."""
    p, shared, pm, w = _problem(tw)
    data, wt = (pm if per_member else shared), (w if weighted else None)
    loss, grad = _fit(tw, p, data, wt)
    assert np.isfinite(loss).all() and (loss > 0).all() and np.abs(grad).min() > 0
    worst = 0.0
    for j in range(2):
        h = np.zeros_like(p)
        h[j] = 1e-6 * np.abs(p[j])
        fd = (_fit(tw, p + h, data, wt)[0] - _fit(tw, p - h, data, wt)[0]) / (2 * h[j])
        worst = max(worst, (np.abs(fd - grad[j]) / np.abs(grad).max(axis=0)).max())
    print("central differences vs gradient, relative to the member's largest component:", worst)
    assert worst < 1.25e-9


@pytest.mark.parametrize("per_member", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_the_gauss_newton_matrix_is_2_jt_w_j(tw, per_member, weighted):
    """against numpy.einsum on the same dout: another summation order, so to rounding — n = ncols nout terms, each product rounded twice (w d_j, then times d_l) and
    each partial sum once, on both sides: |difference| <= 2 (n + 2) u sum |terms|, u = 2^-53"""
    p, shared, pm, w = _problem(tw)
    data, wt = (pm if per_member else shared), (w if weighted else None)
    y, sens = _closed_form(p)
    loss, grad, gnp = F.restate(tw, T, y, sens, p, data, wt, gn=True)
    loss2, grad2 = F.restate(tw, T, y, sens, p, data, wt)
    assert np.array_equal(loss, loss2) and np.array_equal(grad, grad2)  # asking for the matrix changes nothing else
    out, J = tw.evaluate(T, y, sens, p)
    W = wt if weighted else np.ones((NCOLS, tw.nout))
    want = 2 * np.einsum("jckb,ck,lckb->bjl", J, W, J)
    bound = 2 * (NCOLS * tw.nout + 2) * 2.0 ** -53 * 2 * np.einsum("jckb,ck,lckb->bjl", np.abs(J), W, np.abs(J))
    got = F.unpack(gnp, 2)
    assert np.array_equal(got, np.transpose(got, (0, 2, 1))) and (np.abs(got - want) <= bound).all(), np.abs(got - want).max()
    assert (np.linalg.eigvalsh(got) > 0).all()
    # and the gradient is 2 J^T W r, to the same kind of bound
    r = out - (data if per_member else data[:, :, None])
    gwant = 2 * np.einsum("jckb,ck,ckb->jb", J, W, r)
    gbound = 2 * (NCOLS * tw.nout + 2) * 2.0 ** -53 * 2 * np.einsum("jckb,ck,ckb->jb", np.abs(J), W, np.abs(r))
    assert (np.abs(grad - gwant) <= gbound).all()


@pytest.mark.parametrize("per_member", [False, True])
def test_a_missing_observation_is_an_observation_of_weight_zero(tw, per_member):
    p, shared, pm, w = _problem(tw)
    data = (pm if per_member else shared).copy()
    holes = [(0, 1), (2, 0), (4, 2)]
    w0, nan_data = w.copy(), data.copy()
    for c, k in holes:
        w0[c, k] = 0.0
        nan_data[c, k] = np.nan
    a = _fit(tw, p, nan_data, w, gn=True)
    b = _fit(tw, p, data, w0, gn=True)
    for x, y in zip(a, b):
        assert np.isfinite(x).all() and np.array_equal(x, y)
    full = _fit(tw, p, data, w, gn=True)
    assert not np.array_equal(a[0], full[0])  # the holes do change the result


def test_no_observation_at_all_gives_exact_zeros(tw):
    p, shared, pm, w = _problem(tw)
    for data in (np.full_like(shared, np.nan), np.full_like(pm, np.nan)):
        for wt in (None, w):
            for x in _fit(tw, p, data, wt, gn=True):
                assert np.array_equal(x, np.zeros_like(x))
    # per-member data: one member without observations, the others unchanged
    one = pm.copy()
    one[:, :, 3] = np.nan
    a, b = _fit(tw, p, one, w, gn=True), _fit(tw, p, pm, w, gn=True)
    keep = np.arange(NB) != 3
    for x, y in zip(a, b):
        assert np.array_equal(x[..., 3], np.zeros_like(x[..., 3])) and np.array_equal(x[..., keep], y[..., keep])


@pytest.mark.parametrize("per_member", [False, True])
def test_no_weights_are_unit_weights_bit_for_bit(tw, per_member):
    p, shared, pm, _ = _problem(tw)
    data = pm if per_member else shared
    a = _fit(tw, p, data, None, gn=True)
    b = _fit(tw, p, data, np.ones((NCOLS, tw.nout)), gn=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_members_without_all_columns_are_blank(tw):
    p, shared, _, w = _problem(tw)
    y, sens = _closed_form(p)
    mc = np.array([NCOLS, 0, NCOLS - 1, NCOLS, 2, NCOLS, 1], dtype=np.int32)
    a = F.restate(tw, T, y, sens, p, shared, w, member_cols=mc, gn=True)
    b = F.restate(tw, T, y, sens, p, shared, w, gn=True)
    blank = mc < NCOLS
    for x, z in zip(a, b):
        assert np.isnan(x[..., blank]).all() and np.array_equal(x[..., ~blank], z[..., ~blank])
