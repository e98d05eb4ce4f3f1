"""The CPU restatement of the fit-objective kernel (csrc/dsh_out_fit_kernel.hpp; tests/test_out_fit_ref.py, tests/test_gpu_out_fit.py).

out and d(out)/dp come from out_sens_models.HostTwin.evaluate (the front end's own host twin, which tests/test_diffsl_out_sens.py holds to hand-written derivatives and
central differences); the accumulation is the kernel's, restated here: columns in order, outputs in order inside a column, vectorised over the members, and ONE IEEE
operation per numpy call, so nothing contracts and the results repeat the device's bit for bit.

    L = 0; G_j = 0; H_jl = 0
    for c, for k:   d = data(c, k, b); a NaN is a missing observation: nothing is added
                    r = out - d;  wr = w r (weights) or r;  L = L + wr r
                    G_j = G_j + wr d_j
                    wd = w d_j (weights) or d_j;  H_jl = H_jl + wd d_l   (l >= j)
    loss = L;  grad_j = 2 G_j;  gn_q = 2 H_jl   (q counts the pairs (j, l), l >= j, row-major)"""
import numpy as np


def accumulate(out, dout, data, weights=None, member_cols=None, gn=False):
    """device layouts: out [ncols, nout, nb], dout [np, ncols, nout, nb]; data [ncols, nout] (shared) or [ncols, nout, nb]; weights [ncols, nout] or None
    -> loss [nb], grad [np, nb] and, if gn, the packed upper triangle [np (np + 1) / 2, nb].  Members with member_cols[b] < ncols: NaN everywhere."""
    out, dout, data = np.asarray(out, dtype=float), np.asarray(dout, dtype=float), np.asarray(data, dtype=float)
    ncols, nout, nb = out.shape
    npar = dout.shape[0]
    assert dout.shape == (npar, ncols, nout, nb) and data.shape in ((ncols, nout), (ncols, nout, nb))
    assert weights is None or np.shape(weights) == (ncols, nout)
    pairs = [(j, l) for j in range(npar) for l in range(j, npar)]
    L, G, H = np.zeros(nb), np.zeros((npar, nb)), np.zeros((len(pairs), nb))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(ncols):
            for k in range(nout):
                d = np.broadcast_to(data[c, k], (nb,))
                seen = ~np.isnan(d)
                r = out[c, k] - d
                wr = weights[c, k] * r if weights is not None else r
                L = np.where(seen, L + wr * r, L)
                for j in range(npar):
                    G[j] = np.where(seen, G[j] + wr * dout[j, c, k], G[j])
                if gn:
                    for q, (j, l) in enumerate(pairs):
                        wd = weights[c, k] * dout[j, c, k] if weights is not None else dout[j, c, k]
                        H[q] = np.where(seen, H[q] + wd * dout[l, c, k], H[q])
        loss, grad, gnp = L, 2.0 * G, 2.0 * H
    if member_cols is not None:
        blank = np.asarray(member_cols) < ncols
        loss[blank], grad[:, blank], gnp[:, blank] = np.nan, np.nan, np.nan
    return (loss, grad, gnp) if gn else (loss, grad)


def restate(tw, t_cols, y, sens, p, data, weights=None, member_cols=None, gn=False):
    """the whole kernel: HostTwin `tw` on y [ncols, n, nb], sens [np, ncols, n, nb], p [np, nb], then the accumulation"""
    out, dout = tw.evaluate(t_cols, y, sens, p, member_cols=member_cols)
    return accumulate(out, dout, data, weights, member_cols, gn)


def unpack(gnp, npar):
    """packed upper triangle [np (np + 1) / 2, nb] -> full symmetric [nb, np, np]"""
    full = np.empty((gnp.shape[1], npar, npar))
    q = 0
    for j in range(npar):
        for l in range(j, npar):
            full[:, j, l] = full[:, l, j] = gnp[q]
            q += 1
    return full


def from_solver_outputs(out, dout, data, weights=None, gn=False):
    """the layouts of Solver.solve_dense_sens_outputs / solve_dense_sens_fit: out [nt, nb, nout], dout [np, nt, nb, nout], data [nt, nout] or [nt, nb, nout]
    -> loss [nb], grad [nb, np][, gn [nb, np, np]]"""
    data = np.asarray(data, dtype=float)
    r = accumulate(np.transpose(out, (0, 2, 1)), np.transpose(dout, (0, 1, 3, 2)), np.transpose(data, (0, 2, 1)) if data.ndim == 3 else data, weights, None, gn)
    return (r[0], np.ascontiguousarray(r[1].T)) + ((unpack(r[2], dout.shape[0]),) if gn else ())
