"""Models and the CPU checker of the output-sensitivity tests (tests/test_diffsl_out_sens.py, tests/test_gpu_out_sens.py).

The checker is the product front end's own host twin (Target::HostOutSens: dsl_out, dsl_out_jac_mul, dsl_out_sens_mul) compiled with g++ and the flags of
diffsl_models.host_model_so, plus a loop written here that evaluates it per member and column in the device layouts — the same operations in the same order as
csrc/dsh_out_sens_kernel.hpp: out_jac_mul(x, s_j) and out_sens_mul(x, e_j) as separate roots, added once."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import diffsl_models as D

# in = [k, y0], two states, three outputs: only + - * /
RATIONAL = """
in = [k, y0]
u_i { x = y0, y = 1 }
F_i { -k * x, -y }
out_i { k*x*y + y0, x / (y + k), x + y }
"""

# the same shape with smooth elementary functions (no open-circuit fits: their steep tanh terms make finite differences useless)
TRANSCENDENTAL = """
in = [k, y0]
u_i { x = y0, y = 1 }
F_i { -k * x, -y }
out_i { exp(-k*x) * sin(y + y0), sqrt(x*x + k) / (1 + y*y), pow(x, 1.5) * tanh(k*y) }
"""

# exponential decay of tests/test_gpu_resident_sens.py with outputs that mix states and parameters
DECAY = "in_i { k = 0.1, y0 = 1.0 }\nu_i { x = y0, y = y0 }\nF_i { -k * u_i }\nout_i { x + y, k * x }\n"

ROBERTSON_DAE_OUT = D.ROBERTSON_DAE.replace("out_i { x, y, z, x + y + z }", "out_i { x + y + z, k1 * x }")


def spm_out():
    """the single-particle battery model (n = 42, one parameter) with a voltage-like output through the sparse surface-concentration tensors, and one plain one"""
    return D.spm(20, no_stops=True) + "out_i { 2.0 * tanh(3.0 - 5.0 * sp_i) + 0.05 * arcsinh(current / sqrt(sn_i * (1.0 - sn_i))), sn_i }\n"


_LOOP = r"""
extern "C" void ref_out_sens(long nb, long ncols, int n, int np, int nout, const double* t_cols, const double* y, const double* sens, const double* p,
                             const int* member_cols, double* out, double* dout) {
  double x[512], s[512], pv[64], e[64], g[256], gj[256], gs[256];
  const double nan = __builtin_nan("");
  for (long c = 0; c < ncols; ++c)
    for (long b = 0; b < nb; ++b) {
      if (member_cols && c >= member_cols[b]) {
        for (int k = 0; k < nout; ++k) { out[(c * nout + k) * nb + b] = nan; for (int j = 0; j < np; ++j) dout[((j * ncols + c) * nout + k) * nb + b] = nan; }
        continue;
      }
      for (int i = 0; i < n; ++i) x[i] = y[(c * n + i) * nb + b];
      for (int j = 0; j < np; ++j) pv[j] = p[j * nb + b];
      dsl_out(t_cols[c], x, pv, g);
      for (int k = 0; k < nout; ++k) out[(c * nout + k) * nb + b] = g[k];
      for (int j = 0; j < np; ++j) {
        for (int i = 0; i < n; ++i) s[i] = sens[((j * ncols + c) * n + i) * nb + b];
        for (int q = 0; q < np; ++q) e[q] = q == j ? 1.0 : 0.0;
        dsl_out_jac_mul(t_cols[c], x, pv, s, gj);
        dsl_out_sens_mul(t_cols[c], x, pv, e, gs);
        for (int k = 0; k < nout; ++k) dout[((j * ncols + c) * nout + k) * nb + b] = gj[k] + gs[k];
      }
    }
}
"""


class HostTwin:
    """the compiled host out-sens source of a DiffSL text"""

    def __init__(self, code):
        from diffsol_amd import diffsl
        src, d, _ = diffsl.generate(code, diffsl.TARGET_HOST_OUT_SENS)
        self.source = src
        self.n, self.np, self.nout = d["n"], d["nparams"], d["nout"]
        assert self.n <= 512 and self.np <= 64 and self.nout <= 256
        flags = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"]
        full = src + _LOOP
        key = hashlib.sha1((full + "#" + " ".join(flags)).encode()).hexdigest()[:20]
        so = os.path.join(D.HOST_MODEL_DIR, "out_sens_" + key + ".so")
        if not os.path.exists(so):
            os.makedirs(D.HOST_MODEL_DIR, exist_ok=True)
            with tempfile.TemporaryDirectory(prefix="dsl_out_sens_") as d_:
                cpp, tmp = os.path.join(d_, "model.cpp"), os.path.join(d_, "libmodel.so")
                with open(cpp, "w") as f:
                    f.write(full)
                subprocess.run(["g++"] + flags + ["-I", os.path.join(D.ROOT, "include"), "-o", tmp, cpp], check=True)
                os.replace(tmp, so + ".tmp%d" % os.getpid())
                os.replace(so + ".tmp%d" % os.getpid(), so)
        self.lib = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        self.lib.dsl_out.argtypes = [C.c_double, dp, dp, dp]
        self.lib.dsl_out_jac_mul.argtypes = [C.c_double, dp, dp, dp, dp]
        self.lib.dsl_out_sens_mul.argtypes = [C.c_double, dp, dp, dp, dp]
        self.lib.ref_out_sens.argtypes = [C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, C.POINTER(C.c_int), dp, dp]
        for f in (self.lib.dsl_out, self.lib.dsl_out_jac_mul, self.lib.dsl_out_sens_mul, self.lib.ref_out_sens):
            f.restype = None

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(C.POINTER(C.c_double))

    def out(self, t, x, p):
        x, p, g = np.ascontiguousarray(x, dtype=float), np.ascontiguousarray(p, dtype=float), np.empty(self.nout)
        self.lib.dsl_out(t, self._p(x), self._p(p), self._p(g))
        return g

    def jac_mul(self, t, x, p, v):
        x, p, v, g = (np.ascontiguousarray(a, dtype=float) for a in (x, p, v, np.empty(self.nout)))
        self.lib.dsl_out_jac_mul(t, self._p(x), self._p(p), self._p(v), self._p(g))
        return g

    def sens_mul(self, t, x, p, v):
        x, p, v, g = (np.ascontiguousarray(a, dtype=float) for a in (x, p, v, np.empty(self.nout)))
        self.lib.dsl_out_sens_mul(t, self._p(x), self._p(p), self._p(v), self._p(g))
        return g

    def evaluate(self, t_cols, y, sens, p, member_cols=None):
        """device layouts: y [ncols, n, nb], sens [np, ncols, n, nb], p [np, nb] -> out [ncols, nout, nb], dout [np, ncols, nout, nb]"""
        t_cols, y, sens, p = (np.ascontiguousarray(a, dtype=float) for a in (t_cols, y, sens, p))
        ncols, n, nb = y.shape
        assert n == self.n and sens.shape == (self.np, ncols, n, nb) and p.shape == (self.np, nb) and t_cols.shape == (ncols,)
        out, dout = np.empty((ncols, self.nout, nb)), np.empty((self.np, ncols, self.nout, nb))
        mc = None if member_cols is None else np.ascontiguousarray(member_cols, dtype=np.int32)
        self.lib.ref_out_sens(nb, ncols, n, self.np, self.nout, self._p(t_cols), self._p(y), self._p(sens), self._p(p),
                              mc.ctypes.data_as(C.POINTER(C.c_int)) if mc is not None else None, self._p(out), self._p(dout))
        return out, dout
