// Least-squares fit objective on the device: per ensemble member the weighted sum of squares of (out - data) over every save point and output, its gradient with
// respect to the parameters and (k_out_fit_gn) the Gauss-Newton matrix, from ONE launch — out and d(out)/dp exist neither in device memory nor on the host.
//
//     L = sum w (out - data)^2        dL/dp_j = 2 sum w (out - data) dout/dp_j        GN_jl = 2 sum w dout/dp_j dout/dp_l
//
// (the objective of the reference's gradient example, examples/intro-logistic-closures/src/solve_adjoint_sens_sum_squares.rs: g = 2 (soln - data)).  Compiled by hiprtc
// behind the same generated source as dsh_out_sens_kernel.hpp (Target::HipOutSens: jit_out_component, jit_out_jac_component, jit_out_sens_component; kOutSensN,
// kOutSensNP, kOutSensNOut) as a module of its own per model (dsh_model_out_fit, dsh_jit.hip): neither the k_out_sens module nor an integrator module includes it.
// The translation unit defines DSH_OUT_FIT_GN for models with at most DSH_OUT_FIT_GN_MAX_NP parameters; only then k_out_fit_gn exists.
//
// Layout (b = member, fastest; c = save point / column; i = state; j, l = parameter; k = output):
//     y       [(c * n + i) * nb + b]                        in
//     sens    [j * sens_sj + c * sens_sc + i * nb + b]      in   (as k_out_sens: [j][c][i][b] or the resident integrators' [c][j][i][b], read in place)
//     p       [j * nb + b]                                  in
//     data    [c * nout + k] (shared by all members) or [(c * nout + k) * nb + b] (data_per_member)       in
//     weights [c * nout + k], or NULL: unweighted           in
//     loss    [b]                                           out
//     grad    [j * nb + b]                                  out
//     gn      [q * nb + b]                                  out  (k_out_fit_gn) upper triangle packed row-major: q counts the pairs (j, l), l >= j
// One thread per member, 256 per workgroup, a 1-D grid: the thread walks the columns, and the outputs inside a column, in order, so the order of every sum is fixed and
// a CPU restatement can repeat it bit for bit.  Every load is member-fastest — a wavefront reads 64 consecutive doubles of a row — and only the rows the output
// expressions name are touched, as in k_out_sens.  No LDS, no atomics, 64-bit indices; the 1 + np (+ np (np + 1) / 2) accumulators and the np tangents of the current
// (c, k) live in registers, so the state loads of an output are shared by its tangents.  The columns are NOT split across threads: a small ensemble with many save
// points leaves the device idle.
//
// Arithmetic (no contraction: every a + b * c is two rounded operations):
//     for c, for k:   d = data(c, k, b); if d is NaN: continue               (a missing observation contributes nothing: its terms are computed and selected out, not
//                                                                            branched around — whatever its inputs hold, NaN included, reaches no result)
//                     r = out_k - d;  wr = weights ? w(c, k) * r : r;  L = L + wr * r
//                     d_j = jac_component(S_j) + sens_component(E_j)           (the two roots added once, exactly as k_out_sens does)
//                     G_j = G_j + wr * d_j
//                     wd = weights ? w(c, k) * d_j : d_j;  H_jl = H_jl + wd * d_l   for l >= j
//     loss = L;  grad_j = 2 G_j;  gn_q = 2 H_jl
// member_cols (optional): a member with member_cols[b] < ncols did not produce every column: all of its results are NaN and none of its inputs are read.
#pragma once
#include <hip/hip_runtime.h>

#define DSH_OUT_FIT_GN_MAX_NP 8

namespace dsh {

template <bool GN>
__device__ __forceinline__ void out_fit_member(long long nb, long long ncols, const double* __restrict__ t_cols, const double* __restrict__ y, const double* __restrict__ sens,
                                               long long sens_sj, long long sens_sc, const double* __restrict__ p, const int* __restrict__ member_cols,
                                               const double* __restrict__ data, int data_per_member, const double* __restrict__ weights, double* __restrict__ loss,
                                               double* __restrict__ grad, double* __restrict__ gn) {
  constexpr int NP = kOutSensNP, NOUT = kOutSensNOut, NQ = GN ? NP * (NP + 1) / 2 : 1;
  constexpr long long N = kOutSensN;
  // the loops over the parameters index register arrays: unrolled unless the model has so many parameters that the accumulators cannot be registers anyway
  constexpr bool UNROLL_J = GN || NP <= 16, UNROLL_K = NOUT * NP <= 64;
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  if (member_cols && (long long)member_cols[b] < ncols) {
    const double nan = __builtin_nan("");
    loss[b] = nan;
    for (long long j = 0; j < NP; ++j) grad[j * nb + b] = nan;
    if constexpr (GN)
      for (long long q = 0; q < NQ; ++q) gn[q * nb + b] = nan;
    return;
  }
  double pv[NP], G[NP], H[NQ];
  double L = 0.0;
#pragma unroll
  for (int j = 0; j < NP; ++j) { pv[j] = p[(long long)j * nb + b]; G[j] = 0.0; }
#pragma unroll
  for (int q = 0; q < NQ; ++q) H[q] = 0.0;
  auto P = [&](long i) { return pv[i]; };
  for (long long c = 0; c < ncols; ++c) {
    const double t = t_cols[c];
    const double* __restrict__ yc = y + c * N * nb + b;
    const double* __restrict__ sc = sens + c * sens_sc + b;
    auto X = [&](long i) { return yc[(long long)i * nb]; };
    auto one_output = [&](int k) {
      const long long ck = c * NOUT + k;
      const double d = data_per_member ? data[ck * nb + b] : data[ck];
      const bool seen = d == d;  // NaN: a missing observation.  Selected out below instead of branched around: no divergence, and the state loads stay shared by the outputs
      const double w = weights ? weights[ck] : 0.0;
      const double r = jit_out_component(t, (long)k, X, P) - d;
      const double wr = weights ? w * r : r;
      const double Lc = L + wr * r;
      L = seen ? Lc : L;
      auto tangent = [&](int j) {
        const double* __restrict__ sj = sc + (long long)j * sens_sj;
        auto S = [&](long i) { return sj[(long long)i * nb]; };
        auto E = [&](long i) { return i == (long)j ? 1.0 : 0.0; };
        const double along_state = jit_out_jac_component(t, (long)k, X, S, P);
        const double along_param = jit_out_sens_component(t, (long)k, X, E, P);
        return along_state + along_param;
      };
      if constexpr (GN) {
        double dj[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) { dj[j] = tangent(j); const double Gc = G[j] + wr * dj[j]; G[j] = seen ? Gc : G[j]; }
        int q = 0;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          const double wd = weights ? w * dj[j] : dj[j];
#pragma unroll
          for (int l = j; l < NP; ++l, ++q) { const double Hc = H[q] + wd * dj[l]; H[q] = seen ? Hc : H[q]; }
        }
      } else if constexpr (UNROLL_J) {
#pragma unroll
        for (int j = 0; j < NP; ++j) { const double Gc = G[j] + wr * tangent(j); G[j] = seen ? Gc : G[j]; }
      } else {
#pragma nounroll
        for (int j = 0; j < NP; ++j) { const double Gc = G[j] + wr * tangent(j); G[j] = seen ? Gc : G[j]; }
      }
    };
    if constexpr (UNROLL_K) {
#pragma unroll
      for (int k = 0; k < NOUT; ++k) one_output(k);
    } else {
#pragma nounroll
      for (int k = 0; k < NOUT; ++k) one_output(k);
    }
  }
  loss[b] = L;
#pragma unroll
  for (int j = 0; j < NP; ++j) grad[(long long)j * nb + b] = 2.0 * G[j];
  if constexpr (GN) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) gn[(long long)q * nb + b] = 2.0 * H[q];
  }
}

// grid: ceil(nb / 256) workgroups of 256 threads
extern "C" __global__ void __launch_bounds__(256) k_out_fit(long long nb, long long ncols, const double* __restrict__ t_cols, const double* __restrict__ y,
                                                            const double* __restrict__ sens, long long sens_sj, long long sens_sc, const double* __restrict__ p,
                                                            const int* __restrict__ member_cols, const double* __restrict__ data, int data_per_member,
                                                            const double* __restrict__ weights, double* __restrict__ loss, double* __restrict__ grad) {
  out_fit_member<false>(nb, ncols, t_cols, y, sens, sens_sj, sens_sc, p, member_cols, data, data_per_member, weights, loss, grad, nullptr);
}

#ifdef DSH_OUT_FIT_GN
static_assert(kOutSensNP <= DSH_OUT_FIT_GN_MAX_NP, "k_out_fit_gn keeps np (np + 1) / 2 accumulators in registers: at most 8 parameters");
extern "C" __global__ void __launch_bounds__(256) k_out_fit_gn(long long nb, long long ncols, const double* __restrict__ t_cols, const double* __restrict__ y,
                                                               const double* __restrict__ sens, long long sens_sj, long long sens_sc, const double* __restrict__ p,
                                                               const int* __restrict__ member_cols, const double* __restrict__ data, int data_per_member,
                                                               const double* __restrict__ weights, double* __restrict__ loss, double* __restrict__ grad,
                                                               double* __restrict__ gn) {
  out_fit_member<true>(nb, ncols, t_cols, y, sens, sens_sj, sens_sc, p, member_cols, data, data_per_member, weights, loss, grad, gn);
}
#endif

}  // namespace dsh
