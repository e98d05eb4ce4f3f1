// Output sensitivities on the device: out_i and d(out_i)/dp_j at every save point of every ensemble member from ONE launch.
//
// The reference's solve_dense_sensitivities (crates/diffsol/src/ode_solver/sensitivities.rs:360-397) returns, for a model with an out_i, per save point and
// parameter j
//     out.jac_mul(y, s_j) + out.sens_mul(y, e_j)
// — the tangent of the outputs along the state sensitivity s_j plus their explicit dependence on parameter j.  This header is compiled by hiprtc behind the source the
// DiffSL front end generates for Target::HipOutSens (diffsol_amd/host/diffsl.hpp: jit_out_component, jit_out_jac_component, jit_out_sens_component over accessors
// X(i), V(i), P(i); constants kOutSensN, kOutSensNP, kOutSensNOut), as its own module per model: the integrator modules never include it, so their code objects do
// not depend on it, and a model that never asks for output sensitivities never pays for the compilation (dsh_model_set_out_sens_source / dsh_model_out_sens, dsh_jit.hip).
//
// Layout (b = member, fastest everywhere; c = save point / column; i = state; j = parameter; k = output):
//     y    [(c * n + i) * nb + b]                          in
//     sens [j * sens_sj + c * sens_sc + i * nb + b]        in   (sens_sj = ncols n nb, sens_sc = n nb: [j][c][i][b]; the resident integrators write [c][j][i][b])
//     p    [j * nb + b]                                    in
//     out  [(c * nout + k) * nb + b]                       out
//     dout [((j * ncols + c) * nout + k) * nb + b]         out
// One thread per (b, c): a wavefront reads and writes 64 consecutive doubles (512 bytes) of a row in every access.  No LDS, nothing shared between threads.  The
// accessors read only the states (and sensitivity components) the output expressions name: a terminal voltage that depends on two surface concentrations touches
// two state rows and two sensitivity rows per parameter of the 42 the battery model has.  Both loops (outputs outside, parameters inside) have compile-time bounds and
// are unrolled for small models, so the state loads of an output are shared by its np tangents; rolled, the repeated loads of a thread hit the same lines again.
//
// Arithmetic: the two terms are evaluated as separate expression roots and added ONCE, always — also when one of them is the structural zero (emitted as the literal
// 0.0) — so the host twin (Target::HostOutSens: dsl_out_jac_mul(x, s_j) + dsl_out_sens_mul(x, e_j)) performs the same operations in the same order; compiled without
// contraction like every exact kernel.  The unit vector e_j never exists in memory: V(i) = (i == j ? 1.0 : 0.0) in registers.
//
// member_cols (optional): member b produced columns 0 .. member_cols[b] - 1 only (a failed or stopped member); the others are written as NaN in both outputs and their
// inputs are not read.
#pragma once
#include <hip/hip_runtime.h>

namespace dsh {

template <bool UNROLL>
__device__ __forceinline__ void out_sens_point(double t, long long nb, long long ncols, long long b, long long c, const double* __restrict__ yc, const double* __restrict__ sc,
                                               long long sens_sj, const double (&pv)[kOutSensNP], double* __restrict__ out, double* __restrict__ dout) {
  constexpr long long NOUT = kOutSensNOut;
  auto X = [&](long i) { return yc[(long long)i * nb]; };
  auto P = [&](long i) { return pv[i]; };
  auto one_output = [&](int k) {
    out[((long long)c * NOUT + k) * nb + b] = jit_out_component(t, (long)k, X, P);
    auto one_param = [&](int j) {
      const double* __restrict__ sj = sc + (long long)j * sens_sj;
      auto S = [&](long i) { return sj[(long long)i * nb]; };
      auto E = [&](long i) { return i == (long)j ? 1.0 : 0.0; };
      const double along_state = jit_out_jac_component(t, (long)k, X, S, P);
      const double along_param = jit_out_sens_component(t, (long)k, X, E, P);
      dout[(((long long)j * ncols + c) * NOUT + k) * nb + b] = along_state + along_param;
    };
    if constexpr (UNROLL) {
#pragma unroll
      for (int j = 0; j < kOutSensNP; ++j) one_param(j);
    } else {
#pragma nounroll
      for (int j = 0; j < kOutSensNP; ++j) one_param(j);
    }
  };
  if constexpr (UNROLL) {
#pragma unroll
    for (int k = 0; k < kOutSensNOut; ++k) one_output(k);
  } else {
#pragma nounroll
    for (int k = 0; k < kOutSensNOut; ++k) one_output(k);
  }
}

// grid: (ceil(nb / blockDim.x), min(ncols, 65535)); columns beyond the grid's second extent are walked by the same threads
extern "C" __global__ void __launch_bounds__(256) k_out_sens(long long nb, long long ncols, const double* __restrict__ t_cols, const double* __restrict__ y,
                                                             const double* __restrict__ sens, long long sens_sj, long long sens_sc, const double* __restrict__ p,
                                                             const int* __restrict__ member_cols, double* __restrict__ out, double* __restrict__ dout) {
  constexpr long long N = kOutSensN, NP = kOutSensNP, NOUT = kOutSensNOut;
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  double pv[kOutSensNP];
#pragma unroll
  for (int j = 0; j < kOutSensNP; ++j) pv[j] = p[(long long)j * nb + b];
  const long long mine = member_cols ? (long long)member_cols[b] : ncols;
  for (long long c = blockIdx.y; c < ncols; c += gridDim.y) {
    if (c >= mine) {
      const double nan = __builtin_nan("");
      for (long long k = 0; k < NOUT; ++k) {
        out[(c * NOUT + k) * nb + b] = nan;
        for (long long j = 0; j < NP; ++j) dout[((j * ncols + c) * NOUT + k) * nb + b] = nan;
      }
      continue;
    }
    out_sens_point<(kOutSensNOut * kOutSensNP <= 64)>(t_cols[c], nb, ncols, b, c, y + c * N * nb + b, sens + c * sens_sc + b, sens_sj, pv, out, dout);
  }
}

}  // namespace dsh
