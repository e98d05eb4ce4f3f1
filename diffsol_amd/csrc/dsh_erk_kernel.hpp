// Device-resident explicit Runge-Kutta integrator, Tsit45 (launch code and documentation: dsh_erk_resident.hip).  In a header so that run-time-compiled model
// modules (dsh_jit.hip) instantiate the same kernel for user models.
#pragma once
#include "dsh_resident.hpp"

namespace dsh {

constexpr int kErkStages = 7, kErkPoly = 4, kErkOrder = 4;

// Tableau::tsit45 (crates/diffsol/src/ode_solver/tableau.rs:161-304).  The numbers below are data of the method; tests/test_erk_ref_golden.py parses the lines between
// the two markers and compares them with tests/golden/reference_tsit45.json.  The first column of `a` is not typed in: the reference computes it as
// a(i,0) = c(i) - (a(i,1) + ... + a(i,i-1)), summed left to right from zero (tableau.rs:221-227), and so does erk_a() below.
// TSIT45-TABLEAU-BEGIN
constexpr double kTsitC[7] = {0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0};
constexpr double kTsitB[7] = {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774, 0.0};
constexpr double kTsitD[7] = {-0.001780011052225777, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552, -0.45808210592918697, 0.015151515151515152};
// a(i,j) for 1 <= j < i <= 5, row by row: a21 | a31 a32 | a41 a42 a43 | a51 a52 a53 a54
constexpr double kTsitALower[10] = {0.335480655492357, -6.359448489975075, 4.362295432869581, -11.74888356406283, 7.495539342889836, -0.09249506636175525, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.02826905039406838};
// dense output: b_i(theta) = sum_q beta[q][i] theta^(q+1)
constexpr double kTsitBeta[4][7] = {
    {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {-2.76370619727483, 0.1317, 3.93029623689475, -12.4110771669337, 37.509313416511, -27.8965262891973, 1.5},
    {2.91325546182191, -0.2234, -5.9410338721315, 30.3381886302823, -88.1789048947664, 65.0918946747937, -4.0},
    {-1.05308849772902, 0.1017, 2.49062728565125, -16.5481028892449, 47.3795219628193, -34.8706578614966, 2.5}};
// TSIT45-TABLEAU-END

// a(i, j), i = 1..6, j < i (row 6 = b: first same as last)
__host__ __device__ constexpr double erk_a(int i, int j) {
  if (i == 6) return kTsitB[j];
  const int row0 = (i - 2) * (i - 1) / 2;  // kTsitALower offset of row i (i >= 2)
  if (j >= 1) return kTsitALower[row0 + j - 1];
  double a_sum = 0.0;
  for (int q = 1; q < i; ++q) a_sum += kTsitALower[row0 + q - 1];
  return kTsitC[i] - a_sum;
}

struct ErkConsts {
  ResidentConsts r;
  // ExplicitRkConfig (config.rs:132-160): the four step-size bounds of Rk::factor
  double min_shrink, max_shrink, min_growth, max_growth;
  // OdeSolverMethod::solve (method.rs:227-258 over :881-961): steps_cap > 0 makes the launch write the state after EVERY accepted step (y_out [steps_cap][N][nb],
  // steps_t_out [steps_cap][nb]; columns beyond steps_cap are counted, not stored) instead of interpolating at save points
  double* steps_t_out;
  int steps_cap, steps_pad;
  // Forward sensitivities (k_erk_resident<.., SENS = true>; problem.tsit45_sens(), explicit_rk.rs:46-54): s_j = dy/dp_j of every parameter integrated alongside.
  // The fields have the meaning of AdaptiveConsts' (dsh_adaptive_kernel.hpp): sens_out n_eval x NP x N x nb (device, batch-fastest); sens_error_control != 0: the
  // sensitivities take part in the error test with sens_rtol / sens_atol (SensEquations::include_in_error_control), else they do not; sens_pad = 1: sens_atol[0] for
  // every state.  Appended: a kernel without sensitivities never reads them.
  double* sens_out;
  double sens_rtol, sens_atol[4];
  int sens_error_control, sens_pad;
  // Integrated outputs (k_erk_resident<.., INTOUT = true>; OdeBuilder::integrate_out(true)): g(t) = integral of out(y, t) carried by the solver state, y_out holds g.
  // out_error_control != 0 (output tolerances were given, output_in_error_control): g takes part in the error test with out_rtol / out_atol, else it does not;
  // out_pad = 1: out_atol[0] for every output.  Appended: a kernel without integrated outputs never reads them.
  double out_rtol, out_atol[8];
  int out_error_control, out_pad;
};

// Doubles a lane keeps: 14 N without sensitivities (7 stage increments, y, dy, old_y, stage point, stage derivative, error vector, atol), 12 N more per parameter
// with them (7 stage increments, s, ds, old_s, stage point, stage derivative).  The plain kernel's largest instantiation (N = 8: 112 doubles) compiles without
// scratch memory; a model with forward sensitivities is admitted up to the same count.
constexpr int kErkMaxLaneDoubles = 112;
__host__ __device__ constexpr bool erk_sens_admitted(int64_t n, int64_t np) { return n >= 1 && np >= 1 && n * (14 + 12 * np) <= kErkMaxLaneDoubles; }
// Integrated outputs (INTOUT): 12 doubles more per output (7 increments, g, old_g, dg, the error entry, out_atol), within the same count; at most 8 outputs
// (ErkConsts::out_atol).  nout_e: the model's out_i count, or its state count when it has none (identity output).  No sensitivities; root functions are allowed.
constexpr int kErkMaxOut = 8;
__host__ __device__ constexpr bool erk_out_admitted(int64_t n, int64_t nout_e) {
  return n >= 1 && nout_e >= 1 && nout_e <= kErkMaxOut && 14 * n + 12 * nout_e <= kErkMaxLaneDoubles;
}
template <class Mdl> constexpr int erk_nout_e() { return model_nout<Mdl>::value > 0 ? model_nout<Mdl>::value : Mdl::N; }
// out(y, t): out_i of the model, the state itself for a model without (state.rs:1097-1103)
template <class Mdl, int NO>
__device__ __forceinline__ void erk_out(double t, const double (&y)[Mdl::N], const double (&p)[Mdl::NP], double (&o)[NO]) {
  if constexpr (model_nout<Mdl>::value > 0) Mdl::out(t, y, p, o);
  else {
DSH_UNROLL_N
    for (int i = 0; i < NO; ++i) o[i] = y[i];
  }
}

// The gemv that every stage point, error vector and dense output is (nalgebra's order, as the checkers restate it): ret = d[:, 0..n) c accumulated from column 0
// upward, every term 1.0 * d[j][r] * c[j]; with a base vector ret = base + d[:, 0..n) c, the base added in the first term.  `c` is anything indexable: a tableau row
// (kTsitD: error_norm, runge_kutta.rs:783-822; kTsitB: the accepted g, :900-909), the beta function of a save point (interpolate_from_diff, :962-966), or a(i, .) of
// stage i (ErkRowA: do_stage, :537-607).
struct ErkRowA {
  int i;
  __device__ constexpr double operator[](int j) const { return erk_a(i, j); }
};
template <int R, class Row>
__device__ __forceinline__ void erk_fold(const Row& c, int n, const double (&d)[kErkStages][R], double (&ret)[R]) {
DSH_UNROLL_N
  for (int r = 0; r < R; ++r) {
    double acc = 1.0 * d[0][r] * c[0];
#pragma unroll
    for (int j = 1; j < n; ++j) acc = 1.0 * d[j][r] * c[j] + acc;
    ret[r] = acc;
  }
}
template <int R, class Row>
__device__ __forceinline__ void erk_fold(const Row& c, int n, const double (&base)[R], const double (&d)[kErkStages][R], double (&ret)[R]) {
DSH_UNROLL_N
  for (int r = 0; r < R; ++r) {
    double acc = 1.0 * d[0][r] * c[0] + 1.0 * base[r];
#pragma unroll
    for (int j = 1; j < n; ++j) acc = 1.0 * d[j][r] * c[j] + acc;
    ret[r] = acc;
  }
}
// interpolate_beta_function (runge_kutta.rs:968-981) inside the last step [old_t, t].  Apart from its application, because the kernel with sensitivities computes it
// once per save point and applies it to the state and to every sensitivity (interpolate_sens_inplace, :1237-1309).
__device__ __forceinline__ void erk_beta_function(double t, double old_t, double tt, double (&bf)[kErkStages]) {
  const double dt = t - old_t;
  const double theta = dt == 0.0 ? 1.0 : (tt - old_t) / dt;
  double thetav[kErkPoly];
  thetav[0] = theta;
#pragma unroll
  for (int q = 1; q < kErkPoly; ++q) thetav[q] = theta * thetav[q - 1];
#pragma unroll
  for (int i = 0; i < kErkStages; ++i) {
    double acc = 1.0 * kTsitBeta[0][i] * thetav[0];
#pragma unroll
    for (int q = 1; q < kErkPoly; ++q) acc = 1.0 * kTsitBeta[q][i] * thetav[q] + acc;
    bf[i] = acc;
  }
}
// interpolate_inplace (runge_kutta.rs:1080-1127; for g interpolate_out_inplace, :1185-1235): the beta function of tt applied to (base, d) of the last step
template <int R>
__device__ __forceinline__ void erk_interpolate(double t, double old_t, double tt, const double (&base)[R], const double (&d)[kErkStages][R], double (&ret)[R]) {
  double bf[kErkStages];
  erk_beta_function(t, old_t, tt, bf);
  erk_fold(bf, kErkStages, base, d, ret);
}
// The two output layouts, each address written once: column `col` of y_out [col][R][nb] (R rows: the states, or the integrated outputs) and the block of parameter j
// in column `col` of sens_out [col][np][N][nb].  The lanes that shadow a member store nothing.
template <int R>
__device__ __forceinline__ void erk_write_col(double* __restrict__ y_out, int64_t nb, int64_t b, bool active, int col, const double (&v)[R]) {
DSH_UNROLL_N
  for (int i = 0; i < R; ++i) if (active) y_out[((int64_t)col * R + i) * nb + b] = v[i];
}
template <int N>
__device__ __forceinline__ void erk_write_sens(double* __restrict__ sens_out, int64_t nb, int64_t b, bool active, int col, int np, int j, const double (&v)[N]) {
DSH_UNROLL_N
  for (int i = 0; i < N; ++i) if (active) sens_out[(((int64_t)col * np + j) * N + i) * nb + b] = v[i];
}
// what a column of y_out holds: g with integrated outputs, y without
template <bool INTOUT, class G, class Y>
__device__ __forceinline__ auto& erk_column(G& g, Y& y) {
  if constexpr (INTOUT) return g;
  else return y;
}

// One lane per member: ExplicitRk::step (explicit_rk.rs:196-243) over the Rk core (runge_kutta.rs), root finding on the dense output, tstop, solve_dense /
// solve.  Per lane: the 7 stage increments (diff, 7 x N), state and old state (y, dy, old_y), the error vector and the controller's scalars — no LDS.
// The register allocator picks the occupancy (no waves-per-SIMD attribute): see DESIGN.md for the compiler's numbers.
// SENS: ExplicitRk<.., SensEquations> — per parameter j the stage increments sdiff_j, s_j, ds_j, old_s_j and the stage point and its derivative, all in registers
// (every loop over the parameters is unrolled: no array is indexed at run time); models within erk_sens_admitted() only.
// INTOUT: problem.integrate_out — g = integral of out(y, t), with its own stage increments gdiff, carried like the state (runge_kutta.rs:529-533, :568-575, :802-810,
// :900-909, :1185-1235); y_out holds g, NOUT_E rows per column in place of N; models within erk_out_admitted() only, without SENS.
template <class Mdl, bool BA, bool WAVE, bool SENS = false, bool INTOUT = false>
__global__ __launch_bounds__(64) void k_erk_resident(int64_t nb, const double* __restrict__ p_g, const double* __restrict__ atol_g, const ErkConsts* __restrict__ Cp,
                                                     const double* __restrict__ t_eval, double* __restrict__ y_out, int32_t* __restrict__ stats_out,
                                                     int32_t* __restrict__ status_out, double* __restrict__ t_root_out, int32_t* __restrict__ root_idx_out,
                                                     int32_t* __restrict__ ncols_out, unsigned long long* __restrict__ totals) {
  constexpr int N = Mdl::N, NP = Mdl::NP, NR = Mdl::NROOTS > 0 ? Mdl::NROOTS : 1, S = kErkStages;
  static_assert(!Mdl::HAS_MASS, "explicit Runge-Kutta methods take no mass matrix (MassMatrixNotSupported, runge_kutta.rs:236-239)");
  static_assert(!SENS || Mdl::NROOTS == 0, "device-resident Tsit45 with forward sensitivities: models without root functions");
  static_assert(!SENS || erk_sens_admitted(Mdl::N, Mdl::NP), "device-resident Tsit45 with forward sensitivities: N (14 + 12 NP) <= 112 doubles per lane");
  static_assert(!INTOUT || (!SENS && erk_out_admitted(Mdl::N, erk_nout_e<Mdl>())), "device-resident Tsit45 with integrated outputs: 14 N + 12 NOUT <= 112 doubles per lane, NOUT <= 8, no sensitivities");
  const ErkConsts& T = *Cp;
  const ResidentConsts& C = T.r;
  const dsh_adaptive_options& o = C.o;
  const int64_t bglobal = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool active = bglobal < nb;  // the other lanes shadow the wavefront's first member (no stores): invisible in the group reductions
  const int64_t b = active ? bglobal : (int64_t)blockIdx.x * 64;
  const double rtol = C.rtol;
  double p[NP], atol[N];
  load_vec<NP>(p_g, nb, b, p);
DSH_UNROLL_N
  for (int i = 0; i < N; ++i) atol[i] = BA ? atol_g[i] : atol_g[(int64_t)i * nb + b];

  // ------------------------------------------------------------ RkState::new_and_consistent(problem, tableau.order())
  int32_t status = kRsOk;
  double t = C.t0, h = 0.0;
  double y[N], dy[N];
  Mdl::init(t, p, y);
  Mdl::rhs(t, y, p, dy);
  const bool det = o.deterministic_pow != 0;
  h = initial_step_size<Mdl, WAVE>(t, C.h0, y, dy, p, atol, rtol, kErkOrder, det);

  // ------------------------------------------------------------ Rk::_new (runge_kutta.rs:107-194)
  double diff[S][N];
#pragma unroll
  for (int j = 0; j < S; ++j)
DSH_UNROLL_N
    for (int i = 0; i < N; ++i) diff[j][i] = 0.0;
  double old_y[N], old_t = t;  // old_state (its dy and h are never read)
DSH_UNROLL_N
  for (int i = 0; i < N; ++i) old_y[i] = y[i];
  double g0[NR] = {0.0};
  double rf_t0 = t;
  if constexpr (Mdl::NROOTS > 0) Mdl::root(t, y, p, g0);
  bool has_prev_err = false;
  double prev_err = 0.0;
  int n_steps = 0, n_err_fails = 0;

  // ------------------------------------------------------------ RkState::new_with_sensitivities (state.rs:1001-1029), Rk::new_augmented
  // s_j = SensInit(t0) e_j, ds_j = SensRhs(s_j) about (y0, t0) = J(y0) s_j + (df/dp) e_j (sens_equations.rs:168-174: the Jacobian product first); the step size
  // above is the state equations' alone
  constexpr int NPS = SENS ? NP : 1, NS = SENS ? N : 1, SS = SENS ? S : 1;
  double sdiff[NPS][SS][NS], s[NPS][NS], ds[NPS][NS], old_s[NPS][NS], s_atol[NS];
  // old_state.s / old_state.ds: the stage point of every sensitivity and its derivative.  Declared here and not next to sy / sdy in the step loop: an array in that
  // scope, even unused, changes the schedule of the SENS = false kernel, which is to stay the kernel it was (profiles/erk_tsit45_sens.md)
  double ss[NPS][NS], sds[NPS][NS];
  if constexpr (SENS) {
DSH_UNROLL_N
    for (int i = 0; i < N; ++i) s_atol[i] = T.sens_atol[T.sens_pad != 0 ? 0 : (i < 4 ? i : 0)];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      double ev[NP], jm[N], dfdp[N];
#pragma unroll
      for (int k = 0; k < NP; ++k) ev[k] = k == j ? 1.0 : 0.0;
      Mdl::init_sens_mul(t, p, ev, s[j]);
      Mdl::sens_mul(t, y, p, ev, dfdp);
      Mdl::jac_mul(t, y, p, s[j], jm);
#pragma unroll
      for (int q = 0; q < S; ++q)
DSH_UNROLL_N
        for (int i = 0; i < N; ++i) sdiff[j][q][i] = 0.0;
DSH_UNROLL_N
      for (int i = 0; i < N; ++i) { ds[j][i] = jm[i] + dfdp[i]; old_s[j][i] = s[j][i]; }
    }
  }

  // ------------------------------------------------------------ integrate_out (state.rs:1097-1109): g = 0, dg = out(y0, t0); gdiff starts at zero like diff
  constexpr int NO = INTOUT ? erk_nout_e<Mdl>() : 1, SO = INTOUT ? S : 1;
  double gdiff[SO][NO], g[NO], old_g[NO], dg[NO], o_atol[NO];
  double sdg[NO];  // old_state.dg: out at the stage point (declared here for the reason given at ss / sds)
  if constexpr (INTOUT) {
    erk_out<Mdl, NO>(t, y, p, dg);
#pragma unroll
    for (int k = 0; k < NO; ++k) {
      g[k] = 0.0; old_g[k] = 0.0;
      o_atol[k] = T.out_atol[T.out_pad != 0 ? 0 : k];
#pragma unroll
      for (int q = 0; q < S; ++q) gdiff[q][k] = 0.0;
    }
  }

  // handle_tstop (runge_kutta.rs:752-781): 0 nothing, 1 reached, 2 StopTimeBeforeCurrentTime
  bool has_tstop = true;
  const double tstop = t_eval[C.n_eval - 1];
  auto handle_tstop = [&]() __attribute__((always_inline)) -> int {
    const double troundoff = 100.0 * kEps * (fabs(t) + fabs(h));
    if (fabs(t - tstop) <= troundoff) return 1;
    if ((h > 0.0 && tstop < t - troundoff) || (h < 0.0 && tstop > t + troundoff)) return 2;
    if ((h > 0.0 && t + h > tstop + troundoff) || (h < 0.0 && t + h < tstop - troundoff)) {
      const double factor = (tstop - t) / h;
      h *= factor;
    }
    return 0;
  };
  auto interpolate = [&](double tt, double (&ret)[N]) __attribute__((always_inline)) { erk_interpolate(t, old_t, tt, old_y, diff, ret); };  // the root finder's
  // What a column of y_out holds: NROW rows of g with INTOUT, of y without; (col_old, col_diff) is what its dense output interpolates
  constexpr int NROW = INTOUT ? NO : N;
  const double (&col_now)[NROW] = erk_column<INTOUT>(g, y);
  const double (&col_old)[NROW] = erk_column<INTOUT>(old_g, old_y);
  const double (&col_diff)[S][NROW] = erk_column<INTOUT>(gdiff, diff);
  auto column_at = [&](double tt, double (&ret)[NROW]) __attribute__((always_inline)) { erk_interpolate(t, old_t, tt, col_old, col_diff, ret); };

  int col = 0;
  double t_root = 0.0;
  int root_idx = -1;
  const bool steps_mode = !SENS && T.steps_cap > 0;  // every accepted step out (ErkConsts::steps_cap)
  auto steps_write = [&](double tw, const double (&v)[NROW]) __attribute__((always_inline)) {
    if (col < T.steps_cap) {
      if (active) T.steps_t_out[(int64_t)col * nb + b] = tw;
      erk_write_col(y_out, nb, b, active, col, v);
    }
    col++;
  };
  if (steps_mode) steps_write(t, col_now);  // write_out before the first step (method.rs:900); state.g = 0
  {  // set_stop_time (runge_kutta.rs:436-444); t_eval[0] >= t0 is checked on the host
    const int r = handle_tstop();
    if (r == 1) status = kRsStopTimeAtCurrentTime;
    else if (r == 2) status = kRsStopTimeBeforeCurrentTime;
  }

  long guard = 0;
  bool done = status != kRsOk || (!WAVE && !active);
  while (!done) {
    if (++guard > o.max_steps) { status = kRsMaxStepsExceeded; break; }
    // ================================================================ ExplicitRk::step (explicit_rk.rs:196-243)
    double hh = h;  // rk.start_step() (the state is never mutated between steps here)
    int nattempts = 0;
    double fac = 1.0, error_norm = 0.0;
    double sy[N], sdy[N];  // old_state.y / old_state.dy: the stage point and its derivative
    while (true) {
      // start_step_attempt (runge_kutta.rs:505-516): first same as last
DSH_UNROLL_N
      for (int r = 0; r < N; ++r) diff[0][r] = hh * dy[r];
      if constexpr (SENS) {  // :518-522
#pragma unroll
        for (int j = 0; j < NP; ++j)
DSH_UNROLL_N
          for (int r = 0; r < N; ++r) sdiff[j][0][r] = hh * ds[j][r];
      }
      if constexpr (INTOUT) {  // :529-533
#pragma unroll
        for (int k = 0; k < NO; ++k) gdiff[0][k] = hh * dg[k];
      }
#pragma unroll
      for (int i = 1; i < S; ++i) {
        // do_stage (runge_kutta.rs:537-566): old_state.y = y + diff[:, 0..i] a_row_i (nalgebra gemv order), diff[:, i] = h f(old_state.y, t + c_i h)
        const double ts = t + kTsitC[i] * hh;
        erk_fold(ErkRowA{i}, i, y, diff, sy);
        Mdl::rhs(ts, sy, p, sdy);
DSH_UNROLL_N
        for (int r = 0; r < N; ++r) diff[i][r] = hh * sdy[r];
        if constexpr (INTOUT) {  // :568-575: old_state.dg = out(old_state.y, t + c_i h), gdiff[:, i] = h old_state.dg
          erk_out<Mdl, NO>(ts, sy, p, sdg);
#pragma unroll
          for (int k = 0; k < NO; ++k) gdiff[i][k] = hh * sdg[k];
        }
        if constexpr (SENS) {  // :578-607: SensRhs about the stage point (sy, ts); old_state.s_j = s_j + sdiff_j[:, 0..i] a_row_i, sdiff_j[:, i] = h SensRhs(old_state.s_j)
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            double ev[NP], jm[N], dfdp[N];
#pragma unroll
            for (int k = 0; k < NP; ++k) ev[k] = k == j ? 1.0 : 0.0;
            erk_fold(ErkRowA{i}, i, s[j], sdiff[j], ss[j]);
            Mdl::sens_mul(ts, sy, p, ev, dfdp);
            Mdl::jac_mul(ts, sy, p, ss[j], jm);
DSH_UNROLL_N
            for (int r = 0; r < N; ++r) { sds[j][r] = jm[r] + dfdp[r]; sdiff[j][i][r] = hh * sds[j][r]; }
          }
        }
      }
      // error_norm (runge_kutta.rs:783-800): diff d, no linear solve
      double err[N];
      erk_fold(kTsitD, S, diff, err);
      error_norm = fmax(0.0, group_norm<WAVE>(wms<N>(err, y, atol, rtol)));
      if constexpr (INTOUT) {  // :802-810: gdiff d against state.g (the g at the start of the step) with the output tolerances, after the states' norm
        if (T.out_error_control) {
          double oerr[NO];
          erk_fold(kTsitD, S, gdiff, oerr);
          error_norm = fmax(error_norm, group_norm<WAVE>(wms<NO>(oerr, g, o_atol, T.out_rtol)));
        }
      }
      if constexpr (SENS) {  // :812-822: scaled by state.s_j at the start of the step; the states' norm, then j = 0, 1, ..
        if (T.sens_error_control) {
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            double serr[N];
            erk_fold(kTsitD, S, sdiff[j], serr);
            error_norm = fmax(error_norm, group_norm<WAVE>(wms<N>(serr, s[j], s_atol, T.sens_rtol)));
          }
        }
      }
      {  // Rk::factor (runge_kutta.rs:466-495) with safety_factor = 1
        const double safety = 0.9 * 1.0;
        double f = safety * pi_controller_raw(error_norm, has_prev_err, prev_err, o.pi_control_integral, o.pi_control_proportional, kErkOrder + 1, det);
        if (f > T.max_shrink && f < T.min_growth) f = 1.0;
        if (f < T.min_shrink) f = T.min_shrink;
        if (f > T.max_growth) f = T.max_growth;
        fac = f;
      }
      if (error_norm < 1.0) break;
      hh *= fac;
      nattempts += 1;
      has_prev_err = false;
      n_err_fails += 1;  // error_test_fail (runge_kutta.rs:843-867)
      if (nattempts >= o.max_error_test_failures) { status = kRsTooManyErrorTestFailures; break; }
      if (fabs(hh) < o.min_timestep) { status = kRsStepSizeTooSmall; break; }
    }
    if (status != kRsOk) break;
    prev_err = error_norm; has_prev_err = true;
    // ---- step_accepted(h, h * factor, rescale_dy = false) (runge_kutta.rs:894-960): old_state <- (last stage point, its derivative, t + h, new_h); swap
    {
      if constexpr (INTOUT) {  // :900-909: old_state.g = state.g + gdiff b (all seven terms: b, not row 6 of a), then the swap (which takes the last stage's dg along)
        erk_fold(kTsitB, S, g, gdiff, old_g);
#pragma unroll
        for (int k = 0; k < NO; ++k) { const double gk = g[k]; g[k] = old_g[k]; old_g[k] = gk; dg[k] = sdg[k]; }
      }
DSH_UNROLL_N
      for (int r = 0; r < N; ++r) { old_y[r] = y[r]; y[r] = sy[r]; dy[r] = sdy[r]; }
      if constexpr (SENS) {
#pragma unroll
        for (int j = 0; j < NP; ++j)
DSH_UNROLL_N
          for (int r = 0; r < N; ++r) { old_s[j][r] = s[j][r]; s[j][r] = ss[j][r]; ds[j][r] = sds[j][r]; }
      }
      const double nt = t + hh;
      old_t = t;
      t = nt;
      h = hh * fac;
    }
    n_steps += 1;
    int reason = 0;  // 0 internal, 1 tstop, 3 root
    if constexpr (Mdl::NROOTS > 0) {
      const int rr = check_root<Mdl, WAVE>(g0, rf_t0, y, t, p, interpolate, t_root, root_idx);
      if (rr == 2) { status = kRsRootBatchMismatch; break; }
      if (rr == 1) reason = 3;
    }
    if (reason == 0 && has_tstop) {
      const int r = handle_tstop();
      if (r == 2) { status = kRsStopTimeBeforeCurrentTime; break; }
      if (r == 1) { has_tstop = false; reason = 1; }
    }
    // ================================================================ solve_dense (method.rs:467-520) / solve (:881-961)
    const double upto = reason == 3 ? t_root : t;
    if (steps_mode) {  // InternalTimestep / TstopReached -> write_out: state.y (state.g with INTOUT); a root is written below, at the root
      if (reason != 3) steps_write(t, col_now);
    } else {
      while (col < C.n_eval && t_eval[col] <= upto) {
        double v[NROW];
        if constexpr (!SENS) {
          column_at(t_eval[col], v);
          erk_write_col(y_out, nb, b, active, col, v);
        } else {  // interpolate_sens_inplace (:1237-1309): one beta function for the state, old_state.s_j and sdiff_j.  The state's column is written first, and in
          // this branch: after the sensitivities' the compiler gives this kernel 16 vector registers more; with bf in the loop's scope the plain kernel's schedule changes
          double bf[S];
          erk_beta_function(t, old_t, t_eval[col], bf);
          erk_fold(bf, S, old_y, diff, v);
          erk_write_col(y_out, nb, b, active, col, v);
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            double sv[N];
            erk_fold(bf, S, old_s[j], sdiff[j], sv);
            erk_write_sens(T.sens_out, nb, b, active, col, NP, j, sv);
          }
        }
        col++;
      }
    }
    if (reason == 3) {  // state_mut_back(t_root) (:396-434): the column after the drained ones holds the state (g with INTOUT) at the root
      double v[NROW];
      column_at(t_root, v);
      if (steps_mode) steps_write(t_root, v);
      else if (col < C.n_eval) {
        erk_write_col(y_out, nb, b, active, col, v);
        col++;
      }
      done = true;
    }
    if (reason == 1) done = true;
  }
  if (active) {
    if (ncols_out != nullptr) ncols_out[b] = col;
    if (!steps_mode) {  // columns that were never reached (root stop or error exit): NaN
      double nan_col[NROW];
DSH_UNROLL_N
      for (int i = 0; i < NROW; ++i) nan_col[i] = __builtin_nan("");
      for (; col < C.n_eval; ++col) {
        erk_write_col(y_out, nb, b, active, col, nan_col);
        if constexpr (SENS) {  // NROW is N here
#pragma unroll
          for (int j = 0; j < NP; ++j) erk_write_sens(T.sens_out, nb, b, active, col, NP, j, nan_col);
        }
      }
    }
    if (status_out != nullptr) status_out[b] = status;
    if (t_root_out != nullptr) t_root_out[b] = root_idx >= 0 ? t_root : __builtin_nan("");
    if (root_idx_out != nullptr) root_idx_out[b] = root_idx;
    if (stats_out != nullptr) {  // the SDIRK layout: steps, Newton iterations, LU setups, error-test failures, Newton failures — an explicit method has no Newton, no LU
      stats_out[0 * nb + b] = n_steps;
      stats_out[1 * nb + b] = 0;
      stats_out[2 * nb + b] = 0;
      stats_out[3 * nb + b] = n_err_fails;
      stats_out[4 * nb + b] = 0;
    }
  }
  const unsigned long long mine[6] = {active ? (unsigned long long)n_steps : 0ull, 0ull, 0ull, active ? (unsigned long long)n_err_fails : 0ull, 0ull,
                                      (active && status != kRsOk) ? 1ull : 0ull};
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const unsigned long long sum = wave_sum_u64(mine[q]);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&totals[q], sum);
  }
}

}  // namespace dsh
