// Device-resident (E)SDIRK integration — TR-BDF2 and ESDIRK34 — for ensembles of small systems (gfx950): SURVEY §8(f) row 1 for BASELINE config 5
// ("electrical-circuits DAE with event/root-finding, ESDIRK34, divergent-step repacking").
//
// One launch integrates the whole ensemble, one lane per member, everything of Sdirk::step (crates/diffsol/src/ode_solver/sdirk.rs:409-543) and the
// Rk core (runge_kutta.rs:466-960) per lane: stage predictor and Newton solves with the shared M - γhJ (linearised at φ + γ·state.y like the
// reference), embedded error estimate filtered through one LU solve, PI controller, JacobianUpdate policy, consistent DAE initialisation
// (state.rs:84-162), root finding on the dense output (root.rs), tstop handling and solve_dense (method.rs:467-520).  With per-member control
// (group = 1) every member stops at ITS OWN event time — what the lock-step backend cannot do (vector/cuda.rs:1166-1171 panics when the batch
// disagrees on the crossing); with wavefront lock-step (group = 64) the reference's batched semantics hold per 64-member group.
//
// State per lane (n = 4, s = 4): stage derivatives diff (n x s), state/old state (y, dy), φ, LU factors in registers; cached Jacobian in LDS.
// Arithmetic is the oracle's operation for operation (oracle/oracle_sdirk.hpp); pow()/sin() are ocml's.
#include <cmath>
#include <cstring>
#include <vector>

#include "dsh_resident_host.hpp"

#include "dsh_sdirk_kernel.hpp"
#include "dsh_jit.hpp"

using namespace dsh;

namespace dsh {
bool sdirk_fast_launch(int method, int model, int64_t size, bool ba, bool wave, dim3 grid, hipStream_t stream, int64_t nb, const double* p, const double* atol,
                       const SdirkConsts* consts, const double* t_eval, double* y_out, int32_t* stats, int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols,
                       unsigned long long* totals);  // dsh_sdirk_fast.hip
int erk_model_has_resident(int model, int64_t size);  // dsh_erk_resident.hip
}

extern "C" {

int dsh_model_has_resident(int method, int model, int64_t size) {
  if (method == 0) return dsh_model_has_adaptive(model, size);
  if (method == 3) return erk_model_has_resident(model, size);  // Tsit45
  if (method != 1 && method != 2) return 0;
  if (is_jit_model(model)) {
    const JitInfo* ji = jit_info(model);
    if (!ji) return 0;
    // banded lane-per-member form with a mass matrix: BDF only so far (k_bdf_lane_banded); TR-BDF2 / ESDIRK34 of such a model run wavefront per member
    return (ji->form == DSH_JIT_FORM_STATIC && ji->n <= 4) || (ji->form == DSH_JIT_FORM_STATIC_BANDED && ji->n <= 512 && !ji->has_mass) ? 1 : 0;
  }
  bool ok = false;
  dispatch_static_model(model, size, [&](auto mdl) {
    using Mdl = decltype(mdl);
    ok = Mdl::N <= 4;
  });
  return ok ? 1 : 0;
}

}  // extern "C"
namespace {
template <class Mdl> constexpr bool sdirk_sens_ok() {
  if constexpr (model_has_sens<Mdl>::value) return Mdl::N <= 4 && !Mdl::HAS_MASS && Mdl::NROOTS == 0 && model_band_k<Mdl>::value == 0;
  else return false;
}
int sdirk_solve_resident_impl(const SolveArgs& a, int method);
}  // namespace
extern "C" {
int dsh_sdirk_solve_resident(dsh_ctx* ctx, int method, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol,
                             double t0, double h0, const dsh_adaptive_options* opts, const double* t_eval_host, int64_t n_eval, double* y_out, int32_t* stats,
                             int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols, int64_t* totals_host) {
  DSH_ENTER(ctx);
  return sdirk_solve_resident_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, t_eval_host, n_eval, y_out, stats, status, t_root, root_idx, ncols, totals_host,
                                    nullptr, nullptr}, method);
}
// OdeSolverMethod::solve (method.rs:227-258 over :881-961) inside the launch of the device-resident TR-BDF2 / ESDIRK34: the state after every accepted step of every member
// (arguments as dsh_bdf_solve_adaptive_steps; the models of dsh_model_has_resident(method, ..))
int dsh_sdirk_solve_resident_steps(dsh_ctx* ctx, int method, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol,
                                   double t0, double h0, const dsh_adaptive_options* opts, double t_final, int64_t max_cols, double* y_out, double* t_out, int32_t* stats,
                                   int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols, int64_t* totals_host) {
  DSH_ENTER(ctx);
  DSH_REQUIRE(max_cols >= 2 && max_cols <= 0x7fffffff && y_out != nullptr && t_out != nullptr && ncols != nullptr, "dsh_sdirk_solve_resident_steps: max_cols >= 2, y_out, t_out and ncols are needed");
  const StepsSpec st{t_out, max_cols};
  return sdirk_solve_resident_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, &t_final, 1, y_out, stats, status, t_root, root_idx, ncols, totals_host, nullptr, &st},
                                   method);
}
// TR-BDF2 / ESDIRK34 with forward sensitivities in the same launch (dsh_bdf_solve_adaptive_sens is the BDF): the same models (dsh_model_has_adaptive_sens)
int dsh_sdirk_solve_resident_sens(dsh_ctx* ctx, int method, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol,
                                  double t0, double h0, const dsh_adaptive_options* opts, const double* t_eval_host, int64_t n_eval, double sens_rtol,
                                  const double* sens_atol_host, int64_t nsens_atol, double* y_out, double* sens_out, int32_t* stats, int32_t* status, int64_t* totals_host) {
  DSH_ENTER(ctx);
  DSH_REQUIRE(sens_out != nullptr, "sens_out is null");
  DSH_REQUIRE(nsens_atol == 0 || sens_atol_host != nullptr, "sens_atol is null");
  if (!dsh_model_has_adaptive_sens(model, size)) {
    set_error("dsh_sdirk_solve_resident_sens: the model has no device-resident integrator with forward sensitivities (identity-mass ODE model with parameter derivatives and no root functions: register-resident n <= 4, or the banded lane-per-member form)");
    return DSH_E_UNSUPPORTED;
  }
  const SensSpec sp{sens_out, sens_rtol, sens_atol_host, nsens_atol};
  return sdirk_solve_resident_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, t_eval_host, n_eval, y_out, stats, status, nullptr, nullptr, nullptr, totals_host,
                                    &sp, nullptr}, method);
}
}  // extern "C"
namespace {
int sdirk_solve_resident_impl(const SolveArgs& a, int method) {
  static const char* const who = "dsh_sdirk_solve_resident";
  DSH_REQUIRE_AS(who, method == 1 || method == 2, "method must be 1 (TR-BDF2) or 2 (ESDIRK34)");
  if (const int rc = check_solve_args(a, who); rc != DSH_OK) return rc;
  dsh_ctx* const ctx = a.ctx;
  const int model = a.model;
  const int64_t size = a.size, nb = a.nb;
  const bool sens = a.sens != nullptr;
  if (!dsh_model_has_resident(method, model, size)) { set_error("dsh_sdirk_solve_resident: model has no device-resident kernel (needs a static model, n <= 4)"); return DSH_E_UNSUPPORTED; }
  if (nb == 0) return DSH_OK;
  SdirkConsts T;
  std::memset((void*)&T, 0, sizeof T);
  fill_resident(T.r, a);
  DSH_REQUIRE_AS(who, T.r.o.group == 1 || T.r.o.group == 64, "group must be 1 (per member) or 64 (wavefront lock-step)");
  {
    // per-member control: DSH_MEMBER_LANES = 32 | 16 | 8 puts that many members on a wavefront (measured in profiles/r05_member_lanes.md); 0 / unset: 64
    static const int member_lanes_env = [] { const char* e = std::getenv("DSH_MEMBER_LANES"); const int v = e && *e ? std::atoi(e) : -1; return (v == 8 || v == 16 || v == 32 || v == 64) ? v : -1; }();
    // default: 32 members per wavefront while that still leaves at most two wavefronts per SIMD (the kernel's register occupancy) on the chip's 1024 SIMDs — the wavefront
    // pays for the union of 32 paths instead of 64 (config 5, 65 536 members: 21.1 -> 19.9 ms, same bits) —, 64 beyond (more wavefronts would queue)
    // (measured, RLC / ESDIRK34 with events, ms at 64 | 32 members per wavefront: 16 384 members 21.4 | 22.7, 32 768: 20.8 | 19.7, 49 152: 21.0 | 19.8, 65 536: 20.8 | 19.7 —
    // the kernel lasts as long as its slowest member's chain whatever the ensemble size; the halved wavefronts pay from half a wavefront per SIMD on)
    const int64_t simds = 4 * (int64_t)ctx->num_cu;
    const int auto_lanes = ((nb + 63) / 64 * 2 >= simds && (nb + 31) / 32 <= 2 * simds) ? 32 : 0;
    T.r.member_lanes = (T.r.o.group == 1 && !is_jit_model(model)) ? (member_lanes_env > 0 ? (member_lanes_env == 64 ? 0 : member_lanes_env) : auto_lanes) : 0;
  }
  fill_tableau(method, T);  // resets the steps fields: ahead of fill_steps
  fill_steps(T, a.steps);
  if (const int rc = fill_sens(T, a.sens, model, size, true, who); rc != DSH_OK) return rc;
  const bool ba = a.atol_nb == 1 && nb != 1;
  const bool wave = T.r.o.group == 64;
  const int per_wave = T.r.member_lanes > 0 ? T.r.member_lanes : 64;
  const dim3 grid((unsigned)((nb + per_wave - 1) / per_wave)), blk(64);
  ResidentLaunch L(ctx);
  if (const int rc = L.open(&T, sizeof T, a.t_eval_host, a.n_eval); rc != DSH_OK) return rc;
  const SdirkConsts* const consts_dev = (const SdirkConsts*)L.consts;
  if (is_jit_model(model)) {
    const std::string name = std::string("dsh::k_sdirk_resident<dsh::JitModel, ") + (ba ? "true" : "false") + ", " + (wave ? "true" : "false") + ", " + (method == 1 ? "3" : "4") + (sens ? ", true>" : ">");
    const int rc = jit_launch(ctx, model, "dsh_sdirk_kernel.hpp", name, {name}, name, grid, blk, 0, nb, a.p, a.atol, consts_dev, L.t_eval, a.y_out, a.stats, a.status, a.t_root,
                              a.root_idx, a.ncols, L.totals);
    if (rc != DSH_OK) return rc;
  } else if (!sens && T.r.o.deterministic_pow == 2 &&
             // the fast-arithmetic build (dsh_sdirk_fast.hip): static models with n <= 4; a model without it falls through to the exact kernel below
             sdirk_fast_launch(method, model, size, ba, wave, grid, ctx->stream, nb, a.p, a.atol, consts_dev, L.t_eval, a.y_out, a.stats, a.status, a.t_root, a.root_idx,
                               a.ncols, L.totals)) {
  } else if (sens) {
    dispatch_static_model(model, size, [&](auto mdl) {
      using Mdl = decltype(mdl);
      if constexpr (sdirk_sens_ok<Mdl>())
        with_bools_stages(ba, wave, method == 1 ? 3 : 4, [&](auto BA, auto WAVE, auto S) {
          hipLaunchKernelGGL((k_sdirk_resident<Mdl, decltype(BA)::value, decltype(WAVE)::value, decltype(S)::value, true>), grid, blk, 0, ctx->stream, nb, a.p, a.atol,
                             consts_dev, L.t_eval, a.y_out, a.stats, a.status, a.t_root, a.root_idx, a.ncols, L.totals);
        });
    });
  } else
  dispatch_static_model(model, size, [&](auto mdl) {
    using Mdl = decltype(mdl);
    if constexpr (Mdl::N <= 4)
      with_bools_stages(ba, wave, method == 1 ? 3 : 4, [&](auto BA, auto WAVE, auto S) {
        hipLaunchKernelGGL((k_sdirk_resident<Mdl, decltype(BA)::value, decltype(WAVE)::value, decltype(S)::value>), grid, blk, 0, ctx->stream, nb, a.p, a.atol, consts_dev,
                           L.t_eval, a.y_out, a.stats, a.status, a.t_root, a.root_idx, a.ncols, L.totals);
      });
  });
  return L.close(a.totals_host);
}
}  // namespace
