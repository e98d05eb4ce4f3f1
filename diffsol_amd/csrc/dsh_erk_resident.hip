// Device-resident explicit Runge-Kutta integration — Tsit45, the reference's fourth integrator (problem.tsit45(), crates/diffsol/src/ode_solver/explicit_rk.rs) —
// for ensembles of small NON-STIFF systems (gfx950).
//
// One launch integrates the whole ensemble, one lane per member, everything of ExplicitRk::step (explicit_rk.rs:196-243) and of the Rk core it calls
// (runge_kutta.rs: start_step :446, start_step_attempt :505, do_stage :537, error_norm :783, factor :466 with the four ExplicitRkConfig bounds, error_test_fail :843,
// step_accepted :894, handle_tstop :752, the beta-polynomial dense output :962-1002, pi_controller_raw :1313) per lane: no Jacobian, no LU, no Newton, no LDS.
// First same as last: stage 0 is state.dy, 6 right-hand sides per attempt.  With per-member control (group = 1) every member has its own h and stops at ITS OWN event
// time; with wavefront lock-step (group = 64) the reference's batched semantics hold per 64-member group (norms max-reduced over the wavefront, one h).
//
// Arithmetic is the checker's operation for operation (tests/erk_ref/erk_ref.cpp over the oracle's vector operations); compiled without contraction.  There is no
// fast-arithmetic twin: deterministic_pow = 2 runs this kernel with the portable pow, like 1.
//
// Two trailing template flags add to the lane's state, each for the models its admission function takes: SENS the forward sensitivities of every parameter
// (dsh_erk_solve_resident_sens), INTOUT the integral g of the output equations, returned in place of the states (dsh_erk_solve_resident_out / _steps_out); the
// checker has the same two as modes of its one integrator.  With both off the kernel is the plain one: the same instructions in the same order, the same registers and code length; since the
// folds moved into helpers a few commutative operands are swapped and a few literals enter with the other sign and are subtracted (profiles/erk_kernel_refactor.md).
#include <cmath>
#include <cstring>
#include <string>

#include "dsh_resident_host.hpp"

#include "dsh_erk_kernel.hpp"
#include "dsh_jit.hpp"

using namespace dsh;

namespace dsh {
// The built-in models k_erk_resident<Mdl, .., SENS, INTOUT> is instantiated for.  SENS: those of the plain kernel that carry parameter derivatives, have no root
// functions and keep N (14 + 12 NP) <= 112 doubles per lane (erk_sens_admitted, dsh_erk_kernel.hpp).  INTOUT: those whose states and outputs keep 14 n + 12 nout <= 112
// doubles per lane, nout <= 8 (erk_out_admitted); nout is the out_i count, or the state count for a model without out_i (identity output)
template <class Mdl, bool SENS = false, bool INTOUT = false> constexpr bool erk_admits() {
  constexpr bool plain = Mdl::N <= 4 && !Mdl::HAS_MASS && !model_has_reset<Mdl>::value;
  if constexpr (SENS && model_has_sens<Mdl>::value) return plain && Mdl::NROOTS == 0 && erk_sens_admitted(Mdl::N, Mdl::NP);
  else if constexpr (SENS) return false;
  else if constexpr (INTOUT) return plain && erk_out_admitted(Mdl::N, erk_nout_e<Mdl>());
  else return plain;
}
template <bool SENS, bool INTOUT> bool erk_static_admits(int model, int64_t size) {
  bool ok = false;
  dispatch_static_model(model, size, [&](auto mdl) { ok = erk_admits<decltype(mdl), SENS, INTOUT>(); });
  return ok;
}
// dsh_model_has_resident(3, ..): static models without a mass matrix and without a reset operator — built-in with n <= 4, run-time-compiled (DiffSL) in the static
// form with n <= 8 (the kernel holds 7 n stage values per lane: n = 8 still fits the register file)
int erk_model_has_resident(int model, int64_t size) {
  if (is_jit_model(model)) {
    const JitInfo* ji = jit_info(model);
    if (!ji) return 0;
    return (ji->form == DSH_JIT_FORM_STATIC && ji->n <= 8 && !ji->has_mass && !ji->has_reset) ? 1 : 0;
  }
  return erk_static_admits<false, false>(model, size) ? 1 : 0;
}
int erk_model_has_sens(int model, int64_t size) {
  if (!erk_model_has_resident(model, size)) return 0;
  if (is_jit_model(model)) {
    const JitInfo* ji = jit_info(model);
    if (!ji) return 0;
    return (ji->has_sens && ji->nroots == 0 && erk_sens_admitted(ji->n, ji->np)) ? 1 : 0;
  }
  return erk_static_admits<true, false>(model, size) ? 1 : 0;
}
int64_t erk_model_nout_e(int model, int64_t size) {
  if (is_jit_model(model)) {
    const JitInfo* ji = jit_info(model);
    return ji ? (ji->nout > 0 ? ji->nout : ji->n) : 0;
  }
  int64_t v = 0;
  dispatch_static_model(model, size, [&](auto mdl) { v = erk_nout_e<decltype(mdl)>(); });
  return v;
}
int erk_model_has_out_integral(int model, int64_t size) {
  if (!erk_model_has_resident(model, size)) return 0;
  if (is_jit_model(model)) {
    const JitInfo* ji = jit_info(model);
    return (ji && erk_out_admitted(ji->n, erk_model_nout_e(model, size))) ? 1 : 0;
  }
  return erk_static_admits<false, true>(model, size) ? 1 : 0;
}
}  // namespace dsh

namespace {
// Why a model is refused, in the caller's words: by the plain kernel, or (a model the plain kernel takes) with forward sensitivities / with integrated outputs
enum class ErkRefused { Plain, Sens, Out };
int erk_refuse(int model, int64_t size, ErkRefused what) {
  int64_t n = 0, np = 0, nroots = 0;
  int has_mass = 0;
  const bool known = dsh_model_info(model, size, &n, &np, &has_mass, &nroots) == DSH_OK;
  const int64_t no = what == ErkRefused::Out ? erk_model_nout_e(model, size) : 0;
  if (what == ErkRefused::Sens)
    set_error("dsh_erk_solve_resident_sens: Tsit45 integrates forward sensitivities register-resident only — models with parameter derivatives, without root functions "
              "(stop conditions), whose states and parameters satisfy nstates * (14 + 12 * nparams) <= 112 doubles per member (for example 2 states and up to 3 parameters, "
              "4 states and 1 parameter, 1 state and up to 8 parameters); this model has " + std::to_string(n) + " states, " + std::to_string(np) + " parameters (" +
              std::to_string(n * (14 + 12 * np)) + " doubles) and " + std::to_string(nroots) + " root functions: use BDF, TR-BDF2 or ESDIRK34 for its sensitivities");
  else if (what == ErkRefused::Out)
    set_error("dsh_erk_solve_resident_out: Tsit45 integrates outputs register-resident only — models whose states and outputs satisfy 14 * nstates + 12 * nout <= " +
              std::to_string(kErkMaxLaneDoubles) + " doubles per member with nout <= " + std::to_string(kErkMaxOut) + " (for example 4 states and 4 outputs, 7 states and 1 output, "
              "2 states and 7 outputs; a model without out_i integrates its states); this model has " + std::to_string(n) + " states and " + std::to_string(no) + " outputs (" +
              std::to_string(14 * n + 12 * no) + " doubles): integrate fewer outputs, or append the integrals as states and use BDF, TR-BDF2 or ESDIRK34");
  else if (known && has_mass)
    set_error("dsh_erk_solve_resident: MassMatrixNotSupported — explicit Runge-Kutta methods take no mass matrix (the reference refuses it too); use BDF, TR-BDF2 or ESDIRK34 "
              "(dsh_bdf_solve_adaptive, dsh_sdirk_solve_resident)");
  else
    set_error("dsh_erk_solve_resident: Tsit45 runs register-resident only — built-in static models with n <= 4, DiffSL models in the static form with n <= 8, no reset operator; "
              "banded lane-per-member, wavefront-per-member and workgroup-per-member forms (n > 8) are not provided: use BDF, TR-BDF2 or ESDIRK34 for this model");
  return DSH_E_UNSUPPORTED;
}

// The launch of k_erk_resident<Mdl, BA, WAVE, SENS, INTOUT>: a built-in model by the static dispatch over the models erk_admits takes, a run-time-compiled one under
// the kernel's name with the same flags (trailing defaults left out, as the committed JIT manifests spell them)
template <bool SENS, bool INTOUT>
int erk_launch(const SolveArgs& a, bool ba, bool wave, const ResidentLaunch& L) {
  const dim3 grid((unsigned)((a.nb + 63) / 64)), blk(64);  // 64 members per wavefront in both modes
  const ErkConsts* const consts_dev = (const ErkConsts*)L.consts;
  if (is_jit_model(a.model)) {
    const std::string name = std::string("dsh::k_erk_resident<dsh::JitModel, ") + (ba ? "true" : "false") + ", " + (wave ? "true" : "false") + (SENS ? ", true>" : (INTOUT ? ", false, true>" : ">"));
    return jit_launch(a.ctx, a.model, "dsh_erk_kernel.hpp", name, {name}, name, grid, blk, 0, a.nb, a.p, a.atol, consts_dev, L.t_eval, a.y_out, a.stats, a.status, a.t_root,
                      a.root_idx, a.ncols, L.totals);
  }
  dispatch_static_model(a.model, a.size, [&](auto mdl) {
    using Mdl = decltype(mdl);
    if constexpr (erk_admits<Mdl, SENS, INTOUT>())
      with_bools(ba, wave, [&](auto BA, auto WAVE) {
        hipLaunchKernelGGL((k_erk_resident<Mdl, decltype(BA)::value, decltype(WAVE)::value, SENS, INTOUT>), grid, blk, 0, a.ctx->stream, a.nb, a.p, a.atol, consts_dev, L.t_eval,
                           a.y_out, a.stats, a.status, a.t_root, a.root_idx, a.ncols, L.totals);
      });
  });
  return DSH_OK;
}

int erk_solve_resident_impl(const SolveArgs& a, int method) {
  static const char* const who = "dsh_erk_solve_resident";
  DSH_REQUIRE_AS(who, method == 3, "method must be 3 (Tsit45)");
  if (const int rc = check_solve_args(a, who); rc != DSH_OK) return rc;
  dsh_ctx* const ctx = a.ctx;
  const int model = a.model;
  const int64_t size = a.size, nb = a.nb;
  const bool sens = a.sens != nullptr;
  if (!erk_model_has_resident(model, size)) return erk_refuse(model, size, ErkRefused::Plain);
  if (sens && !erk_model_has_sens(model, size)) return erk_refuse(model, size, ErkRefused::Sens);
  const bool intout = a.intout != nullptr;
  DSH_REQUIRE_AS(who, !(sens && intout), "integrated outputs are not combined with forward sensitivities");
  if (intout && !erk_model_has_out_integral(model, size)) return erk_refuse(model, size, ErkRefused::Out);
  if (intout) {
    const int64_t no = erk_model_nout_e(model, size);
    DSH_REQUIRE_AS(who, a.intout->natol == 0 || a.intout->natol == 1 || a.intout->natol == no,
                   "out_atol must have length 1 or nout (" + std::to_string(no) + " for this model), or 0 to keep the outputs out of the error test; got " +
                       std::to_string(a.intout->natol));
    DSH_REQUIRE_AS(who, a.intout->natol == 0 || a.intout->atol_host != nullptr, "out_atol is null");
  }
  if (nb == 0) return DSH_OK;
  ErkConsts T;
  std::memset((void*)&T, 0, sizeof T);
  fill_resident(T.r, a);
  DSH_REQUIRE_AS(who, T.r.o.group == 1 || T.r.o.group == 64, "group must be 1 (per member) or 64 (wavefront lock-step)");
  // ExplicitRkConfig::default() (config.rs:141-160): NOT the BDF / SDIRK bounds dsh_adaptive_options carries
  T.min_shrink = 0.5; T.max_shrink = 1.0; T.min_growth = 1.0; T.max_growth = 2.0;
  fill_steps(T, a.steps);
  if (const int rc = fill_sens(T, a.sens, model, size, false, who); rc != DSH_OK) return rc;  // admitted models with parameters have at most 4 states
  if (intout) {  // the kernel's NOUT_E is at most 8 (erk_out_admitted)
    const OutSpec& os = *a.intout;
    T.out_rtol = os.rtol; T.out_error_control = os.natol > 0 ? 1 : 0; T.out_pad = os.natol <= 1 ? 1 : 0;
    for (int64_t k = 0; k < os.natol && k < kErkMaxOut; ++k) T.out_atol[k] = os.atol_host[k];
  }
  const bool ba = a.atol_nb == 1 && nb != 1;
  const bool wave = T.r.o.group == 64;
  ResidentLaunch L(ctx);
  if (const int rc = L.open(&T, sizeof T, a.t_eval_host, a.n_eval); rc != DSH_OK) return rc;
  const int rc = sens ? erk_launch<true, false>(a, ba, wave, L) : intout ? erk_launch<false, true>(a, ba, wave, L) : erk_launch<false, false>(a, ba, wave, L);
  if (rc != DSH_OK) return rc;
  return L.close(a.totals_host);
}
// OdeSolverMethod::solve (method.rs:227-258 over :881-961) inside the launch, for the two _steps entries: one save point, t_final, and the columns of every accepted step
int erk_solve_resident_steps_impl(const char* who, SolveArgs a, const double& t_final, int64_t max_cols, double* t_out, int method) {
  DSH_REQUIRE_AS(who, max_cols >= 2 && max_cols <= 0x7fffffff && a.y_out != nullptr && t_out != nullptr && a.ncols != nullptr,
                 std::string(who) + ": max_cols >= 2, y_out, t_out and ncols are needed");
  const StepsSpec st{t_out, max_cols};
  a.t_eval_host = &t_final; a.n_eval = 1; a.steps = &st;
  return erk_solve_resident_impl(a, method);
}
}  // namespace

extern "C" {

int dsh_erk_solve_resident(dsh_ctx* ctx, int method, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol, double t0,
                           double h0, const dsh_adaptive_options* opts, const double* t_eval_host, int64_t n_eval, double* y_out, int32_t* stats, int32_t* status,
                           double* t_root, int32_t* root_idx, int32_t* ncols, int64_t* totals_host) {
  DSH_ENTER(ctx);
  return erk_solve_resident_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, t_eval_host, n_eval, y_out, stats, status, t_root, root_idx, ncols, totals_host,
                                  nullptr, nullptr}, method);
}
// 1 when dsh_erk_solve_resident_sens takes the model: see erk_model_has_sens above
int dsh_erk_model_has_sens(int model, int64_t size) { return erk_model_has_sens(model, size); }
// Tsit45 with forward sensitivities in the same launch (problem.tsit45_sens(); arguments as dsh_sdirk_solve_resident_sens, method = 3): sens_out n_eval x np x n x nb,
// nsens_atol = 0 leaves the sensitivities out of the error control.  A model outside dsh_erk_model_has_sens: DSH_E_UNSUPPORTED.
int dsh_erk_solve_resident_sens(dsh_ctx* ctx, int method, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol, double t0,
                                double h0, const dsh_adaptive_options* opts, const double* t_eval_host, int64_t n_eval, double sens_rtol, const double* sens_atol_host,
                                int64_t nsens_atol, double* y_out, double* sens_out, int32_t* stats, int32_t* status, int64_t* totals_host) {
  DSH_ENTER(ctx);
  DSH_REQUIRE(sens_out != nullptr, "sens_out is null");
  DSH_REQUIRE(nsens_atol == 0 || sens_atol_host != nullptr, "sens_atol is null");
  const SensSpec sp{sens_out, sens_rtol, sens_atol_host, nsens_atol};
  return erk_solve_resident_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, t_eval_host, n_eval, y_out, stats, status, nullptr, nullptr, nullptr, totals_host,
                                  &sp, nullptr}, method);
}
// OdeSolverMethod::solve (method.rs:227-258 over :881-961) inside the launch: the state after every accepted step of every member (arguments as
// dsh_sdirk_solve_resident_steps)
int dsh_erk_solve_resident_steps(dsh_ctx* ctx, int method, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol,
                                 double t0, double h0, const dsh_adaptive_options* opts, double t_final, int64_t max_cols, double* y_out, double* t_out, int32_t* stats,
                                 int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols, int64_t* totals_host) {
  DSH_ENTER(ctx);
  return erk_solve_resident_steps_impl(__func__, {ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, nullptr, 0, y_out, stats, status, t_root, root_idx, ncols, totals_host,
                                                  nullptr, nullptr}, t_final, max_cols, t_out, method);
}
// rows of y_out in the *_out entries: the model's out_i count, its state count without out_i; 0 for a model Tsit45 does not take
int64_t dsh_erk_model_nout(int model, int64_t size) { return erk_model_has_resident(model, size) ? erk_model_nout_e(model, size) : 0; }
// 1 when dsh_erk_solve_resident_out / _steps_out take the model: see erk_model_has_out_integral above
int dsh_erk_model_has_out_integral(int model, int64_t size) { return erk_model_has_out_integral(model, size); }
// Tsit45 with the output equations integrated alongside the states (OdeBuilder::integrate_out(true) over problem.tsit45()): arguments as dsh_erk_solve_resident;
// y_out n_eval x nout x nb holds g(t) = integral of out(y, t) from t0 (nout: the model's out_i count, its state count without out_i).  nout_atol = 0 keeps g out of the
// error test, 1 gives one out_atol for every output, nout one each.  A model outside dsh_erk_model_has_out_integral: DSH_E_UNSUPPORTED.
int dsh_erk_solve_resident_out(dsh_ctx* ctx, int method, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol, double t0,
                               double h0, const dsh_adaptive_options* opts, const double* t_eval_host, int64_t n_eval, double out_rtol, const double* out_atol_host,
                               int64_t nout_atol, double* y_out, int32_t* stats, int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols, int64_t* totals_host) {
  DSH_ENTER(ctx);
  const OutSpec os{out_rtol, out_atol_host, nout_atol};
  return erk_solve_resident_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, t_eval_host, n_eval, y_out, stats, status, t_root, root_idx, ncols, totals_host,
                                  nullptr, nullptr, &os}, method);
}
// the same for every accepted step (arguments as dsh_erk_solve_resident_steps): column 0 is g(t0) = 0
int dsh_erk_solve_resident_steps_out(dsh_ctx* ctx, int method, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol,
                                     double t0, double h0, const dsh_adaptive_options* opts, double t_final, int64_t max_cols, double out_rtol, const double* out_atol_host,
                                     int64_t nout_atol, double* y_out, double* t_out, int32_t* stats, int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols,
                                     int64_t* totals_host) {
  DSH_ENTER(ctx);
  const OutSpec os{out_rtol, out_atol_host, nout_atol};
  return erk_solve_resident_steps_impl(__func__, {ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, nullptr, 0, y_out, stats, status, t_root, root_idx, ncols, totals_host,
                                                  nullptr, nullptr, &os}, t_final, max_cols, t_out, method);
}

}  // extern "C"
