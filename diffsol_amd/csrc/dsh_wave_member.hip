// Device-resident BDF for MEDIUM-sized systems (8 < n <= 64): one WAVEFRONT per ensemble member, lane = state component (gfx950).
// BASELINE config 4 (single-particle battery model, n = 42, 262 144 members, stop conditions on the terminal voltage) on the device.
//
// dsh_adaptive.hip keeps a whole member in one lane's registers, which ends at n = 4.  Here the member is spread over the lanes of one wavefront:
// lane i holds component i of the state, of the prediction, of psi, its row of the difference array D (8 doubles) and its row of M - cJ (the LU
// factors, NP doubles: the wavefront LU of dsh_lu_wave.hpp, in place); the cached Jacobian sits in LDS.  Every scalar of Bdf::step — t, h, order,
// Convergence, JacobianUpdate, PI memory — is wavefront-uniform, so the control flow of one member never diverges, and members do not wait for each
// other: per-member step sizes, orders and EVENT TIMES (the reference's CPU semantics for a sweep) with no host in the loop and no SIMT tax.
//   * model evaluation: x is exchanged through 512 B of LDS; component i of f and row i of J by dyn_component (dsh_models_dyn.hpp)
//   * norms: per-lane terms, summed in index order over v_readlane (the oracle's sequential sum: bit-identical)
//   * linear solves: wave_lu_solve_rows — the rows stay where the factorisation left them, no interchange of the right-hand side
// Arithmetic is the oracle's operation for operation; pow() and the model's tanh/asinh/exp are ocml's (tests state the tolerance).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsh_resident_host.hpp"
#include "dsh_wave_member_kernel.hpp"
#include "dsh_team_member_kernel.hpp"
#include "dsh_sdirk_wave_member_kernel.hpp"
#include "dsh_jit.hpp"

using namespace dsh;


extern "C" {

// 1: one wavefront per member (n <= 64; BDF and the SDIRK methods); 2: one workgroup per member (64 < n <= 320, identity mass; BDF — dsh_team_member_kernel.hpp); 0: neither
int dsh_model_has_wave_member(int model, int64_t size) {
  if (is_jit_model(model)) {  // run-time-sized DiffSL model: at most two stop conditions, one lane per component
    const JitInfo* ji = jit_info(model);
    if (!(ji && ji->form == DSH_JIT_FORM_DYNAMIC && ji->nroots <= 2 && ji->np <= 64)) return 0;  // (the workgroup form would take up to 128 / 192 parameters)
    // with a mass matrix (DAEs: consistent initialisation and M in the residual and in M - cJ) the kernel keeps M's rows in LDS next to J's: n <= 48
    if (ji->n <= (ji->has_mass ? 48 : 64)) return 1;
    return !ji->has_mass && ji->n <= kTeamMaxN ? 2 : 0;
  }
  if (!(model == DSH_MODEL_DYDT_Y2 || model == DSH_MODEL_GAUSSIAN_DECAY || model == DSH_MODEL_HEAT1D || model == DSH_MODEL_SPM ||
        (model == DSH_MODEL_ROBERTSON_ODE && size > 1)))
    return 0;
  int64_t n = 0;
  int has_mass = 0;
  if (dsh_model_info(model, size, &n, nullptr, &has_mass, nullptr) != DSH_OK) return 0;
  if (n < 1) return 0;
  if (n <= 64) return 1;
  return !has_mass && n <= kTeamMaxN ? 2 : 0;  // the workgroup form takes identity-mass models
}

// the register-resident LU of the workgroup-per-member BDF (64 < n <= 128) — on unless DSH_TEAM_REG_LU=0 (read at every launch: the tests compare the two forms)
static bool team_reg_lu_on() { const char* e = getenv("DSH_TEAM_REG_LU"); return !(e && e[0] == '0'); }
// identity-mass models above this size take the workgroup form (two wavefronts, the LU in registers) instead of the wavefront-per-member kernel; DSH_TEAM_SMALL_MIN overrides
static int team_small_min() { const char* e = getenv("DSH_TEAM_SMALL_MIN"); const int v = e ? atoi(e) : 32; return v < 8 ? 8 : (v > 64 ? 64 : v); }
static int bdf_solve_wave_member_impl(const SolveArgs& a);
// OdeSolverMethod::solve (method.rs:227-258 over :881-961) inside the launch of the wavefront- / workgroup-per-member BDF: the state after every accepted step of every
// member (y_out [max_cols][n][nb], t_out [max_cols][nb], ncols[b] = the columns member b produced; columns beyond max_cols are counted, not stored), to t_final
int dsh_bdf_solve_wave_member_steps(dsh_ctx* ctx, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol, double t0,
                                    double h0, const dsh_adaptive_options* opts, double t_final, int64_t max_cols, double* y_out, double* t_out, int32_t* stats,
                                    int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols, int64_t* totals_host) {
  DSH_ENTER(ctx);
  DSH_REQUIRE(max_cols >= 2 && max_cols <= 0x7fffffff && y_out != nullptr && t_out != nullptr && ncols != nullptr, "dsh_bdf_solve_wave_member_steps: max_cols >= 2, y_out, t_out and ncols are needed");
  const StepsSpec st{t_out, max_cols};
  return bdf_solve_wave_member_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, &t_final, 1, y_out, stats, status, t_root, root_idx, ncols, totals_host, nullptr, &st});
}
int dsh_bdf_solve_wave_member(dsh_ctx* ctx, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol, double t0,
                              double h0, const dsh_adaptive_options* opts, const double* t_eval_host, int64_t n_eval, double* y_out, int32_t* stats,
                              int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols, int64_t* totals_host) {
  DSH_ENTER(ctx);
  return bdf_solve_wave_member_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, t_eval_host, n_eval, y_out, stats, status, t_root, root_idx, ncols, totals_host, nullptr, nullptr});
}
// hybrid models whose events are handled INSIDE the wavefront-per-member kernels (BDF, TR-BDF2, ESDIRK34: the reset applied at every event, then on to the last save
// point): run-time-compiled models with a reset operator, root functions and no mass matrix, n <= 64
int dsh_model_has_wave_member_reset(int model, int64_t size) {
  const int kind = is_jit_model(model) ? dsh_model_has_wave_member(model, size) : 0;  // 1: a wavefront per member (n <= 64); 2: a workgroup per member (64 < n <= 320; BDF)
  if (kind == 0) return 0;
  const JitInfo* ji = jit_info(model);
  return ji && ji->has_reset && !ji->has_mass && ji->nroots > 0 ? kind : 0;
}
// forward sensitivities in the wavefront-per-member BDF (k_bdf_wave_member<.., SENS>): run-time-compiled dense ODE models with parameter derivatives, n <= 64, at most
// kWmMaxSensParams parameters, no mass matrix, no root functions
int dsh_model_has_wave_member_sens(int model, int64_t size) {
  const int kind = is_jit_model(model) ? dsh_model_has_wave_member(model, size) : 0;  // 2: the workgroup-per-member BDF (64 < n <= 320)
  if (kind == 0) return 0;
  const JitInfo* ji = jit_info(model);
  return ji && ji->has_sens && !ji->has_mass && ji->nroots == 0 && ji->np <= kWmMaxSensParams ? kind : 0;
}
int dsh_bdf_solve_wave_member_sens(dsh_ctx* ctx, int model, int64_t size, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol, double t0,
                                   double h0, const dsh_adaptive_options* opts, const double* t_eval_host, int64_t n_eval, double sens_rtol, const double* sens_atol_host,
                                   int64_t nsens_atol, double* y_out, double* sens_out, int32_t* stats, int32_t* status, int64_t* totals_host) {
  DSH_ENTER(ctx);
  DSH_REQUIRE(sens_out != nullptr, "sens_out is null");
  DSH_REQUIRE(nsens_atol == 0 || sens_atol_host != nullptr, "sens_atol is null");
  if (!dsh_model_has_wave_member_sens(model, size)) {
    set_error("dsh_bdf_solve_wave_member_sens: needs a run-time-compiled ODE model with parameter derivatives, n <= 320, at most 16 parameters, no mass matrix, no root functions");
    return DSH_E_UNSUPPORTED;
  }
  for (int64_t i = 1; i < nsens_atol; ++i) DSH_REQUIRE(sens_atol_host[i] == sens_atol_host[0], "the wavefront-per-member kernel takes one sens_atol for every state");
  const SensSpec sp{sens_out, sens_rtol, sens_atol_host, nsens_atol};
  return bdf_solve_wave_member_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, t_eval_host, n_eval, y_out, stats, status, nullptr, nullptr, nullptr, totals_host, &sp, nullptr});
}
static int bdf_solve_wave_member_impl(const SolveArgs& a) {
  static const char* const who = "dsh_bdf_solve_wave_member";
  if (const int rc = check_solve_args(a, who); rc != DSH_OK) return rc;
  dsh_ctx* const ctx = a.ctx;
  const int model = a.model;
  const int64_t size = a.size, nb = a.nb;
  const bool sens = a.sens != nullptr;
  const int wm_kind = dsh_model_has_wave_member(model, size);
  if (!wm_kind) { set_error("dsh_bdf_solve_wave_member: needs a run-time-sized model (built-in or DiffSL) with n <= 64 (n <= 48 with a mass matrix; identity mass: n <= 320, one workgroup per member) and at most two stop conditions"); return DSH_E_UNSUPPORTED; }
  if (nb == 0) return DSH_OK;
  int64_t n = 0, np = 0, nroots = 0;
  int has_mass = 0;
  if (const int rc = dsh_model_info(model, size, &n, &np, &has_mass, &nroots); rc != DSH_OK) return rc;
  DSH_REQUIRE_AS(who, np <= (wm_kind == 2 ? 64 * team_waves((int)n) : 64) && nroots <= 2, "wave-member kernel: at most 64 parameters (workgroup form: one per thread) and 2 root functions");
  WaveMemberConsts C;
  std::memset((void*)&C, 0, sizeof C);
  C.model = model; C.n = (int)n; C.np = (int)np; C.nroots = (int)nroots;
  fill_sens_one(C, a.sens);
  fill_steps(C, a.steps);
  fill_resident(C.r, a);
  fill_bdf_tables(C.alpha, C.gamma, C.ec2, C.u);
  const int ab = a.atol_nb == 1 ? 1 : 0;
  ResidentLaunch L(ctx);
  // what every kernel of this file takes behind (nb, p, atol, ab, consts, t_eval [, jac_scratch])
#define DSH_WM_OUT a.y_out, a.stats, a.status, a.t_root, a.root_idx, a.ncols, L.totals
  // 32 < n <= 64, identity mass, no sensitivities: the workgroup form with the LU in registers too (faster from n = 33 on: 1024 members 11.9 -> 7.5 ms there, 13.9 -> 8.8 ms at n = 48) — the wavefront-per-member kernel's elimination (one lane per row, a
  // jump per pivot into straight-line code) needs more than the 512 registers a wavefront can have next to the integrator's state at NP = 64 (2.5 KB of scratch, most of
  // its traffic inside the elimination: 227 us per factorisation at n = 60 inside that kernel against 90 us here; profiles/r06_team_reg_lu.md)
  const bool small_team = wm_kind == 1 && n > team_small_min() && !has_mass && !sens && team_reg_lu_on();
  if (wm_kind == 2 || small_team) {
    // one workgroup per member (48 < n <= 320): the factors in registers (n <= 128) / LDS / global scratch, the cached Jacobians in global scratch (n^2 doubles per member)
    const int waves = team_waves((int)n);
    // 64 < n <= 128 without sensitivities: the factors in the registers of four wavefronts (dsh_team_reg_lu.hpp; DSH_TEAM_REG_LU=0: in LDS, two wavefronts, as before).
    // NL, the compile-time bound on n: n rounded up to 8 for a run-time-compiled model (its module is its own), five steps for the built-in ones
    // (120: the reference's own benchmark size, robertson_ode x 40).
    const bool reg_lu = !sens && n <= kTrgMaxN && team_reg_lu_on();
    const int NL = !reg_lu ? 0 : (is_jit_model(model) ? trg_nl((int)n) : (n <= 48 ? 48 : (n <= 64 ? 64 : (n <= 80 ? 80 : (n <= 96 ? 96 : (n <= 112 ? 112 : (n <= 120 ? 120 : 128)))))));
    const size_t lds_team = sizeof(double) * (reg_lu ? team_rl_lds_doubles(NL) : team_lds_doubles((int)n, waves));
    double* jac_scratch = nullptr;
    if (const int rc = L.blocks.take((int64_t)(sizeof(double) * team_scratch_doubles((int)n, waves)) * nb, 0, &jac_scratch); rc != DSH_OK) return rc;
    if (const int rc = L.open(&C, sizeof C, a.t_eval_host, a.n_eval); rc != DSH_OK) return rc;
    const WaveMemberConsts* const consts_dev = (const WaveMemberConsts*)L.consts;
    if (is_jit_model(model)) {
      const std::string name = reg_lu ? std::string("dsh::k_bdf_team_member_rl<") + std::to_string(NL) + ">"
                                      : std::string("dsh::k_bdf_team_member<") + std::to_string(waves) + (sens ? ", true>" : ">");
      const int rc = jit_launch(ctx, model, "dsh_jit_team_member.hpp", name, {name}, name, dim3((unsigned)nb), dim3(reg_lu ? trg_threads(NL) : 64 * waves), (unsigned)lds_team, nb, a.p,
                                a.atol, ab, consts_dev, L.t_eval, jac_scratch, DSH_WM_OUT);
      if (rc != DSH_OK) return rc;
    } else if (reg_lu) {
      static bool attr_rl_dev[64] = {false};
      bool& attr = attr_rl_dev[ctx->device & 63];
      if (!attr) {
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_bdf_team_member_rl<48>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_bdf_team_member_rl<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_bdf_team_member_rl<80>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_bdf_team_member_rl<96>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_bdf_team_member_rl<112>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_bdf_team_member_rl<120>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_bdf_team_member_rl<128>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr = true;
      }
#define DSH_TMR_LAUNCH(NLV) \
  hipLaunchKernelGGL((k_bdf_team_member_rl<NLV>), dim3((unsigned)nb), dim3(trg_threads(NLV)), lds_team, ctx->stream, nb, a.p, a.atol, ab, consts_dev, L.t_eval, jac_scratch, DSH_WM_OUT)
      if (getenv("DSH_TEAM_DEBUG")) {  // how many members share a CU (two when the workspace fits twice)
        int occ = 0;
        if (NL == 128) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_bdf_team_member_rl<128>, kTrgThreads, lds_team);
        else if (NL == 120) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_bdf_team_member_rl<120>, kTrgThreads, lds_team);
        else if (NL == 112) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_bdf_team_member_rl<112>, kTrgThreads, lds_team);
        else if (NL == 96) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_bdf_team_member_rl<96>, kTrgThreads, lds_team);
        else if (NL == 64) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_bdf_team_member_rl<64>, trg_threads(64), lds_team);
        else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_bdf_team_member_rl<80>, kTrgThreads, lds_team);
        fprintf(stderr, "k_bdf_team_member_rl<%d>: n = %d, %zu bytes of LDS, %d workgroups per CU\n", NL, (int)n, lds_team, occ);
      }
      if (NL == 48) DSH_TMR_LAUNCH(48); else if (NL == 64) DSH_TMR_LAUNCH(64); else if (NL == 80) DSH_TMR_LAUNCH(80); else if (NL == 96) DSH_TMR_LAUNCH(96); else if (NL == 112) DSH_TMR_LAUNCH(112); else if (NL == 120) DSH_TMR_LAUNCH(120); else DSH_TMR_LAUNCH(128);
#undef DSH_TMR_LAUNCH
    } else {
      static bool attr_dev[64] = {false};
      bool& attr = attr_dev[ctx->device & 63];
      if (!attr) {
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_bdf_team_member<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_bdf_team_member<3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr = true;
      }
#define DSH_TM_LAUNCH(WV) \
  hipLaunchKernelGGL((k_bdf_team_member<WV>), dim3((unsigned)nb), dim3(64 * WV), lds_team, ctx->stream, nb, a.p, a.atol, ab, consts_dev, L.t_eval, jac_scratch, DSH_WM_OUT)
      if (waves == 2) DSH_TM_LAUNCH(2); else if (waves == 3) DSH_TM_LAUNCH(3); else if (waves == 4) DSH_TM_LAUNCH(4); else DSH_TM_LAUNCH(5);
#undef DSH_TM_LAUNCH
    }
  } else {
    const size_t lds_bytes = sizeof(double) * (128 + (size_t)n * 64 + (has_mass ? (size_t)n * 64 + 64 : (sens ? 64 : 0)));  // xs | ps | sJ | (sM | xs2)  (sensitivities: xs2)
    if (const int rc = L.open(&C, sizeof C, a.t_eval_host, a.n_eval); rc != DSH_OK) return rc;
    const WaveMemberConsts* const consts_dev = (const WaveMemberConsts*)L.consts;
#define DSH_WM_LAUNCH(NPV) \
  hipLaunchKernelGGL((k_bdf_wave_member<NPV>), dim3((unsigned)nb), dim3(64), lds_bytes, ctx->stream, nb, a.p, a.atol, ab, consts_dev, L.t_eval, DSH_WM_OUT)
    if (is_jit_model(model)) {
      const std::string name = std::string("dsh::k_bdf_wave_member<") + (n <= 16 ? "16" : n <= 32 ? "32" : n <= 48 ? "48" : "64") + (sens ? ", true>" : ">");
      const int rc = jit_launch(ctx, model, "dsh_jit_wave_member.hpp", name, {name}, name, dim3((unsigned)nb), dim3(64), (unsigned)lds_bytes, nb, a.p, a.atol, ab, consts_dev, L.t_eval,
                                DSH_WM_OUT);
      if (rc != DSH_OK) return rc;
    } else if (n <= 16) DSH_WM_LAUNCH(16);
    else if (n <= 32) DSH_WM_LAUNCH(32);
    else if (n <= 48) DSH_WM_LAUNCH(48);
    else DSH_WM_LAUNCH(64);
#undef DSH_WM_LAUNCH
  }
  return L.close(a.totals_host);
}

// has_wave_member for the SDIRK methods: the wavefront-per-member models (n <= 64); the workgroup-per-member form is BDF only
int dsh_model_has_wave_member_sdirk(int model, int64_t size) { return dsh_model_has_wave_member(model, size); }  // 1: a wavefront per member; 2: a workgroup per member (k_sdirk_wave_member<.., TW>)

static int sdirk_solve_wave_member_impl(const SolveArgs& a, int method);
// OdeSolverMethod::solve (method.rs:227-258 over :881-961) inside the launch of the wavefront- / workgroup-per-member TR-BDF2 / ESDIRK34: the arguments of
// dsh_bdf_solve_wave_member_steps plus the method
int dsh_sdirk_solve_wave_member_steps(dsh_ctx* ctx, int model, int64_t size, int method, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol,
                                      double t0, double h0, const dsh_adaptive_options* opts, double t_final, int64_t max_cols, double* y_out, double* t_out,
                                      int32_t* stats, int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols, int64_t* totals_host) {
  DSH_ENTER(ctx);
  DSH_REQUIRE(max_cols >= 2 && max_cols <= 0x7fffffff && y_out != nullptr && t_out != nullptr && ncols != nullptr, "dsh_sdirk_solve_wave_member_steps: max_cols >= 2, y_out, t_out and ncols are needed");
  const StepsSpec st{t_out, max_cols};
  return sdirk_solve_wave_member_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, &t_final, 1, y_out, stats, status, t_root, root_idx, ncols, totals_host, nullptr, &st}, method);
}
int dsh_sdirk_solve_wave_member(dsh_ctx* ctx, int model, int64_t size, int method, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol,
                                double t0, double h0, const dsh_adaptive_options* opts, const double* t_eval_host, int64_t n_eval, double* y_out, int32_t* stats,
                                int32_t* status, double* t_root, int32_t* root_idx, int32_t* ncols, int64_t* totals_host) {
  DSH_ENTER(ctx);
  return sdirk_solve_wave_member_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, t_eval_host, n_eval, y_out, stats, status, t_root, root_idx, ncols, totals_host, nullptr, nullptr}, method);
}
// forward sensitivities in the wavefront-per-member TR-BDF2 / ESDIRK34 (k_sdirk_wave_member<.., SENS>): the models of dsh_model_has_wave_member_sens
int dsh_sdirk_solve_wave_member_sens(dsh_ctx* ctx, int model, int64_t size, int method, int64_t nb, const double* p, const double* atol, int64_t atol_nb, double rtol,
                                     double t0, double h0, const dsh_adaptive_options* opts, const double* t_eval_host, int64_t n_eval, double sens_rtol,
                                     const double* sens_atol_host, int64_t nsens_atol, double* y_out, double* sens_out, int32_t* stats, int32_t* status, int64_t* totals_host) {
  DSH_ENTER(ctx);
  DSH_REQUIRE(sens_out != nullptr, "sens_out is null");
  DSH_REQUIRE(nsens_atol == 0 || sens_atol_host != nullptr, "sens_atol is null");
  if (!dsh_model_has_wave_member_sens(model, size)) {
    set_error("dsh_sdirk_solve_wave_member_sens: needs a run-time-compiled ODE model with parameter derivatives, n <= 320, at most 16 parameters, no mass matrix, no root functions");
    return DSH_E_UNSUPPORTED;
  }
  for (int64_t i = 1; i < nsens_atol; ++i) DSH_REQUIRE(sens_atol_host[i] == sens_atol_host[0], "the wavefront-per-member kernels take one sens_atol for every state");
  const SensSpec sp{sens_out, sens_rtol, sens_atol_host, nsens_atol};
  return sdirk_solve_wave_member_impl({ctx, model, size, nb, p, atol, atol_nb, rtol, t0, h0, opts, t_eval_host, n_eval, y_out, stats, status, nullptr, nullptr, nullptr, totals_host, &sp, nullptr}, method);
}
static int sdirk_solve_wave_member_impl(const SolveArgs& a, int method) {
  static const char* const who = "dsh_sdirk_solve_wave_member";
  DSH_REQUIRE_AS(who, method == 1 || method == 2, "method: 1 TR-BDF2, 2 ESDIRK34");
  if (const int rc = check_solve_args(a, who); rc != DSH_OK) return rc;
  dsh_ctx* const ctx = a.ctx;
  const int model = a.model;
  const int64_t size = a.size, nb = a.nb;
  const bool sens = a.sens != nullptr;
  const int wm_kind = dsh_model_has_wave_member_sdirk(model, size);  // 2: one workgroup per member (64 < n <= 320, identity mass)
  if (!wm_kind) { set_error("dsh_sdirk_solve_wave_member: needs a run-time-sized model (built-in or DiffSL) with n <= 64 (n <= 48 with a mass matrix; 64 < n <= 320 without one) and at most two stop conditions"); return DSH_E_UNSUPPORTED; }
  if (nb == 0) return DSH_OK;
  int64_t n = 0, np = 0, nroots = 0;
  int has_mass = 0;
  if (const int rc = dsh_model_info(model, size, &n, &np, &has_mass, &nroots); rc != DSH_OK) return rc;
  WaveSdirkConsts C;
  std::memset((void*)&C, 0, sizeof C);
  C.model = model; C.n = (int)n; C.np = (int)np; C.nroots = (int)nroots;
  fill_tableau(method, C.T);  // resets the steps fields: ahead of fill_steps
  fill_steps(C.T, a.steps);
  fill_sens_one(C.T, a.sens);
  fill_resident(C.T.r, a);
  const int ab = a.atol_nb == 1 ? 1 : 0;
  const int S = C.T.s;
  ResidentLaunch L(ctx);
  if (wm_kind == 2) {
    // one workgroup per member (64 < n <= 320): the factors in LDS, the cached Jacobians in global scratch (n^2 doubles per member) — k_sdirk_wave_member<.., TW>
    const int waves = team_waves((int)n);
    const size_t lds_team = sizeof(double) * team_lds_doubles((int)n, waves);
    double* jac_scratch = nullptr;
    if (const int rc = L.blocks.take((int64_t)(sizeof(double) * team_scratch_doubles((int)n, waves)) * nb, 0, &jac_scratch); rc != DSH_OK) return rc;
    if (const int rc = L.open(&C, sizeof C, a.t_eval_host, a.n_eval); rc != DSH_OK) return rc;
    const WaveSdirkConsts* const consts_dev = (const WaveSdirkConsts*)L.consts;
    if (is_jit_model(model)) {
      const std::string name = std::string("dsh::k_sdirk_wave_member<16, ") + std::to_string(S) + (sens ? ", true, " : ", false, ") + std::to_string(waves) + ">";
      const int rc = jit_launch(ctx, model, "dsh_jit_sdirk_wave_member.hpp", name, {name}, name, dim3((unsigned)nb), dim3(64 * waves), (unsigned)lds_team, nb, a.p, a.atol, ab, consts_dev,
                                L.t_eval, DSH_WM_OUT, jac_scratch);
      if (rc != DSH_OK) return rc;
    } else {
      static bool attr_dev[64] = {false};
      bool& attr = attr_dev[ctx->device & 63];
      if (!attr) {
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_sdirk_wave_member<16, 3, false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_sdirk_wave_member<16, 3, false, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_sdirk_wave_member<16, 4, false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        DSH_HIP_CHECK(hipFuncSetAttribute((const void*)k_sdirk_wave_member<16, 4, false, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr = true;
      }
#define DSH_TS_LAUNCH(SV, TWV)                                                                                                                                      \
  hipLaunchKernelGGL((k_sdirk_wave_member<16, SV, false, TWV>), dim3((unsigned)nb), dim3(64 * TWV), lds_team, ctx->stream, nb, a.p, a.atol, ab, consts_dev, L.t_eval, \
                     DSH_WM_OUT, jac_scratch)
      if (S == 3) { if (waves == 2) DSH_TS_LAUNCH(3, 2); else if (waves == 3) DSH_TS_LAUNCH(3, 3); else if (waves == 4) DSH_TS_LAUNCH(3, 4); else DSH_TS_LAUNCH(3, 5); }
      else { if (waves == 2) DSH_TS_LAUNCH(4, 2); else if (waves == 3) DSH_TS_LAUNCH(4, 3); else if (waves == 4) DSH_TS_LAUNCH(4, 4); else DSH_TS_LAUNCH(4, 5); }
#undef DSH_TS_LAUNCH
    }
  } else {
    const size_t lds_bytes = sizeof(double) * (128 + (size_t)n * 64 + (has_mass ? (size_t)n * 64 + 64 : (sens ? 64 : 0)));  // xs | ps | sJ | (sM | xs2)  (sensitivities: xs2)
    if (const int rc = L.open(&C, sizeof C, a.t_eval_host, a.n_eval); rc != DSH_OK) return rc;
    const WaveSdirkConsts* const consts_dev = (const WaveSdirkConsts*)L.consts;
#define DSH_WS_LAUNCH(NPV, SV)                                                                                                                                    \
  hipLaunchKernelGGL((k_sdirk_wave_member<NPV, SV>), dim3((unsigned)nb), dim3(64), lds_bytes, ctx->stream, nb, a.p, a.atol, ab, consts_dev, L.t_eval, DSH_WM_OUT, \
                     (double*)nullptr)
#define DSH_WS_LAUNCH_S(NPV) do { if (S == 3) DSH_WS_LAUNCH(NPV, 3); else DSH_WS_LAUNCH(NPV, 4); } while (0)
    if (is_jit_model(model)) {
      const std::string name = std::string("dsh::k_sdirk_wave_member<") + (n <= 16 ? "16" : n <= 32 ? "32" : n <= 48 ? "48" : "64") + ", " + std::to_string(S) + (sens ? ", true>" : ">");
      const int rc = jit_launch(ctx, model, "dsh_jit_sdirk_wave_member.hpp", name, {name}, name, dim3((unsigned)nb), dim3(64), (unsigned)lds_bytes, nb, a.p, a.atol, ab, consts_dev,
                                L.t_eval, DSH_WM_OUT, (double*)nullptr);
      if (rc != DSH_OK) return rc;
    } else if (n <= 16) DSH_WS_LAUNCH_S(16);
    else if (n <= 32) DSH_WS_LAUNCH_S(32);
    else if (n <= 48) DSH_WS_LAUNCH_S(48);
    else DSH_WS_LAUNCH_S(64);
#undef DSH_WS_LAUNCH_S
#undef DSH_WS_LAUNCH
  }
#undef DSH_WM_OUT
  return L.close(a.totals_host);
}

}  // extern "C"
