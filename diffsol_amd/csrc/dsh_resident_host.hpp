// The host half that every device-resident solve driver shares (dsh_adaptive.hip, dsh_sdirk_resident.hip, dsh_erk_resident.hip, dsh_wave_member.hip): the
// argument checks, the common constants, the device blocks of the call and the bracket around its launch.  A driver adds what is its own — model admission,
// tableau or BDF tables, grid, kernel — between fill_* and ResidentLaunch::open / close.  Host only: never included by a kernel header.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "dsh_internal.hpp"
#include "dsh_resident.hpp"
#include "dsh_bdf_tables.hpp"
#include "dsh_ctx_blocks.hpp"

namespace dsh {

struct SensSpec { double* out; double rtol; const double* atol_host; int64_t natol; };  // forward sensitivities in the same launch (the *_sens entry points)
struct OutSpec { double rtol; const double* atol_host; int64_t natol; };  // integrated outputs in place of the states (the Tsit45 *_out entry points); natol = 0: outside the error test
struct StepsSpec { double* t_out; int64_t cap; };  // OdeSolverMethod::solve: every accepted step out (the *_steps entry points; steps_cap of the consts)

// what every driver takes; the extern "C" entry points fill it
struct SolveArgs {
  dsh_ctx* ctx;
  int model;
  int64_t size, nb;
  const double* p;
  const double* atol;
  int64_t atol_nb;
  double rtol, t0, h0;
  const dsh_adaptive_options* opts;
  const double* t_eval_host;
  int64_t n_eval;
  double* y_out;
  int32_t* stats;
  int32_t* status;
  double* t_root;
  int32_t* root_idx;
  int32_t* ncols;
  int64_t* totals_host;
  const SensSpec* sens;
  const StepsSpec* steps;
  const OutSpec* intout = nullptr;
};

// DSH_REQUIRE under the name of the public entry family instead of the enclosing function's
#define DSH_REQUIRE_AS(who, cond, msg)                        \
  do {                                                        \
    if (!(cond)) {                                            \
      ::dsh::set_error(std::string(who) + ": " + (msg));      \
      return DSH_E_INVALID;                                   \
    }                                                         \
  } while (0)

inline int check_solve_args(const SolveArgs& a, const char* who) {
  DSH_REQUIRE_AS(who, a.ctx != nullptr, "ctx is null");
  DSH_REQUIRE_AS(who, a.n_eval >= 1 && a.t_eval_host != nullptr, "t_eval must hold at least one time");
  DSH_REQUIRE_AS(who, a.atol_nb == 1 || a.atol_nb == a.nb, "atol must be broadcast (nbatch 1) or per member");
  for (int64_t q = 0; q + 1 < a.n_eval; ++q) DSH_REQUIRE_AS(who, a.t_eval_host[q] <= a.t_eval_host[q + 1], "t_eval must be increasing (InvalidTEval)");
  DSH_REQUIRE_AS(who, a.t_eval_host[0] >= a.t0, "t_eval[0] before t0 (InvalidTEval)");
  return DSH_OK;
}

// the scalars of the call, the options or their defaults, and the constants of Convergence (convergence.rs:36-42) and of the line search (line_search.rs:100)
inline void fill_resident(ResidentConsts& r, const SolveArgs& a) {
  r.rtol = a.rtol; r.t0 = a.t0; r.h0 = a.h0; r.n_eval = (int)a.n_eval; r.member_lanes = 0;
  if (a.opts) r.o = *a.opts; else dsh_adaptive_default_options(&r.o);
  if (r.o.max_steps <= 0) r.o.max_steps = 10000000;
  r.eta_reset = std::pow(20.0, 1.25);
  r.eta_reset_ts = std::pow(100.0, 1.25);
  r.ls_steptol = std::pow(2.220446049250313e-16, 2.0 / 3.0);
}

// Forward sensitivities of the lane-per-member kernels: sens_atol per state (up to 4 states) or one value for every state (sens_pad = 1).  one_above_4: the kernel
// carries models with more than 4 states (BDF, TR-BDF2 / ESDIRK34 in the banded form), which take one value only.
template <class Consts>
int fill_sens(Consts& C, const SensSpec* sens, int model, int64_t size, bool one_above_4, const char* who) {
  if (!sens) return DSH_OK;
  C.sens_out = sens->out; C.sens_rtol = sens->rtol; C.sens_error_control = sens->natol > 0 ? 1 : 0;
  int64_t ns = 0, npar = 0, nroots = 0;
  int has_mass = 0;
  if (dsh_model_info(model, size, &ns, &npar, &has_mass, &nroots) != DSH_OK) return DSH_E_INVALID;
  DSH_REQUIRE_AS(who, sens->natol == 0 || sens->natol == 1 || sens->natol == ns, "sens_atol must have length 1 or nstates");
  if (one_above_4) {
    bool uniform = true;
    for (int64_t i = 1; i < sens->natol; ++i) uniform = uniform && sens->atol_host[i] == sens->atol_host[0];
    DSH_REQUIRE_AS(who, ns <= 4 || uniform, "device-resident sensitivities of models with more than 4 states take one sens_atol for every state");
  }
  C.sens_pad = ((one_above_4 && ns > 4) || sens->natol <= 1) ? 1 : 0;  // 1: sens_atol[0] for every state
  for (int64_t i = 0; i < 4 && i < ns; ++i) C.sens_atol[i] = sens->natol == 0 ? 0.0 : (sens->natol == 1 ? sens->atol_host[0] : sens->atol_host[i]);
  return DSH_OK;
}
// the wavefront- / workgroup-per-member kernels: one sens_atol for every state (the entry points refuse anything else), sens_pad = 1 with and without sensitivities
template <class Consts>
void fill_sens_one(Consts& C, const SensSpec* sens) {
  const double atol = sens && sens->natol > 0 ? sens->atol_host[0] : 0.0;
  C.sens_out = sens ? sens->out : nullptr; C.sens_rtol = sens ? sens->rtol : 0.0; C.sens_error_control = sens && sens->natol > 0 ? 1 : 0; C.sens_pad = 1;
  if constexpr (std::is_array_v<decltype(C.sens_atol)>) { for (double& v : C.sens_atol) v = atol; }
  else C.sens_atol = atol;
}

template <class Consts>
void fill_steps(Consts& C, const StepsSpec* steps) {
  if (steps) { C.steps_t_out = steps->t_out; C.steps_cap = (int)steps->cap; }
}

// Bdf::_new tables (bdf.rs:286-306) by the one function the lock-step fast kernel evaluates at compile time (dsh_bdf_tables.hpp: the same 64-bit patterns), and
// compute_r(order, 1.0) (bdf.rs:433-463) for the orders 1..5, stored 6x6 column-major
inline void fill_bdf_tables(double (&alpha)[6], double (&gamma)[6], double (&ec2)[6], double (&u)[5][36]) {
  const BdfTables T = bdf_new_tables();
  for (int i = 0; i <= 5; ++i) { alpha[i] = T.alpha[i]; gamma[i] = T.gamma[i]; ec2[i] = T.ec2[i]; }
  for (int ord = 1; ord <= 5; ++ord) {
    double* U = u[ord - 1];
    for (int k = 0; k < 36; ++k) U[k] = 0.0;
    for (int j = 0; j <= ord; ++j) U[j * 6 + 0] = 1.0;
    for (int j = 1; j <= ord; ++j)
      for (int i = 1; i <= ord; ++i) U[j * 6 + i] = U[j * 6 + i - 1] * ((double)i - 1.0 - 1.0 * (double)j) / (double)i;
  }
}

// f(std::bool_constant<a>, std::bool_constant<b>): run-time flags to the template arguments of a kernel (BA x WAVE)
template <class F>
void with_bools(bool a, bool b, F&& f) {
  if (a) { if (b) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
  else { if (b) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}
// the same with the stage count of the (E)SDIRK tableau: 3 (TR-BDF2) | 4 (ESDIRK34)
template <class F>
void with_bools_stages(bool a, bool b, int s, F&& f) {
  with_bools(a, b, [&](auto A, auto B) {
    if (s == 3) f(A, B, std::integral_constant<int, 3>{}); else f(A, B, std::integral_constant<int, 4>{});
  });
}

// The device side of one solve: constants, save points and the six totals, owned until the scope ends (CtxBlocks), and the bracket around the launch.
//   open : allocate, upload, zero the totals — then timing_begin, directly ahead of the driver's launch
//   close: launch error, timing_end directly after the launch, totals back, synchronise, timing_collect
// A block of the driver's own (the Jacobian scratch of the workgroup forms) is taken from `blocks` before open.  A driver never calls dsh_free.
struct ResidentLaunch {
  dsh_ctx* ctx;
  CtxBlocks blocks;
  const void* consts = nullptr;
  const double* t_eval = nullptr;
  unsigned long long* totals = nullptr;
  explicit ResidentLaunch(dsh_ctx* c) : ctx(c), blocks(c) {}

  // bdf_cache: keep constants and save points in the context's block between solves (the BDF driver only)
  int open(const void* consts_host, size_t cbytes, const double* t_eval_host, int64_t n_eval, bool bdf_cache = false) {
    const size_t tbytes = sizeof(double) * (size_t)n_eval;
    if (bdf_cache && tbytes <= 4096) {
      const int rc = from_cache(consts_host, cbytes, t_eval_host, tbytes);
      if (rc != DSH_OK) return rc;
    }
    if (!consts) {
      void* consts_dev = nullptr;
      double* t_eval_dev = nullptr;
      int rc = blocks.take((int64_t)cbytes, 0, &consts_dev);
      if (rc != DSH_OK) return rc;
      rc = blocks.take((int64_t)tbytes, 0, &t_eval_dev);
      if (rc != DSH_OK) return rc;
      DSH_HIP_CHECK(hipMemcpyAsync(consts_dev, consts_host, cbytes, hipMemcpyHostToDevice, ctx->stream));
      DSH_HIP_CHECK(hipMemcpyAsync(t_eval_dev, t_eval_host, tbytes, hipMemcpyHostToDevice, ctx->stream));
      consts = consts_dev; t_eval = t_eval_dev;
    }
    const int rc = blocks.take((int64_t)(sizeof(unsigned long long) * 8), 1, &totals);
    if (rc != DSH_OK) return rc;
    DSH_HIP_CHECK(timing_begin(ctx));
    return DSH_OK;
  }

  int close(int64_t* totals_host) {
    DSH_HIP_CHECK(hipGetLastError());
    DSH_HIP_CHECK(timing_end(ctx));
    unsigned long long got[8] = {0};
    DSH_HIP_CHECK(hipMemcpyAsync(got, totals, sizeof(unsigned long long) * 6, hipMemcpyDeviceToHost, ctx->stream));
    DSH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    DSH_HIP_CHECK(timing_collect(ctx));
    if (totals_host) for (int q = 0; q < 6; ++q) totals_host[q] = (int64_t)got[q];
    return DSH_OK;
  }

 private:
  // Repeated solves of one problem (a parameter study, the benchmark loop) pass the same constants and save points every time: they stay on the device and are
  // compared on the host, byte-wise (the caller memsets its block), instead of being uploaded again (two pageable host-to-device copies, ~15 us each on a 2.5 ms
  // solve).  One small block per context (one thread per context), released with it (dsh_ctx_destroy).  Without the block (out of memory): consts stays null.
  int from_cache(const void* consts_host, size_t cbytes, const double* t_eval_host, size_t tbytes) {
    if (!ctx->const_cache_dev && hipMalloc((void**)&ctx->const_cache_dev, cbytes + 4096) != hipSuccess) { (void)hipGetLastError(); ctx->const_cache_dev = nullptr; }
    if (!ctx->const_cache_dev) return DSH_OK;
    if (!ctx->const_cache_host) ctx->const_cache_host = new std::vector<unsigned char>();
    std::vector<unsigned char>& held = *ctx->const_cache_host;
    std::vector<unsigned char> now(cbytes + tbytes);
    std::memcpy(now.data(), consts_host, cbytes);
    std::memcpy(now.data() + cbytes, t_eval_host, tbytes);
    if (now != held) {
      held.swap(now);  // the staging vector must outlive the asynchronous copy: it is the cache itself
      const int rc = [&]() -> int {
        DSH_HIP_CHECK(hipMemcpyAsync(ctx->const_cache_dev, held.data(), held.size(), hipMemcpyHostToDevice, ctx->stream));
        DSH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return DSH_OK;
      }();
      if (rc != DSH_OK) { held.clear(); return rc; }  // what the device holds is unknown: the next call uploads again
    }
    consts = ctx->const_cache_dev;
    t_eval = (const double*)(ctx->const_cache_dev + cbytes);
    return DSH_OK;
  }
};

}  // namespace dsh
