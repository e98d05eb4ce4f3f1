// CHECKER — TEST INFRASTRUCTURE ONLY.  Not part of the product path.
//
// Independent CPU restatement of diffsol's explicit Runge-Kutta integrator with the Tsit45 tableau, over the oracle's existing headers (vectors, models and DiffSL
// host twins, Tableau, root finder, problem set-up: included read-only).  Written from the reference (paths relative to its crates/diffsol/src):
//   ode_solver/tableau.rs:161-304         Tableau::tsit45 (first column of `a` computed as there, :221-227)
//   ode_solver/runge_kutta.rs:107-194     Rk::_new;  :232-284 check_explicit_rk;  :436-444 set_stop_time;  :446-464 start_step;  :466-495 factor;
//                            :505-516     start_step_attempt;  :537-566 do_stage;  :752-781 handle_tstop;  :783-800 error_norm;  :843-867 error_test_fail;
//                            :894-960     step_accepted;  :962-1002 beta-polynomial dense output;  :1080-1127 interpolate_inplace;  :1313-1336 pi_controller_raw
//   ode_solver/explicit_rk.rs:196-243     ExplicitRk::step;  ode_solver/config.rs:132-160 ExplicitRkConfig
//   ode_solver/method.rs:227-258, :467-520, :881-961   solve / solve_dense
#include <dlfcn.h>

#include <cstring>
#include <thread>

#include "../../oracle/oracle_ode.hpp"
#include "../../oracle/oracle_sdirk.hpp"

using namespace orc;

namespace {

Tableau tsit45() {  // tableau.rs:161-304
  Tableau t;
  t.s = 7; t.order = 4;
  t.c = {0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0};
  t.b = {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774, 0.0};
  t.d = {-0.001780011052225777, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552, -0.45808210592918697, 0.015151515151515152};
  t.a = M(7, 7, 1);
  t.a.at(0, 2, 1) = 0.335480655492357;
  t.a.at(0, 3, 1) = -6.359448489975075;
  t.a.at(0, 4, 1) = -11.74888356406283;
  t.a.at(0, 5, 1) = -12.92096931784711;
  t.a.at(0, 3, 2) = 4.362295432869581;
  t.a.at(0, 4, 2) = 7.495539342889836;
  t.a.at(0, 5, 2) = 8.159367898576159;
  t.a.at(0, 4, 3) = -0.09249506636175525;
  t.a.at(0, 5, 3) = -0.071584973281401;
  t.a.at(0, 5, 4) = -0.02826905039406838;
  for (int i = 1; i < 7; ++i) {  // :221-227
    double a_sum = 0.0;
    for (int j = 1; j < i; ++j) a_sum += t.A(i, j);
    t.a.at(0, i, 0) = t.c[(size_t)i] - a_sum;
  }
  for (int j = 0; j < 6; ++j) t.a.at(0, 6, j) = t.b[(size_t)j];
  t.has_beta = true;
  t.beta = M(7, 4, 1);  // column-major 7 x 4 (:266-300)
  t.beta.d = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
              -2.76370619727483, 0.1317, 3.93029623689475, -12.4110771669337, 37.509313416511, -27.8965262891973, 1.5,
              2.91325546182191, -0.2234, -5.9410338721315, 30.3381886302823, -88.1789048947664, 65.0918946747937, -4.0,
              -1.05308849772902, 0.1017, 2.49062728565125, -16.5481028892449, 47.3795219628193, -34.8706578614966, 2.5};
  return t;
}

struct ExplicitRk : SolverBase {
  const Problem* pr;
  Tableau tab;
  Stats statistics;
  std::vector<std::vector<double>> a_rows;
  M diff;  // n x s
  V error;
  StateCommon state, old_state;
  std::optional<double> tstop;
  std::optional<RootFinder> root_finder;
  std::optional<double> prev_error_norm;
  bool is_state_mutated = false;
  // config.rs:141-160
  double minimum_timestep, maximum_timestep_growth, minimum_timestep_growth, maximum_timestep_shrink, minimum_timestep_shrink;
  int maximum_error_test_failures;
  OdeErr init_error = OdeErr::Ok;
  bool mass_refused = false;

  ExplicitRk(const Problem* p, Tableau t) : pr(p), tab(std::move(t)) {
    const OdeSolverOptions& o = p->ode_options;
    minimum_timestep = o.min_timestep;
    maximum_error_test_failures = o.max_error_test_failures;
    maximum_timestep_growth = o.max_timestep_growth.value_or(2.0);
    minimum_timestep_growth = o.min_timestep_growth.value_or(1.0);
    maximum_timestep_shrink = o.max_timestep_shrink.value_or(1.0);
    minimum_timestep_shrink = o.min_timestep_shrink.value_or(0.5);
    if (p->eqn->has_mass()) { mass_refused = true; return; }  // check_explicit_rk (runge_kutta.rs:236-239): MassMatrixNotSupported
    // problem.tsit45(): RkState::new_and_consistent(problem, tableau.order())
    init_error = new_and_consistent(*p, tab.order, state);
    if (init_error != OdeErr::Ok) return;
    const int n = p->n(), nb = p->nb();
    for (int i = 0; i < tab.s; ++i) { std::vector<double> row; for (int j = 0; j < i; ++j) row.push_back(tab.A(i, j)); a_rows.push_back(row); }
    if (p->eqn->model->nroots > 0) { root_finder.emplace(p->eqn->model->nroots, n, nb); root_finder->init(*p->eqn, state.y, state.t); }
    diff = M(n, tab.s, nb);
    old_state = state;
    error = V(n, nb);
  }

  OdeErr handle_tstop(double ts, std::optional<StopReason>& out) {  // runge_kutta.rs:752-781
    out.reset();
    const double eps = std::numeric_limits<double>::epsilon();
    const double troundoff = 100.0 * eps * (std::fabs(state.t) + std::fabs(state.h));
    if (std::fabs(state.t - ts) <= troundoff) { out = StopReason::TstopReached; return OdeErr::Ok; }
    if ((state.h > 0.0 && ts < state.t - troundoff) || (state.h < 0.0 && ts > state.t + troundoff)) return OdeErr::StopTimeBeforeCurrentTime;
    if ((state.h > 0.0 && state.t + state.h > ts + troundoff) || (state.h < 0.0 && state.t + state.h < ts - troundoff)) {
      const double factor = (ts - state.t) / state.h;
      state.h *= factor;
    }
    return OdeErr::Ok;
  }
  OdeErr set_stop_time(double ts) override {  // runge_kutta.rs:436-444
    tstop = ts;
    std::optional<StopReason> r;
    OdeErr e = handle_tstop(ts, r);
    if (e != OdeErr::Ok) return e;
    if (r && *r == StopReason::TstopReached) { tstop.reset(); return OdeErr::StopTimeAtCurrentTime; }
    return OdeErr::Ok;
  }

  void do_stage(int i, double h) {  // runge_kutta.rs:537-566
    const double t = state.t + tab.c[(size_t)i] * h;
    copy_from(old_state.y, state.y);
    gemv_cols(diff, i, 1.0, a_rows[(size_t)i].data(), 1.0, old_state.y);
    pr->eqn->rhs(old_state.y, t, old_state.dy);
    V col(state.y.n, state.y.nb);
    axpy(col, h, old_state.dy, 0.0);
    diff.set_column(i, col);
  }

  double factor(double error_norm, double safety_factor) const {  // runge_kutta.rs:466-495
    const double safety = 0.9 * safety_factor;
    const double raw = pi_controller_raw(error_norm, prev_error_norm, pr->ode_options.pi_control_integral, pr->ode_options.pi_control_proportional, tab.order + 1);
    double f = safety * raw;
    if (f > maximum_timestep_shrink && f < minimum_timestep_growth) f = 1.0;
    if (f < minimum_timestep_shrink) f = minimum_timestep_shrink;
    if (f > maximum_timestep_growth) f = maximum_timestep_growth;
    return f;
  }

  OdeErr step(StopReason& reason) override {  // explicit_rk.rs:196-243
    if (is_state_mutated) {  // Rk::start_step (runge_kutta.rs:446-464)
      if (root_finder) root_finder->init(*pr->eqn, state.y, state.t);
      if (tstop) { OdeErr e = set_stop_time(*tstop); if (e != OdeErr::Ok) return e; }
      is_state_mutated = false;
    }
    double h = state.h;
    int nattempts = 0;
    double fac = 1.0, error_norm = 0.0;
    while (true) {
      {  // start_step_attempt (runge_kutta.rs:505-516): the first stage is h * dy of the previous step's last stage
        V c0(state.dy.n, state.dy.nb);
        axpy(c0, h, state.dy, 0.0);
        diff.set_column(0, c0);
      }
      for (int i = 1; i < tab.s; ++i) do_stage(i, h);
      // error_norm (runge_kutta.rs:783-800) with the identity as linear solver
      gemv_cols(diff, tab.s, 1.0, tab.d.data(), 0.0, error);
      error_norm = std::fmax(0.0, squared_norm(error, state.y, pr->atol, pr->rtol));
      fac = factor(error_norm, 1.0);
      if (error_norm < 1.0) break;
      h *= fac;
      nattempts += 1;
      prev_error_norm.reset();
      statistics.number_of_error_test_failures += 1;  // error_test_fail (runge_kutta.rs:843-867)
      if (nattempts >= maximum_error_test_failures) return OdeErr::TooManyErrorTestFailures;
      if (std::fabs(h) < minimum_timestep) return OdeErr::StepSizeTooSmall;
    }
    prev_error_norm = error_norm;
    // step_accepted(h, h * factor, false) (runge_kutta.rs:894-960)
    old_state.t = state.t + h;
    old_state.h = h * fac;
    std::swap(old_state, state);
    statistics.number_of_steps += 1;
    if (root_finder) {
      auto interp = [&](double tt, V& yy) { (void)interpolate_inplace(tt, yy); };
      auto ret = root_finder->check_root(interp, *pr->eqn, state.y, state.t);
      if (root_finder->mismatch) return OdeErr::RootBatchMismatch;
      if (ret) { root_time = ret->first; root_index = ret->second; reason = StopReason::RootFound; return OdeErr::Ok; }
    }
    if (tstop) {
      std::optional<StopReason> r;
      OdeErr e = handle_tstop(*tstop, r);
      if (e != OdeErr::Ok) return e;
      if (r && *r == StopReason::TstopReached) { tstop.reset(); reason = StopReason::TstopReached; return OdeErr::Ok; }
    }
    reason = StopReason::InternalTimestep;
    return OdeErr::Ok;
  }

  OdeErr interpolate_inplace(double t, V& ret) const override {  // runge_kutta.rs:1080-1127, :962-981
    if (is_state_mutated) { if (t != state.t) return OdeErr::InterpolationTimeOutsideCurrentStep; copy_from(ret, state.y); return OdeErr::Ok; }
    const bool is_forward = state.h > 0.0;
    if ((is_forward && (t > state.t || t < old_state.t)) || (!is_forward && (t < state.t || t > old_state.t))) return OdeErr::InterpolationTimeOutsideCurrentStep;
    const double dt = state.t - old_state.t;
    const double theta = dt == 0.0 ? 1.0 : (t - old_state.t) / dt;
    const int poly_order = tab.beta.nc, s_star = tab.beta.nr;
    std::vector<double> thetav{theta};
    for (int i = 1; i < poly_order; ++i) thetav.push_back(theta * thetav[(size_t)i - 1]);
    V beta_f(s_star, 1);
    gemv_cols(tab.beta, poly_order, 1.0, thetav.data(), 0.0, beta_f);
    copy_from(ret, old_state.y);
    gemv_cols(diff, s_star, 1.0, beta_f.d.data(), 1.0, ret);
    return OdeErr::Ok;
  }
  OdeErr interpolate_dy_inplace(double, V&) const override { return OdeErr::InterpolationTimeOutsideCurrentStep; }  // not restated
  OdeErr state_mut_back(double) override { return OdeErr::InterpolationTimeOutsideCurrentStep; }                    // not restated (no resets here)
  OdeErr apply_reset() override { return OdeErr::InterpolationTimeOutsideCurrentStep; }
  const V& y() const override { return state.y; }
  const V& dy() const override { return state.dy; }
  double t() const override { return state.t; }
  double h() const override { return state.h; }
  int order() const override { return tab.order; }
  const Stats& stats() const override { return statistics; }
  const Problem& problem() const override { return *pr; }
};

// status codes of the device kernels (dsh_resident.hpp ResidentStatus): the OdeErr ordinal, 20 for a root batch mismatch
int status_of(OdeErr e) { return e == OdeErr::RootBatchMismatch ? 20 : (int)e; }

// The options of one ensemble solve, read from the caller's array of kNumSolveOptions doubles (null: every default), handed down per call: the groups of an
// ensemble run on threads, so nothing here is process-wide.  The first four are the reference's OdeSolverOptions fields that ExplicitRk reads
// (max_error_test_failures and min_timestep: runge_kutta.rs:843-867 through ExplicitRkConfig, config.rs:141-160; the two controller constants: :466-495 into :1313-1336).
// max_steps HAS NO COUNTERPART IN THE REFERENCE, whose solve loops run until the stop time, a root or an error: it is the device ABI's own limit
// (dsh_adaptive_options.max_steps), restated as the kernels document it — one count per step() call, tested before the step (++guard > max_steps), status 99
// (MaxStepsExceeded), a value <= 0 meaning 10 000 000.
constexpr int kNumSolveOptions = 5;
constexpr int kStatusMaxStepsExceeded = 99;
struct SolveOptions {
  OdeSolverOptions ode;
  long max_steps = 10000000;
  explicit SolveOptions(const double* v) {
    if (!v) return;
    ode.max_error_test_failures = (int)v[0];
    ode.min_timestep = v[1];
    ode.pi_control_integral = v[2];
    ode.pi_control_proportional = v[3];
    if ((long)v[4] > 0) max_steps = (long)v[4];
  }
};
// the step cap of the solve loops below: true when the step may be taken
struct StepGuard {
  long guard = 0, max_steps;
  explicit StepGuard(const SolveOptions& o) : max_steps(o.max_steps) {}
  bool next() { return !(++guard > max_steps); }
};

// one problem of `cnt` members (cnt = 1: an independent IVP; cnt > 1: a lock-step batched problem); atol: [n] (natol_rows = 1) or one row per member
std::unique_ptr<Problem> make_problem(int model_id, int model_size, int cnt, const double* p, int np, double rtol, const double* atol, int natol_rows, double t0, double h0,
                                      const SolveOptions& so = SolveOptions(nullptr)) {
  auto pr = std::make_unique<Problem>();
  pr->ode_options = so.ode;
  std::vector<double> pv(p, p + (size_t)np * cnt);
  pr->eqn = std::make_unique<Eqn>(make_model(model_id, model_size), cnt, pv);
  const int n = pr->n();
  pr->rtol = rtol;
  pr->atol = V(n, natol_rows == 1 ? 1 : cnt);
  std::memcpy(pr->atol.d.data(), atol, sizeof(double) * pr->atol.d.size());
  pr->t0 = t0; pr->h0 = h0;
  return pr;
}

}  // namespace

extern "C" {

void erk_set_det_pow(int on) { det_pow_flag() = on != 0; }

// out: c[7], b[7], d[7], a[7][7] row-major, beta[4][7] (power-major), then order: 99 doubles
void erk_tableau(double* out) {
  const Tableau t = tsit45();
  int k = 0;
  for (int i = 0; i < 7; ++i) out[k++] = t.c[(size_t)i];
  for (int i = 0; i < 7; ++i) out[k++] = t.b[(size_t)i];
  for (int i = 0; i < 7; ++i) out[k++] = t.d[(size_t)i];
  for (int i = 0; i < 7; ++i) for (int j = 0; j < 7; ++j) out[k++] = t.A(i, j);
  for (int q = 0; q < 4; ++q) for (int i = 0; i < 7; ++i) out[k++] = t.beta.at(0, i, q);
  out[k++] = (double)t.order;
}

int erk_model_dims(int model_id, int model_size, int* out3) {
  auto m = make_model(model_id, model_size);
  out3[0] = m->n; out3[1] = m->np; out3[2] = m->has_mass ? 1 : 0;
  return 0;
}

// load a CPU model library generated from DiffSL (Target::HostC) into THIS library's registry; returns its model id or -1
int erk_load_external_model(const char* path) {
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) return -1;
  ExternalFns f;
  f.dims = (decltype(f.dims))dlsym(h, "dsl_dims");
  f.rhs = (decltype(f.rhs))dlsym(h, "dsl_rhs");
  f.jac_mul = (decltype(f.jac_mul))dlsym(h, "dsl_jac_mul");
  f.mass_gemv = (decltype(f.mass_gemv))dlsym(h, "dsl_mass_gemv");
  f.init = (decltype(f.init))dlsym(h, "dsl_init");
  f.root = (decltype(f.root))dlsym(h, "dsl_root");
  f.out = (decltype(f.out))dlsym(h, "dsl_out");
  f.sens_mul = (decltype(f.sens_mul))dlsym(h, "dsl_sens_mul");
  f.init_sens_mul = (decltype(f.init_sens_mul))dlsym(h, "dsl_init_sens_mul");
  f.reset = (decltype(f.reset))dlsym(h, "dsl_reset");
  if (!f.dims || !f.rhs || !f.jac_mul || !f.mass_gemv || !f.init || !f.root || !f.out) return -1;
  external_models().push_back(f);
  return MODEL_EXTERNAL_BASE + (int)external_models().size() - 1;
}

// The reference's test harness (ode_solver/mod.rs:104-194) on one IVP: for each point, use_tstop ? set_stop_time(t) + step to TstopReached, y = state.y
// : step while t < t_point, y = interpolate(t_point).  y_out [npoints][n]; counters[3] = steps, error-test failures, rhs calls.  Returns 0, -OdeErr, or -100 for a
// mass matrix (MassMatrixNotSupported).
int erk_solve_to_points(int model_id, int model_size, const double* p, int np, double rtol, const double* atol, double t0, double h0, const double* t_points, int npoints,
                        int use_tstop, double* y_out, long* counters) {
  auto pr = make_problem(model_id, model_size, 1, p, np, rtol, atol, 1, t0, h0);
  ExplicitRk s(pr.get(), tsit45());
  if (s.mass_refused) return -100;
  if (s.init_error != OdeErr::Ok) return -(int)s.init_error;
  const int n = pr->n();
  V tmp(n, 1);
  for (int k = 0; k < npoints; ++k) {
    if (use_tstop) {
      OdeErr e = s.set_stop_time(t_points[k]);
      if (e == OdeErr::StopTimeAtCurrentTime) { std::memcpy(y_out + (size_t)k * n, s.y().d.data(), sizeof(double) * n); continue; }
      if (e != OdeErr::Ok) return -(int)e;
      while (true) {
        StopReason r;
        e = s.step(r);
        if (e != OdeErr::Ok) return -(int)e;
        if (r == StopReason::TstopReached) break;
      }
      std::memcpy(y_out + (size_t)k * n, s.y().d.data(), sizeof(double) * n);
    } else {
      while (std::fabs(s.t()) < std::fabs(t_points[k])) {
        StopReason r;
        OdeErr e = s.step(r);
        if (e != OdeErr::Ok) return -(int)e;
      }
      OdeErr e = s.interpolate_inplace(t_points[k], tmp);
      if (e != OdeErr::Ok) return -(int)e;
      std::memcpy(y_out + (size_t)k * n, tmp.d.data(), sizeof(double) * n);
    }
  }
  if (counters) { counters[0] = s.stats().number_of_steps; counters[1] = s.stats().number_of_error_test_failures; counters[2] = pr->eqn->rhs_stats.calls; }
  return 0;
}

// solve_dense (method.rs:467-520) / solve (:227-258, :881-961) for an ensemble: group = 1 every member its own IVP, group = G consecutive groups of G members as one
// lock-step batched problem each.  steps_cap = 0: states at t_eval, y_out [nsys][nt][n]; steps_cap > 0: t_eval[0] is the final time, every accepted step out,
// y_out [nsys][steps_cap][n], t_out [nsys][steps_cap] (columns beyond the cap are counted, not stored).  atol [n] (natol_rows = 1) or [nsys][n].
// stats_out [nsys][5] (steps, 0, 0, error-test failures, 0), status_out / root_t_out (NaN: none) / root_idx_out / ncols_out [nsys].  options: null, or the
// kNumSolveOptions doubles of SolveOptions (max_error_test_failures, min_timestep, pi_control_integral, pi_control_proportional, max_steps).  Returns the number of
// failed members.
int erk_solve_ensemble(int model_id, int model_size, int nsys, const double* p, int np, double rtol, const double* atol, int natol_rows, double t0, double h0,
                       const double* t_eval, int nt, int nthreads, int group, int steps_cap, double* y_out, double* t_out, long* stats_out, int* status_out,
                       double* root_t_out, int* root_idx_out, int* ncols_out, const double* options) {
  const SolveOptions so(options);
  if (group < 1) group = 1;
  if (nthreads < 1) nthreads = 1;
  const int ngroups = (nsys + group - 1) / group;
  const int n_model = make_model(model_id, model_size)->n;
  std::vector<int> failed_per_thread((size_t)nthreads, 0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto work = [&](int tid) {
    for (int g = tid; g < ngroups; g += nthreads) {
      const int s0 = g * group, cnt = std::min(group, nsys - s0);
      auto pr = make_problem(model_id, model_size, cnt, p + (size_t)s0 * np, np, rtol, natol_rows == 1 ? atol : atol + (size_t)s0 * n_model, natol_rows, t0, h0, so);
      const int n = pr->n();
      const int width = steps_cap > 0 ? steps_cap : nt;
      ExplicitRk sv(pr.get(), tsit45());
      int col = 0;
      OdeErr err = sv.mass_refused ? OdeErr::InterpolationTimeOutsideCurrentStep : sv.init_error;
      V tmp(n, cnt);
      auto put = [&](int c, const V& v) {
        for (int b = 0; b < cnt; ++b) std::memcpy(y_out + ((size_t)(s0 + b) * width + c) * n, v.d.data() + (size_t)b * n, sizeof(double) * n);
      };
      auto steps_write = [&](double tw, const V& v) {
        if (col < steps_cap) { put(col, v); for (int b = 0; b < cnt; ++b) t_out[(size_t)(s0 + b) * steps_cap + col] = tw; }
        col++;
      };
      bool rooted = false;
      if (err == OdeErr::Ok) {
        if (steps_cap > 0) steps_write(sv.t(), sv.y());
        err = sv.set_stop_time(t_eval[nt - 1]);
      }
      StepGuard cap(so);
      bool capped = false;
      while (err == OdeErr::Ok) {
        if (!cap.next()) { capped = true; break; }
        StopReason r;
        err = sv.step(r);
        if (err != OdeErr::Ok) break;
        const double upto = r == StopReason::RootFound ? sv.root_time : sv.t();
        if (steps_cap > 0) { if (r != StopReason::RootFound) steps_write(sv.t(), sv.y()); }
        else
          while (col < nt && t_eval[col] <= upto) { (void)sv.interpolate_inplace(t_eval[col], tmp); put(col, tmp); col++; }
        if (r == StopReason::TstopReached) break;
        if (r == StopReason::RootFound) {  // state_mut_back(root): the column after the drained ones holds the state at the root
          (void)sv.interpolate_inplace(sv.root_time, tmp);
          if (steps_cap > 0) steps_write(sv.root_time, tmp);
          else if (col < nt) { put(col, tmp); col++; }
          rooted = true;
          break;
        }
      }
      for (int b = 0; b < cnt; ++b) {
        const int m = s0 + b;
        if (ncols_out) ncols_out[m] = col;
        if (steps_cap == 0)
          for (int c2 = col; c2 < nt; ++c2) for (int i = 0; i < n; ++i) y_out[((size_t)m * nt + c2) * n + i] = nan;
        if (status_out) status_out[m] = capped ? kStatusMaxStepsExceeded : status_of(err);
        if (root_t_out) root_t_out[m] = rooted ? sv.root_time : nan;
        if (root_idx_out) root_idx_out[m] = rooted ? sv.root_index : -1;
        if (stats_out) {
          long* o = stats_out + (size_t)m * 5;
          o[0] = sv.stats().number_of_steps; o[1] = 0; o[2] = 0; o[3] = sv.stats().number_of_error_test_failures; o[4] = 0;
        }
      }
      if (err != OdeErr::Ok || capped) failed_per_thread[(size_t)tid] += cnt;
    }
  };
  std::vector<std::thread> th;
  for (int i = 0; i < nthreads; ++i) th.emplace_back(work, i);
  for (auto& t : th) t.join();
  int failed = 0;
  for (int f : failed_per_thread) failed += f;
  return failed;
}

}  // extern "C"
