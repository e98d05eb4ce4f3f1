// CHECKER — TEST INFRASTRUCTURE ONLY.  Not part of the product path.
//
// Independent CPU restatement of diffsol's explicit Runge-Kutta integrator with forward sensitivities, ExplicitRk<.., SensEquations> with the Tsit45 tableau
// (problem.tsit45_sens()), over the oracle's headers and the plain Tsit45 checker (tests/erk_ref/erk_ref.cpp: tableau, controller, stop time, dense output, problem
// set-up — included read-only).  Written from the reference (paths relative to its crates/diffsol/src):
//   ode_solver/state.rs:1001-1029          RkState::new_with_sensitivities: s_j = SensInit(t0) e_j, ds_j = SensRhs(s_j) about (y0, t0); the step size from the states alone
//   ode_equations/sens_equations.rs:62-70  SensInit;  :119-125 SensRhs::update_state (df/dp at the linearisation point);  :168-174 SensRhs::call_inplace: J x + (df/dp)_j
//   ode_solver/runge_kutta.rs:505-526      start_step_attempt: sdiff_j[:, 0] = h ds_j;  :578-607 do_stage: SensRhs about the stage point, old_state.s_j = s_j + sdiff_j a_row_i;
//                            :812-822      error_norm: sdiff_j d against state.s_j with the sensitivity tolerances, max-chained after the states' norm, j = 0, 1, ..;
//                            :894-930      step_accepted (the swap takes s and ds along);  :1237-1309 interpolate_sens_inplace
//   ode_solver/explicit_rk.rs:46-54, :196-243   ExplicitRk::step with the augmented equations
//   ode_solver/mod.rs:104-194              the test harness (interpolate / interpolate_sens at every point)
#include "../erk_ref/erk_ref.cpp"

namespace {

struct ExplicitRkSens : ExplicitRk {
  int naug = 0;
  std::vector<V> s, ds, old_s, old_ds;  // state.s / state.ds, old_state.s / old_state.ds
  std::vector<M> sdiff;                 // per parameter n x stages
  V sens_error, sens_y;                 // sens_y: the point SensRhs is linearised about
  M sens_mat;                           // df/dp there, n x np

  ExplicitRkSens(const Problem* p, Tableau t) : ExplicitRk(p, std::move(t)) {
    if (mass_refused || init_error != OdeErr::Ok) return;
    const int n = p->n(), nb = p->nb();
    naug = p->eqn->model->np;
    sens_mat = M(n, naug, nb);
    sens_y = V(n, nb);
    sens_error = V(n, nb);
    // new_with_sensitivities (state.rs:1001-1029).  The base constructor has set the step size already; set_step_size reads y, dy and the state equations only, so the
    // order of the two does not show in any number (the right-hand-side count is the same)
    s.assign((size_t)naug, V(n, nb));
    ds.assign((size_t)naug, V(n, nb));
    for (int j = 0; j < naug; ++j) p->eqn->init_sens(state.t, j, s[(size_t)j]);
    sens_update_state(state.y, state.t);
    for (int j = 0; j < naug; ++j) sens_rhs_call(j, s[(size_t)j], state.t, ds[(size_t)j]);
    old_s = s;
    old_ds = ds;
    sdiff.assign((size_t)naug, M(n, tab.s, nb));
  }

  void sens_update_state(const V& y, double t) {  // SensRhs::update_state
    pr->eqn->rhs_sens(y, t, sens_mat);
    copy_from(sens_y, y);
  }
  void sens_rhs_call(int index, const V& x, double t, V& y) const {  // SensRhs::call_inplace: the Jacobian product first, then the column of df/dp
    pr->eqn->jac_mul(sens_y, t, x, y);
    add_assign(y, sens_mat.column(index));
  }

  void do_stage_sens(int i, double h) {  // runge_kutta.rs:578-607, after do_stage(i, h) has left the stage point in old_state.y / old_state.dy
    const double t = state.t + tab.c[(size_t)i] * h;
    sens_update_state(old_state.y, t);
    for (int j = 0; j < naug; ++j) {
      copy_from(old_s[(size_t)j], s[(size_t)j]);
      gemv_cols(sdiff[(size_t)j], i, 1.0, a_rows[(size_t)i].data(), 1.0, old_s[(size_t)j]);
      sens_rhs_call(j, old_s[(size_t)j], t, old_ds[(size_t)j]);
      V col(state.y.n, state.y.nb);
      axpy(col, h, old_ds[(size_t)j], 0.0);
      sdiff[(size_t)j].set_column(i, col);
    }
  }

  OdeErr step(StopReason& reason) override {  // explicit_rk.rs:196-243 with augmented_eqn = Some(SensEquations)
    if (is_state_mutated) return OdeErr::InterpolationTimeOutsideCurrentStep;  // not restated (the state is never mutated here)
    double h = state.h;
    int nattempts = 0;
    double fac = 1.0, error_norm = 0.0;
    while (true) {
      {  // start_step_attempt (runge_kutta.rs:505-526)
        V c0(state.dy.n, state.dy.nb);
        axpy(c0, h, state.dy, 0.0);
        diff.set_column(0, c0);
        for (int j = 0; j < naug; ++j) {
          axpy(c0, h, ds[(size_t)j], 0.0);
          sdiff[(size_t)j].set_column(0, c0);
        }
      }
      for (int i = 1; i < tab.s; ++i) { do_stage(i, h); do_stage_sens(i, h); }
      // error_norm (runge_kutta.rs:783-822)
      gemv_cols(diff, tab.s, 1.0, tab.d.data(), 0.0, error);
      error_norm = std::fmax(0.0, squared_norm(error, state.y, pr->atol, pr->rtol));
      if (pr->sens_error_control)
        for (int j = 0; j < naug; ++j) {
          gemv_cols(sdiff[(size_t)j], tab.s, 1.0, tab.d.data(), 0.0, sens_error);
          error_norm = std::fmax(error_norm, squared_norm(sens_error, s[(size_t)j], pr->sens_atol, pr->sens_rtol));
        }
      fac = factor(error_norm, 1.0);
      if (error_norm < 1.0) break;
      h *= fac;
      nattempts += 1;
      prev_error_norm.reset();
      statistics.number_of_error_test_failures += 1;
      if (nattempts >= maximum_error_test_failures) return OdeErr::TooManyErrorTestFailures;
      if (std::fabs(h) < minimum_timestep) return OdeErr::StepSizeTooSmall;
    }
    prev_error_norm = error_norm;
    // step_accepted(h, h * factor, false) (runge_kutta.rs:894-960): the swap of old_state and state takes s and ds along
    old_state.t = state.t + h;
    old_state.h = h * fac;
    std::swap(old_state, state);
    std::swap(old_s, s);
    std::swap(old_ds, ds);
    statistics.number_of_steps += 1;
    if (tstop) {
      std::optional<StopReason> r;
      OdeErr e = handle_tstop(*tstop, r);
      if (e != OdeErr::Ok) return e;
      if (r && *r == StopReason::TstopReached) { tstop.reset(); reason = StopReason::TstopReached; return OdeErr::Ok; }
    }
    reason = StopReason::InternalTimestep;
    return OdeErr::Ok;
  }

  OdeErr interpolate_sens_inplace(double t, std::vector<V>& ret) const {  // runge_kutta.rs:1237-1309
    const bool is_forward = state.h > 0.0;
    if ((is_forward && (t > state.t || t < old_state.t)) || (!is_forward && (t < state.t || t > old_state.t))) return OdeErr::InterpolationTimeOutsideCurrentStep;
    const double dt = state.t - old_state.t;
    const double theta = dt == 0.0 ? 1.0 : (t - old_state.t) / dt;
    const int poly_order = tab.beta.nc, s_star = tab.beta.nr;
    std::vector<double> thetav{theta};
    for (int i = 1; i < poly_order; ++i) thetav.push_back(theta * thetav[(size_t)i - 1]);
    V beta_f(s_star, 1);
    gemv_cols(tab.beta, poly_order, 1.0, thetav.data(), 0.0, beta_f);
    for (int j = 0; j < naug; ++j) {
      copy_from(ret[(size_t)j], old_s[(size_t)j]);
      gemv_cols(sdiff[(size_t)j], s_star, 1.0, beta_f.d.data(), 1.0, ret[(size_t)j]);
    }
    return OdeErr::Ok;
  }
};

// make_problem of the plain checker plus the sensitivity tolerances (builder.rs build_atols: one vector for every parameter); nsens_atol = 0: the sensitivities stay out of
// the error control (turn_off_sensitivities_error_control), 1: one value for every state, n: per state
std::unique_ptr<Problem> make_sens_problem(int model_id, int model_size, int cnt, const double* p, int np, double rtol, const double* atol, int natol_rows, double t0, double h0,
                                           double sens_rtol, const double* sens_atol, int nsens_atol, const SolveOptions& so = SolveOptions(nullptr)) {
  auto pr = make_problem(model_id, model_size, cnt, p, np, rtol, atol, natol_rows, t0, h0, so);
  pr->sens = true;
  pr->sens_error_control = nsens_atol > 0;
  pr->sens_rtol = sens_rtol;
  pr->sens_atol = V(pr->n(), 1);
  for (int i = 0; i < pr->n(); ++i) pr->sens_atol.d[(size_t)i] = nsens_atol == 0 ? 0.0 : (nsens_atol == 1 ? sens_atol[0] : sens_atol[i]);
  if (!pr->eqn->model->has_sens) throw std::runtime_error("checker: the model has no parameter sensitivities");
  return pr;
}

}  // namespace

extern "C" {

// The reference's test harness (ode_solver/mod.rs:104-194, use_tstop = false) on one IVP with sensitivities: step while t < t_point, interpolate / interpolate_sens there.
// y_out [npoints][n], s_out [npoints][np][n]; counters[4] = steps, error-test failures, right-hand sides, Jacobian products.  Returns 0, -OdeErr, -100 for a mass matrix,
// -101 for a model without parameter derivatives.
int erks_solve_to_points(int model_id, int model_size, const double* p, int np, double rtol, const double* atol, double t0, double h0, double sens_rtol, const double* sens_atol,
                         int nsens_atol, const double* t_points, int npoints, double* y_out, double* s_out, long* counters) {
  std::unique_ptr<Problem> pr;
  try { pr = make_sens_problem(model_id, model_size, 1, p, np, rtol, atol, 1, t0, h0, sens_rtol, sens_atol, nsens_atol); } catch (const std::exception&) { return -101; }
  ExplicitRkSens sv(pr.get(), tsit45());
  if (sv.mass_refused) return -100;
  if (sv.init_error != OdeErr::Ok) return -(int)sv.init_error;
  const int n = pr->n();
  V tmp(n, 1);
  std::vector<V> stmp((size_t)np, V(n, 1));
  for (int k = 0; k < npoints; ++k) {
    while (std::fabs(sv.t()) < std::fabs(t_points[k])) {
      StopReason r;
      OdeErr e = sv.step(r);
      if (e != OdeErr::Ok) return -(int)e;
    }
    OdeErr e = sv.interpolate_inplace(t_points[k], tmp);
    if (e == OdeErr::Ok) e = sv.interpolate_sens_inplace(t_points[k], stmp);
    if (e != OdeErr::Ok) return -(int)e;
    std::memcpy(y_out + (size_t)k * n, tmp.d.data(), sizeof(double) * n);
    for (int j = 0; j < np; ++j) std::memcpy(s_out + ((size_t)k * np + j) * n, stmp[(size_t)j].d.data(), sizeof(double) * n);
  }
  if (counters) {
    counters[0] = sv.stats().number_of_steps; counters[1] = sv.stats().number_of_error_test_failures;
    counters[2] = pr->eqn->rhs_stats.calls; counters[3] = pr->eqn->rhs_stats.jac_muls;
  }
  return 0;
}

// solve_dense_sensitivities for an ensemble: group = 1 every member its own IVP, group = G consecutive groups of G members as one lock-step batched problem each (the
// sensitivity norms are max-reduced over the group like the states').  y_out [nsys][nt][n], s_out [nsys][nt][np][n] (columns never reached: NaN), atol [n]
// (natol_rows = 1) or [nsys][n]; stats_out [nsys][5] (steps, 0, 0, error-test failures, 0), status_out [nsys], calls_out [nsys][2] (right-hand sides, Jacobian
// products of the member's problem).  options: as erk_solve_ensemble's.  Returns the number of failed members, or -101 for a model without parameter derivatives.
int erks_solve_ensemble(int model_id, int model_size, int nsys, const double* p, int np, double rtol, const double* atol, int natol_rows, double t0, double h0, double sens_rtol,
                        const double* sens_atol, int nsens_atol, const double* t_eval, int nt, int nthreads, int group, double* y_out, double* s_out, long* stats_out,
                        int* status_out, long* calls_out, const double* options) {
  const SolveOptions so(options);
  if (group < 1) group = 1;
  if (nthreads < 1) nthreads = 1;
  {
    auto m = make_model(model_id, model_size);
    if (!m->has_sens) return -101;
  }
  const int ngroups = (nsys + group - 1) / group;
  const int n_model = make_model(model_id, model_size)->n;
  std::vector<int> failed_per_thread((size_t)nthreads, 0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto work = [&](int tid) {
    for (int g = tid; g < ngroups; g += nthreads) {
      const int s0 = g * group, cnt = std::min(group, nsys - s0);
      auto pr = make_sens_problem(model_id, model_size, cnt, p + (size_t)s0 * np, np, rtol, natol_rows == 1 ? atol : atol + (size_t)s0 * n_model, natol_rows, t0, h0, sens_rtol,
                                  sens_atol, nsens_atol, so);
      const int n = pr->n();
      ExplicitRkSens sv(pr.get(), tsit45());
      int col = 0;
      OdeErr err = sv.mass_refused ? OdeErr::InterpolationTimeOutsideCurrentStep : sv.init_error;
      V tmp(n, cnt);
      std::vector<V> stmp((size_t)np, V(n, cnt));
      if (err == OdeErr::Ok) err = sv.set_stop_time(t_eval[nt - 1]);
      StepGuard cap(so);
      bool capped = false;
      while (err == OdeErr::Ok) {
        if (!cap.next()) { capped = true; break; }
        StopReason r;
        err = sv.step(r);
        if (err != OdeErr::Ok) break;
        while (col < nt && t_eval[col] <= sv.t()) {
          (void)sv.interpolate_inplace(t_eval[col], tmp);
          (void)sv.interpolate_sens_inplace(t_eval[col], stmp);
          for (int b = 0; b < cnt; ++b) {
            std::memcpy(y_out + ((size_t)(s0 + b) * nt + col) * n, tmp.d.data() + (size_t)b * n, sizeof(double) * n);
            for (int j = 0; j < np; ++j) std::memcpy(s_out + (((size_t)(s0 + b) * nt + col) * np + j) * n, stmp[(size_t)j].d.data() + (size_t)b * n, sizeof(double) * n);
          }
          col++;
        }
        if (r == StopReason::TstopReached) break;
      }
      for (int b = 0; b < cnt; ++b) {
        const int m = s0 + b;
        for (int c2 = col; c2 < nt; ++c2) {
          for (int i = 0; i < n; ++i) y_out[((size_t)m * nt + c2) * n + i] = nan;
          for (int i = 0; i < np * n; ++i) s_out[((size_t)m * nt + c2) * np * n + i] = nan;
        }
        if (status_out) status_out[m] = capped ? kStatusMaxStepsExceeded : status_of(err);
        if (stats_out) {
          long* o = stats_out + (size_t)m * 5;
          o[0] = sv.stats().number_of_steps; o[1] = 0; o[2] = 0; o[3] = sv.stats().number_of_error_test_failures; o[4] = 0;
        }
        if (calls_out) { calls_out[(size_t)m * 2] = pr->eqn->rhs_stats.calls; calls_out[(size_t)m * 2 + 1] = pr->eqn->rhs_stats.jac_muls; }
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
