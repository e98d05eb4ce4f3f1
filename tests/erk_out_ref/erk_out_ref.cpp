// CHECKER — TEST INFRASTRUCTURE ONLY.  Not part of the product path.
//
// Independent CPU restatement of diffsol's explicit Runge-Kutta integrator with the output equations integrated alongside the states (OdeBuilder::integrate_out(true)
// over problem.tsit45()): the solver state carries g(t) = integral of out(y, t), over the oracle's headers and the plain Tsit45 checker (tests/erk_ref/erk_ref.cpp:
// tableau, controller, stop time, dense output, problem set-up — included read-only).  Written from the reference (paths relative to its crates/diffsol/src):
//   ode_solver/state.rs:1097-1109          new_without_initialise: g = 0, dg = out(y0, t0); a model without out integrates its state (identity output)
//   ode_solver/runge_kutta.rs:529-533      start_step_attempt: gdiff[:, 0] = h dg;  :568-575 do_stage: old_state.dg = out(stage point, t + c_i h), gdiff[:, i] = h old_state.dg;
//                            :802-810      error_norm: gdiff d against state.g with out_rtol / out_atol, max-chained after the states' norm (only with output tolerances);
//                            :900-909      step_accepted: old_state.g = state.g + gdiff b, then the swap;  :1185-1235 interpolate_out_inplace;  :396-434 state_mut_back
//   ode_solver/method.rs:830-840, :859-877 solve_dense / solve write g where they write out(y) or y without integrate_out
#include "../erk_ref/erk_ref.cpp"

namespace {

struct ExplicitRkOut : ExplicitRk {
  bool integrate_out = false, out_error_control = false;
  int nout = 0;
  double out_rtol = 0.0;
  V out_atol;                   // nout x 1
  V g, dg, old_g, old_dg;       // state.g / state.dg, old_state.g / old_state.dg
  M gdiff;                      // nout x stages
  V out_error;
  const ExternalModel* ext = nullptr;  // a DiffSL host twin with out_i; null: identity output

  ExplicitRkOut(const Problem* p, Tableau t, bool on, double ortol, const double* oatol, int noatol) : ExplicitRk(p, std::move(t)), integrate_out(on) {
    if (mass_refused || init_error != OdeErr::Ok || !on) return;
    const int n = p->n(), nb = p->nb();
    ext = dynamic_cast<const ExternalModel*>(p->eqn->model.get());
    if (ext && ext->nout == 0) ext = nullptr;
    nout = ext ? ext->nout : n;
    out_error_control = noatol > 0;
    out_rtol = ortol;
    out_atol = V(nout, 1);
    for (int k = 0; k < nout; ++k) out_atol.d[(size_t)k] = noatol == 0 ? 0.0 : (noatol == 1 ? oatol[0] : oatol[k]);
    g = V(nout, nb);
    dg = V(nout, nb);
    call_out(state.y, state.t, dg);
    old_g = g;
    old_dg = dg;
    gdiff = M(nout, tab.s, nb);
    out_error = V(nout, nb);
  }

  void call_out(const V& y, double t, V& o) const {
    if (!ext) { copy_from(o, y); return; }
    for (int b = 0; b < y.nb; ++b) ext->f.out(t, &y.d[(size_t)b * y.n], pr->eqn->pb(b), &o.d[(size_t)b * o.n]);
  }

  OdeErr step(StopReason& reason) override {  // explicit_rk.rs:196-243 with problem.integrate_out
    if (is_state_mutated) return OdeErr::InterpolationTimeOutsideCurrentStep;  // not restated (the state is never mutated here)
    double h = state.h;
    int nattempts = 0;
    double fac = 1.0, error_norm = 0.0;
    while (true) {
      {  // start_step_attempt (runge_kutta.rs:505-533)
        V c0(state.dy.n, state.dy.nb);
        axpy(c0, h, state.dy, 0.0);
        diff.set_column(0, c0);
        if (integrate_out) {
          V cg(nout, state.dy.nb);
          axpy(cg, h, dg, 0.0);
          gdiff.set_column(0, cg);
        }
      }
      for (int i = 1; i < tab.s; ++i) {
        do_stage(i, h);
        if (integrate_out) {  // :568-575, after do_stage(i, h) has left the stage point in old_state.y
          call_out(old_state.y, state.t + tab.c[(size_t)i] * h, old_dg);
          V cg(nout, state.dy.nb);
          axpy(cg, h, old_dg, 0.0);
          gdiff.set_column(i, cg);
        }
      }
      // error_norm (runge_kutta.rs:783-810)
      gemv_cols(diff, tab.s, 1.0, tab.d.data(), 0.0, error);
      error_norm = std::fmax(0.0, squared_norm(error, state.y, pr->atol, pr->rtol));
      if (integrate_out && out_error_control) {
        gemv_cols(gdiff, tab.s, 1.0, tab.d.data(), 0.0, out_error);
        error_norm = std::fmax(error_norm, squared_norm(out_error, g, out_atol, out_rtol));
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
    // step_accepted(h, h * factor, false) (runge_kutta.rs:894-960)
    if (integrate_out) {
      copy_from(old_g, g);
      gemv_cols(gdiff, tab.s, 1.0, tab.b.data(), 1.0, old_g);
    }
    old_state.t = state.t + h;
    old_state.h = h * fac;
    std::swap(old_state, state);
    if (integrate_out) { std::swap(old_g, g); std::swap(old_dg, dg); }
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

  OdeErr interpolate_out_inplace(double t, V& ret) const {  // runge_kutta.rs:1185-1235
    const bool is_forward = state.h > 0.0;
    if ((is_forward && (t > state.t || t < old_state.t)) || (!is_forward && (t < state.t || t > old_state.t))) return OdeErr::InterpolationTimeOutsideCurrentStep;
    const double dt = state.t - old_state.t;
    const double theta = dt == 0.0 ? 1.0 : (t - old_state.t) / dt;
    const int poly_order = tab.beta.nc, s_star = tab.beta.nr;
    std::vector<double> thetav{theta};
    for (int i = 1; i < poly_order; ++i) thetav.push_back(theta * thetav[(size_t)i - 1]);
    V beta_f(s_star, 1);
    gemv_cols(tab.beta, poly_order, 1.0, thetav.data(), 0.0, beta_f);
    copy_from(ret, old_g);
    gemv_cols(gdiff, s_star, 1.0, beta_f.d.data(), 1.0, ret);
    return OdeErr::Ok;
  }
};

}  // namespace

extern "C" {

// number of integrated outputs of a model: its out_i count, its state count without out_i
int erko_model_nout(int model_id, int model_size) {
  auto m = make_model(model_id, model_size);
  const ExternalModel* e = dynamic_cast<const ExternalModel*>(m.get());
  return e && e->nout > 0 ? e->nout : m->n;
}

// The reference's test harness (ode_solver/mod.rs:104-194, use_tstop = false) on one IVP: step while t < t_point, interpolate / interpolate_out there.
// y_out [npoints][n], g_out [npoints][nout] (integrate_out only); counters[3] = steps, error-test failures, right-hand sides.  Returns 0, -OdeErr, -100 for a mass matrix.
int erko_solve_to_points(int model_id, int model_size, const double* p, int np, double rtol, const double* atol, double t0, double h0, int integrate_out, double out_rtol,
                         const double* out_atol, int nout_atol, const double* t_points, int npoints, double* y_out, double* g_out, long* counters) {
  auto pr = make_problem(model_id, model_size, 1, p, np, rtol, atol, 1, t0, h0);
  ExplicitRkOut sv(pr.get(), tsit45(), integrate_out != 0, out_rtol, out_atol, nout_atol);
  if (sv.mass_refused) return -100;
  if (sv.init_error != OdeErr::Ok) return -(int)sv.init_error;
  const int n = pr->n();
  V tmp(n, 1), gtmp(sv.nout, 1);
  for (int k = 0; k < npoints; ++k) {
    while (std::fabs(sv.t()) < std::fabs(t_points[k])) {
      StopReason r;
      OdeErr e = sv.step(r);
      if (e != OdeErr::Ok) return -(int)e;
    }
    OdeErr e = sv.interpolate_inplace(t_points[k], tmp);
    if (e == OdeErr::Ok && integrate_out) e = sv.interpolate_out_inplace(t_points[k], gtmp);
    if (e != OdeErr::Ok) return -(int)e;
    std::memcpy(y_out + (size_t)k * n, tmp.d.data(), sizeof(double) * n);
    if (integrate_out) std::memcpy(g_out + (size_t)k * sv.nout, gtmp.d.data(), sizeof(double) * sv.nout);
  }
  if (counters) { counters[0] = sv.stats().number_of_steps; counters[1] = sv.stats().number_of_error_test_failures; counters[2] = pr->eqn->rhs_stats.calls; }
  return 0;
}

// solve_dense / solve for an ensemble, as erk_solve_ensemble of the plain checker (group, steps_cap, atol rows, the per-member arrays), with integrate_out: y_out holds
// the states as there, g_out [nsys][width][nout] the integrated outputs in the same columns (written only with integrate_out; at a root g interpolated at the root,
// columns never reached NaN, the column before the first step zero).  nout_atol = 0: the outputs stay out of the error test; 1: one out_atol; nout: one each.
// calls_out [nsys]: right-hand sides of the member's problem.  options: as erk_solve_ensemble's.  Returns the number of failed members.
int erko_solve_ensemble(int model_id, int model_size, int nsys, const double* p, int np, double rtol, const double* atol, int natol_rows, double t0, double h0,
                        int integrate_out, double out_rtol, const double* out_atol, int nout_atol, const double* t_eval, int nt, int nthreads, int group, int steps_cap,
                        double* y_out, double* g_out, double* t_out, long* stats_out, int* status_out, double* root_t_out, int* root_idx_out, int* ncols_out, long* calls_out,
                        const double* options) {
  const SolveOptions so(options);
  if (group < 1) group = 1;
  if (nthreads < 1) nthreads = 1;
  const int ngroups = (nsys + group - 1) / group;
  const int n_model = make_model(model_id, model_size)->n;
  std::vector<int> failed_per_thread((size_t)nthreads, 0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto work = [&](int tid) {
    for (int gi = tid; gi < ngroups; gi += nthreads) {
      const int s0 = gi * group, cnt = std::min(group, nsys - s0);
      auto pr = make_problem(model_id, model_size, cnt, p + (size_t)s0 * np, np, rtol, natol_rows == 1 ? atol : atol + (size_t)s0 * n_model, natol_rows, t0, h0, so);
      const int n = pr->n();
      const int width = steps_cap > 0 ? steps_cap : nt;
      ExplicitRkOut sv(pr.get(), tsit45(), integrate_out != 0, out_rtol, out_atol, nout_atol);
      const int no = sv.nout;
      int col = 0;
      OdeErr err = sv.mass_refused ? OdeErr::InterpolationTimeOutsideCurrentStep : sv.init_error;
      V tmp(n, cnt), gtmp(no, cnt);
      auto put = [&](int c, const V& v, const V* gv) {
        for (int b = 0; b < cnt; ++b) {
          std::memcpy(y_out + ((size_t)(s0 + b) * width + c) * n, v.d.data() + (size_t)b * n, sizeof(double) * n);
          if (gv) std::memcpy(g_out + ((size_t)(s0 + b) * width + c) * no, gv->d.data() + (size_t)b * no, sizeof(double) * no);
        }
      };
      auto steps_write = [&](double tw, const V& v, const V* gv) {
        if (col < steps_cap) { put(col, v, gv); for (int b = 0; b < cnt; ++b) t_out[(size_t)(s0 + b) * steps_cap + col] = tw; }
        col++;
      };
      const bool io = integrate_out != 0;
      bool rooted = false;
      if (err == OdeErr::Ok) {
        if (steps_cap > 0) steps_write(sv.t(), sv.y(), io ? &sv.g : nullptr);
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
        if (steps_cap > 0) { if (r != StopReason::RootFound) steps_write(sv.t(), sv.y(), io ? &sv.g : nullptr); }
        else
          while (col < nt && t_eval[col] <= upto) {
            (void)sv.interpolate_inplace(t_eval[col], tmp);
            if (io) (void)sv.interpolate_out_inplace(t_eval[col], gtmp);
            put(col, tmp, io ? &gtmp : nullptr);
            col++;
          }
        if (r == StopReason::TstopReached) break;
        if (r == StopReason::RootFound) {  // state_mut_back(root, integrate_out): y and g at the root
          (void)sv.interpolate_inplace(sv.root_time, tmp);
          if (io) (void)sv.interpolate_out_inplace(sv.root_time, gtmp);
          if (steps_cap > 0) steps_write(sv.root_time, tmp, io ? &gtmp : nullptr);
          else if (col < nt) { put(col, tmp, io ? &gtmp : nullptr); col++; }
          rooted = true;
          break;
        }
      }
      for (int b = 0; b < cnt; ++b) {
        const int m = s0 + b;
        if (ncols_out) ncols_out[m] = col;
        if (steps_cap == 0)
          for (int c2 = col; c2 < nt; ++c2) {
            for (int i = 0; i < n; ++i) y_out[((size_t)m * nt + c2) * n + i] = nan;
            if (io) for (int i = 0; i < no; ++i) g_out[((size_t)m * nt + c2) * no + i] = nan;
          }
        if (status_out) status_out[m] = capped ? kStatusMaxStepsExceeded : status_of(err);
        if (root_t_out) root_t_out[m] = rooted ? sv.root_time : nan;
        if (root_idx_out) root_idx_out[m] = rooted ? sv.root_index : -1;
        if (stats_out) {
          long* o = stats_out + (size_t)m * 5;
          o[0] = sv.stats().number_of_steps; o[1] = 0; o[2] = 0; o[3] = sv.stats().number_of_error_test_failures; o[4] = 0;
        }
        if (calls_out) calls_out[m] = pr->eqn->rhs_stats.calls;
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
