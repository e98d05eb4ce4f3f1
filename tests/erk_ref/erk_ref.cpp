// CHECKER — TEST INFRASTRUCTURE ONLY.  Not part of the product path.
//
// Independent CPU restatement of diffsol's explicit Runge-Kutta integrator with the Tsit45 tableau, over the oracle's existing headers (vectors, models and DiffSL
// host twins, Tableau, root finder, problem set-up: included read-only).  One integrator in three modes: plain (problem.tsit45()), with forward sensitivities
// (ExplicitRk<.., SensEquations>, problem.tsit45_sens()), and with the output equations integrated alongside the states (OdeBuilder::integrate_out(true): the solver
// state carries g(t) = integral of out(y, t)).  The augmented work stands where the reference's own step branches on `augmented_eqn` or `integrate_out`.  Both at once
// is not a mode: the device refuses it and no entry point asks for it.  Written from the reference (paths relative to its crates/diffsol/src):
//   ode_solver/tableau.rs:161-304         Tableau::tsit45 (first column of `a` computed as there, :221-227)
//   ode_solver/runge_kutta.rs:107-194     Rk::_new;  :232-284 check_explicit_rk;  :436-444 set_stop_time;  :446-464 start_step;  :466-495 factor;
//                            :505-516     start_step_attempt;  :537-566 do_stage;  :752-781 handle_tstop;  :783-800 error_norm;  :843-867 error_test_fail;
//                            :894-960     step_accepted;  :962-1002 beta-polynomial dense output;  :1080-1127 interpolate_inplace;  :1313-1336 pi_controller_raw
//   ode_solver/explicit_rk.rs:46-54, :196-243   ExplicitRk::step;  ode_solver/config.rs:132-160 ExplicitRkConfig
//   ode_solver/method.rs:227-258, :467-520, :881-961   solve / solve_dense;  ode_solver/mod.rs:104-194 the test harness
// with sensitivities:
//   ode_solver/state.rs:1001-1029          RkState::new_with_sensitivities: s_j = SensInit(t0) e_j, ds_j = SensRhs(s_j) about (y0, t0); the step size from the states alone
//   ode_equations/sens_equations.rs:62-70  SensInit;  :119-125 SensRhs::update_state (df/dp at the linearisation point);  :168-174 SensRhs::call_inplace: J x + (df/dp)_j
//   ode_solver/runge_kutta.rs:505-526      start_step_attempt: sdiff_j[:, 0] = h ds_j;  :578-607 do_stage: SensRhs about the stage point, old_state.s_j = s_j + sdiff_j a_row_i;
//                            :812-822      error_norm: sdiff_j d against state.s_j with the sensitivity tolerances, max-chained after the states' norm, j = 0, 1, ..;
//                            :894-930      step_accepted (the swap takes s and ds along);  :1237-1309 interpolate_sens_inplace
// with integrated outputs:
//   ode_solver/state.rs:1097-1109          new_without_initialise: g = 0, dg = out(y0, t0); a model without out integrates its state (identity output)
//   ode_solver/runge_kutta.rs:529-533      start_step_attempt: gdiff[:, 0] = h dg;  :568-575 do_stage: old_state.dg = out(stage point, t + c_i h), gdiff[:, i] = h old_state.dg;
//                            :802-810      error_norm: gdiff d against state.g with out_rtol / out_atol, max-chained after the states' norm (only with output tolerances);
//                            :900-909      step_accepted: old_state.g = state.g + gdiff b, then the swap;  :1185-1235 interpolate_out_inplace;  :396-434 state_mut_back
//   ode_solver/method.rs:830-840, :859-877 solve_dense / solve write g where they write out(y) or y without integrate_out
#include <dlfcn.h>

#include <cstring>
#include <thread>

#include "../../oracle/oracle_ode.hpp"
#include "../../oracle/oracle_sdirk.hpp"

using namespace orc;

// The mode of a solve, as the entry points take it (null: plain).  rtol / atol are the tolerances of the augmented part (sens_rtol / sens_atol, out_rtol / out_atol):
// natol = 0 keeps it out of the error test (turn_off_sensitivities_error_control; no output tolerances), 1: one atol for every component, otherwise one each
// ([n] for the sensitivities — builder.rs build_atols: one vector for every parameter —, [nout] for the outputs).
enum { ERK_PLAIN = 0, ERK_SENS = 1, ERK_INTEGRATE_OUT = 2 };
struct ErkMode {
  int kind;
  double rtol;
  const double* atol;
  int natol;
};

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

// the DiffSL host twin behind a model if it has out_i, else null (identity output); the number of integrated outputs: its out_i count, else its state count
const ExternalModel* out_model(const Model& m) {
  const ExternalModel* e = dynamic_cast<const ExternalModel*>(&m);
  return e && e->nout > 0 ? e : nullptr;
}
int nout_of(const Model& m) { const ExternalModel* e = out_model(m); return e ? e->nout : m.n; }

// is_state_mutated of the reference (Rk::start_step, runge_kutta.rs:446-464, and the first branch of the interpolations) is not restated: only state_mut_back and
// the resets set it, and neither is restated here, so the state is never mutated between steps.
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
  // config.rs:141-160
  double minimum_timestep, maximum_timestep_growth, minimum_timestep_growth, maximum_timestep_shrink, minimum_timestep_shrink;
  int maximum_error_test_failures;
  OdeErr init_error = OdeErr::Ok;
  bool mass_refused = false;
  // with sensitivities (naug = 0: off, and every vector below empty)
  int naug = 0;
  std::vector<V> s, ds, old_s, old_ds;  // state.s / state.ds, old_state.s / old_state.ds
  std::vector<M> sdiff;                 // per parameter n x stages
  V sens_y;                             // the point SensRhs is linearised about
  M sens_mat;                           // df/dp there, n x np
  // with integrated outputs (nout = 0: off)
  int nout = 0;
  bool out_error_control = false;
  double out_rtol = 0.0;
  V out_atol;                          // nout x 1
  V g, dg, old_g, old_dg;              // state.g / state.dg, old_state.g / old_state.dg
  M gdiff;                             // nout x stages
  const ExternalModel* ext = nullptr;  // a DiffSL host twin with out_i; null: identity output

  ExplicitRk(const Problem* p, Tableau t, const ErkMode& mode) : pr(p), tab(std::move(t)) {
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
    if (mode.kind == ERK_SENS) {
      naug = p->eqn->model->np;
      sens_mat = M(n, naug, nb);
      sens_y = V(n, nb);
      // new_with_sensitivities (state.rs:1001-1029).  The step size is set already; set_step_size reads y, dy and the state equations only, so the order of the
      // two does not show in any number (the right-hand-side count is the same)
      s.assign((size_t)naug, V(n, nb));
      ds.assign((size_t)naug, V(n, nb));
      for (int j = 0; j < naug; ++j) p->eqn->init_sens(state.t, j, s[(size_t)j]);
      sens_update_state(state.y, state.t);
      for (int j = 0; j < naug; ++j) sens_rhs_call(j, s[(size_t)j], state.t, ds[(size_t)j]);
      old_s = s;
      old_ds = ds;
      sdiff.assign((size_t)naug, M(n, tab.s, nb));
    }
    if (mode.kind == ERK_INTEGRATE_OUT) {
      ext = out_model(*p->eqn->model);
      nout = nout_of(*p->eqn->model);
      out_error_control = mode.natol > 0;
      out_rtol = mode.rtol;
      out_atol = V(nout, 1);
      for (int k = 0; k < nout; ++k) out_atol.d[(size_t)k] = mode.natol == 0 ? 0.0 : (mode.natol == 1 ? mode.atol[0] : mode.atol[k]);
      g = V(nout, nb);
      dg = V(nout, nb);
      call_out(state.y, state.t, dg);
      old_g = g;
      old_dg = dg;
      gdiff = M(nout, tab.s, nb);
    }
  }

  void sens_update_state(const V& y, double t) {  // SensRhs::update_state
    pr->eqn->rhs_sens(y, t, sens_mat);
    copy_from(sens_y, y);
  }
  void sens_rhs_call(int index, const V& x, double t, V& y) const {  // SensRhs::call_inplace: the Jacobian product first, then the column of df/dp
    pr->eqn->jac_mul(sens_y, t, x, y);
    add_assign(y, sens_mat.column(index));
  }
  void call_out(const V& y, double t, V& o) const {
    if (!ext) { copy_from(o, y); return; }
    for (int b = 0; b < y.nb; ++b) ext->f.out(t, &y.d[(size_t)b * y.n], pr->eqn->pb(b), &o.d[(size_t)b * o.n]);
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

  void start_step_attempt(double h) {  // runge_kutta.rs:505-533: the first stage is h * (dy, dg, ds_j) of the previous step's last stage
    V c0(state.dy.n, state.dy.nb);
    axpy(c0, h, state.dy, 0.0);
    diff.set_column(0, c0);
    for (int j = 0; j < naug; ++j) {  // :517-526
      axpy(c0, h, ds[(size_t)j], 0.0);
      sdiff[(size_t)j].set_column(0, c0);
    }
    if (nout > 0) {  // :529-533
      V cg(nout, state.dy.nb);
      axpy(cg, h, dg, 0.0);
      gdiff.set_column(0, cg);
    }
  }

  void do_stage(int i, double h) {  // runge_kutta.rs:537-607
    const double t = state.t + tab.c[(size_t)i] * h;
    copy_from(old_state.y, state.y);
    gemv_cols(diff, i, 1.0, a_rows[(size_t)i].data(), 1.0, old_state.y);
    pr->eqn->rhs(old_state.y, t, old_state.dy);
    V col(state.y.n, state.y.nb);
    axpy(col, h, old_state.dy, 0.0);
    diff.set_column(i, col);
    if (nout > 0) {  // :568-575: out at the stage point, which the lines above have left in old_state.y
      call_out(old_state.y, t, old_dg);
      V cg(nout, state.dy.nb);
      axpy(cg, h, old_dg, 0.0);
      gdiff.set_column(i, cg);
    }
    if (naug > 0) {  // :578-607: SensRhs about the stage point
      sens_update_state(old_state.y, t);
      for (int j = 0; j < naug; ++j) {
        copy_from(old_s[(size_t)j], s[(size_t)j]);
        gemv_cols(sdiff[(size_t)j], i, 1.0, a_rows[(size_t)i].data(), 1.0, old_s[(size_t)j]);
        sens_rhs_call(j, old_s[(size_t)j], t, old_ds[(size_t)j]);
        axpy(col, h, old_ds[(size_t)j], 0.0);
        sdiff[(size_t)j].set_column(i, col);
      }
    }
  }

  double error_norm() {  // runge_kutta.rs:783-822 with the identity as linear solver: the states, then the outputs or the sensitivities (j ascending), max-chained
    gemv_cols(diff, tab.s, 1.0, tab.d.data(), 0.0, error);
    double norm = std::fmax(0.0, squared_norm(error, state.y, pr->atol, pr->rtol));
    if (nout > 0 && out_error_control) {  // :802-810
      V out_error(nout, g.nb);
      gemv_cols(gdiff, tab.s, 1.0, tab.d.data(), 0.0, out_error);
      norm = std::fmax(norm, squared_norm(out_error, g, out_atol, out_rtol));
    }
    if (pr->sens_error_control)  // :812-822
      for (int j = 0; j < naug; ++j) {
        gemv_cols(sdiff[(size_t)j], tab.s, 1.0, tab.d.data(), 0.0, error);
        norm = std::fmax(norm, squared_norm(error, s[(size_t)j], pr->sens_atol, pr->sens_rtol));
      }
    return norm;
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
    double h = state.h;
    int nattempts = 0;
    double fac = 1.0, norm = 0.0;
    while (true) {
      start_step_attempt(h);
      for (int i = 1; i < tab.s; ++i) do_stage(i, h);
      norm = error_norm();
      fac = factor(norm, 1.0);
      if (norm < 1.0) break;
      h *= fac;
      nattempts += 1;
      prev_error_norm.reset();
      statistics.number_of_error_test_failures += 1;  // error_test_fail (runge_kutta.rs:843-867)
      if (nattempts >= maximum_error_test_failures) return OdeErr::TooManyErrorTestFailures;
      if (std::fabs(h) < minimum_timestep) return OdeErr::StepSizeTooSmall;
    }
    prev_error_norm = norm;
    // step_accepted(h, h * factor, false) (runge_kutta.rs:894-960): g advances (:900-909), and the swap of old_state and state takes g, dg, s and ds along (:910-930)
    if (nout > 0) {
      copy_from(old_g, g);
      gemv_cols(gdiff, tab.s, 1.0, tab.b.data(), 1.0, old_g);
    }
    old_state.t = state.t + h;
    old_state.h = h * fac;
    std::swap(old_state, state);
    std::swap(old_g, g);
    std::swap(old_dg, dg);
    std::swap(old_s, s);
    std::swap(old_ds, ds);
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

  // The dense output's weights at t (runge_kutta.rs:962-981 under the bounds test of :1080-1096, :1185-1200, :1237-1252): beta_f = beta (theta, theta^2, ..); none
  // for a time outside the current step.  A dense value is from + d beta_f.
  std::optional<V> dense_weights(double t) const {
    const bool is_forward = state.h > 0.0;
    if ((is_forward && (t > state.t || t < old_state.t)) || (!is_forward && (t < state.t || t > old_state.t))) return std::nullopt;
    const double dt = state.t - old_state.t;
    const double theta = dt == 0.0 ? 1.0 : (t - old_state.t) / dt;
    const int poly_order = tab.beta.nc;
    std::vector<double> thetav{theta};
    for (int i = 1; i < poly_order; ++i) thetav.push_back(theta * thetav[(size_t)i - 1]);
    V beta_f(tab.beta.nr, 1);
    gemv_cols(tab.beta, poly_order, 1.0, thetav.data(), 0.0, beta_f);
    return beta_f;
  }
  void dense_value(const V& beta_f, const V& from, const M& d, V& ret) const {
    copy_from(ret, from);
    gemv_cols(d, tab.beta.nr, 1.0, beta_f.d.data(), 1.0, ret);
  }
  OdeErr interpolate_inplace(double t, V& ret) const override {  // runge_kutta.rs:1080-1127
    const auto beta_f = dense_weights(t);
    return beta_f ? (dense_value(*beta_f, old_state.y, diff, ret), OdeErr::Ok) : OdeErr::InterpolationTimeOutsideCurrentStep;
  }
  OdeErr interpolate_out_inplace(double t, V& ret) const {  // runge_kutta.rs:1185-1235
    const auto beta_f = dense_weights(t);
    return beta_f ? (dense_value(*beta_f, old_g, gdiff, ret), OdeErr::Ok) : OdeErr::InterpolationTimeOutsideCurrentStep;
  }
  OdeErr interpolate_sens_inplace(double t, std::vector<V>& ret) const {  // runge_kutta.rs:1237-1309
    const auto beta_f = dense_weights(t);
    for (int j = 0; beta_f && j < naug; ++j) dense_value(*beta_f, old_s[(size_t)j], sdiff[(size_t)j], ret[(size_t)j]);
    return beta_f ? OdeErr::Ok : OdeErr::InterpolationTimeOutsideCurrentStep;
  }
  // y, and g and the s_j where the mode has them, at t
  OdeErr interpolate_all(double t, V& y, V& gv, std::vector<V>& sv) const {
    OdeErr e = interpolate_inplace(t, y);
    if (e == OdeErr::Ok && nout > 0) e = interpolate_out_inplace(t, gv);
    if (e == OdeErr::Ok && naug > 0) e = interpolate_sens_inplace(t, sv);
    return e;
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

// what a mode cannot be asked of a model: 0, or the entry points' return value
constexpr int kNoSensitivities = -101, kSensWithRoots = -102;
int mode_refused(int model_id, int model_size, const ErkMode& mode) {
  if (mode.kind != ERK_SENS) return 0;
  auto m = make_model(model_id, model_size);
  if (!m->has_sens) return kNoSensitivities;  // the model has no parameter derivatives
  if (m->nroots > 0) return kSensWithRoots;   // sensitivities with root functions are not restated (the device refuses the combination too)
  return 0;
}

// one problem of `cnt` members (cnt = 1: an independent IVP; cnt > 1: a lock-step batched problem); atol: [n] (natol_rows = 1) or one row per member
std::unique_ptr<Problem> make_problem(int model_id, int model_size, int cnt, const double* p, int np, double rtol, const double* atol, int natol_rows, double t0, double h0,
                                      const ErkMode& mode, const SolveOptions& so) {
  auto pr = std::make_unique<Problem>();
  pr->ode_options = so.ode;
  std::vector<double> pv(p, p + (size_t)np * cnt);
  pr->eqn = std::make_unique<Eqn>(make_model(model_id, model_size), cnt, pv);
  const int n = pr->n();
  pr->rtol = rtol;
  pr->atol = V(n, natol_rows == 1 ? 1 : cnt);
  std::memcpy(pr->atol.d.data(), atol, sizeof(double) * pr->atol.d.size());
  pr->t0 = t0; pr->h0 = h0;
  if (mode.kind == ERK_SENS) {
    pr->sens = true;
    pr->sens_error_control = mode.natol > 0;
    pr->sens_rtol = mode.rtol;
    pr->sens_atol = V(n, 1);
    for (int i = 0; i < n; ++i) pr->sens_atol.d[(size_t)i] = mode.natol == 0 ? 0.0 : (mode.natol == 1 ? mode.atol[0] : mode.atol[i]);
  }
  return pr;
}

// Where the columns of a solve go: y [nsys][width][n] always, g [nsys][width][nout] and s [nsys][width][np][n] where the mode has them (null otherwise), t
// [nsys][width] for the time-stamped columns of the steps.  A column comes as the vectors of one problem of cnt members, which are members s0 .. s0 + cnt - 1.
struct ColumnSink {
  double *y, *g, *s, *t;
  int n, nout, np, width;
  void put(int s0, int cnt, int c, const V& yv, const V& gv, const std::vector<V>& sv) const {
    for (int b = 0; b < cnt; ++b) {
      const size_t at = (size_t)(s0 + b) * width + c;
      std::memcpy(y + at * n, yv.d.data() + (size_t)b * n, sizeof(double) * n);
      if (g) std::memcpy(g + at * nout, gv.d.data() + (size_t)b * nout, sizeof(double) * nout);
      if (s) for (int j = 0; j < np; ++j) std::memcpy(s + (at * np + j) * n, sv[(size_t)j].d.data() + (size_t)b * n, sizeof(double) * n);
    }
  }
  void put_step(int s0, int cnt, int c, double tw, const V& yv, const V& gv, const std::vector<V>& sv) const {
    put(s0, cnt, c, yv, gv, sv);
    for (int b = 0; b < cnt; ++b) t[(size_t)(s0 + b) * width + c] = tw;
  }
  void nan_fill(int m, int from) const {  // the columns a member never reached
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t at = (size_t)m * width + from; at < (size_t)(m + 1) * width; ++at) {
      std::fill_n(y + at * n, n, nan);
      if (g) std::fill_n(g + at * nout, nout, nan);
      if (s) std::fill_n(s + at * np * n, (size_t)np * n, nan);
    }
  }
};

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

// number of integrated outputs of a model: its out_i count, its state count without out_i
int erk_model_nout(int model_id, int model_size) { return nout_of(*make_model(model_id, model_size)); }

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

// The reference's test harness (ode_solver/mod.rs:104-194) on one IVP: for each point, use_tstop ? set_stop_time(t) + step to TstopReached, the state
// : step while t < t_point, the dense output at t_point (interpolate / interpolate_out / interpolate_sens).  mode: null for plain.  y_out [npoints][n], g_out
// [npoints][nout] (integrated outputs only, else null), s_out [npoints][np][n] (sensitivities only, else null); counters[4] = steps, error-test failures, right-hand
// sides, Jacobian products.  Returns 0, -OdeErr, -100 for a mass matrix (MassMatrixNotSupported), -101 for sensitivities of a model without parameter derivatives,
// -102 for sensitivities of a model with root functions.
int erk_solve_to_points(int model_id, int model_size, const double* p, int np, double rtol, const double* atol, double t0, double h0, const ErkMode* mode_or_null,
                        const double* t_points, int npoints, int use_tstop, double* y_out, double* g_out, double* s_out, long* counters) {
  const ErkMode mode = mode_or_null ? *mode_or_null : ErkMode{ERK_PLAIN, 0.0, nullptr, 0};
  if (int rc = mode_refused(model_id, model_size, mode)) return rc;
  auto pr = make_problem(model_id, model_size, 1, p, np, rtol, atol, 1, t0, h0, mode, SolveOptions(nullptr));
  ExplicitRk sv(pr.get(), tsit45(), mode);
  if (sv.mass_refused) return -100;
  if (sv.init_error != OdeErr::Ok) return -(int)sv.init_error;
  const int n = pr->n();
  const ColumnSink sink{y_out, sv.nout > 0 ? g_out : nullptr, sv.naug > 0 ? s_out : nullptr, nullptr, n, sv.nout, np, npoints};
  V tmp(n, 1), gtmp(sv.nout, 1);
  std::vector<V> stmp((size_t)sv.naug, V(n, 1));
  for (int k = 0; k < npoints; ++k) {
    if (use_tstop) {
      OdeErr e = sv.set_stop_time(t_points[k]);
      if (e != OdeErr::Ok && e != OdeErr::StopTimeAtCurrentTime) return -(int)e;
      while (e == OdeErr::Ok) {
        StopReason r;
        e = sv.step(r);
        if (e != OdeErr::Ok) return -(int)e;
        if (r == StopReason::TstopReached) break;
      }
      sink.put(0, 1, k, sv.y(), sv.g, sv.s);
    } else {
      while (std::fabs(sv.t()) < std::fabs(t_points[k])) {
        StopReason r;
        OdeErr e = sv.step(r);
        if (e != OdeErr::Ok) return -(int)e;
      }
      OdeErr e = sv.interpolate_all(t_points[k], tmp, gtmp, stmp);
      if (e != OdeErr::Ok) return -(int)e;
      sink.put(0, 1, k, tmp, gtmp, stmp);
    }
  }
  if (counters) {
    counters[0] = sv.stats().number_of_steps; counters[1] = sv.stats().number_of_error_test_failures;
    counters[2] = pr->eqn->rhs_stats.calls; counters[3] = pr->eqn->rhs_stats.jac_muls;
  }
  return 0;
}

// solve_dense (method.rs:467-520) / solve (:227-258, :881-961) / solve_dense_sensitivities for an ensemble: group = 1 every member its own IVP, group = G
// consecutive groups of G members as one lock-step batched problem each (the norms of the augmented part are max-reduced over the group like the states').
// mode: null for plain.  steps_cap = 0: columns at t_eval, width nt; steps_cap > 0: t_eval[0] is the final time, every accepted step a column, width steps_cap,
// t_out [nsys][steps_cap] (columns beyond the cap are counted, not stored).  y_out [nsys][width][n] the states; g_out [nsys][width][nout] the integrated outputs
// in the same columns (written only with integrated outputs: at a root g interpolated at the root, the column before the first step zero); s_out
// [nsys][width][np][n] (written only with sensitivities).  Columns never reached: NaN (steps_cap = 0; the caller's fill otherwise).  atol [n] (natol_rows = 1) or
// [nsys][n].  Per member, each nullable: stats_out [nsys][5] (steps, 0, 0, error-test failures, 0), status_out, root_t_out (NaN: none), root_idx_out, ncols_out
// [nsys], calls_out [nsys][2] (right-hand sides, Jacobian products of the member's problem).  options: null, or the kNumSolveOptions doubles of SolveOptions
// (max_error_test_failures, min_timestep, pi_control_integral, pi_control_proportional, max_steps).  Returns the number of failed members, or -101 / -102 as
// erk_solve_to_points.
int erk_solve_ensemble(int model_id, int model_size, int nsys, const double* p, int np, double rtol, const double* atol, int natol_rows, double t0, double h0,
                       const ErkMode* mode_or_null, const double* t_eval, int nt, int nthreads, int group, int steps_cap, double* y_out, double* g_out, double* s_out,
                       double* t_out, long* stats_out, int* status_out, double* root_t_out, int* root_idx_out, int* ncols_out, long* calls_out, const double* options) {
  const ErkMode mode = mode_or_null ? *mode_or_null : ErkMode{ERK_PLAIN, 0.0, nullptr, 0};
  if (int rc = mode_refused(model_id, model_size, mode)) return rc;
  const SolveOptions so(options);
  if (group < 1) group = 1;
  if (nthreads < 1) nthreads = 1;
  const int ngroups = (nsys + group - 1) / group;
  const auto model = make_model(model_id, model_size);
  const int n = model->n;
  const ColumnSink sink{y_out, mode.kind == ERK_INTEGRATE_OUT ? g_out : nullptr, mode.kind == ERK_SENS ? s_out : nullptr, t_out, n, nout_of(*model), np,
                        steps_cap > 0 ? steps_cap : nt};
  std::vector<int> failed_per_thread((size_t)nthreads, 0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto work = [&](int tid) {
    for (int gi = tid; gi < ngroups; gi += nthreads) {
      const int s0 = gi * group, cnt = std::min(group, nsys - s0);
      auto pr = make_problem(model_id, model_size, cnt, p + (size_t)s0 * np, np, rtol, natol_rows == 1 ? atol : atol + (size_t)s0 * n, natol_rows, t0, h0, mode, so);
      ExplicitRk sv(pr.get(), tsit45(), mode);
      int col = 0;
      OdeErr err = sv.mass_refused ? OdeErr::InterpolationTimeOutsideCurrentStep : sv.init_error;
      V tmp(n, cnt), gtmp(sv.nout, cnt);
      std::vector<V> stmp((size_t)sv.naug, V(n, cnt));
      auto steps_write = [&](double tw, const V& yv, const V& gv, const std::vector<V>& s_v) {
        if (col < steps_cap) sink.put_step(s0, cnt, col, tw, yv, gv, s_v);
        col++;
      };
      bool rooted = false;
      if (err == OdeErr::Ok) {
        if (steps_cap > 0) steps_write(sv.t(), sv.y(), sv.g, sv.s);
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
        if (steps_cap > 0) { if (r != StopReason::RootFound) steps_write(sv.t(), sv.y(), sv.g, sv.s); }
        else
          while (col < nt && t_eval[col] <= upto) { (void)sv.interpolate_all(t_eval[col], tmp, gtmp, stmp); sink.put(s0, cnt, col, tmp, gtmp, stmp); col++; }
        if (r == StopReason::TstopReached) break;
        if (r == StopReason::RootFound) {  // state_mut_back(root, integrate_out): the column after the drained ones holds y (and g) at the root
          (void)sv.interpolate_all(sv.root_time, tmp, gtmp, stmp);
          if (steps_cap > 0) steps_write(sv.root_time, tmp, gtmp, stmp);
          else if (col < nt) { sink.put(s0, cnt, col, tmp, gtmp, stmp); col++; }
          rooted = true;
          break;
        }
      }
      for (int b = 0; b < cnt; ++b) {
        const int m = s0 + b;
        if (ncols_out) ncols_out[m] = col;
        if (steps_cap == 0) sink.nan_fill(m, col);
        if (status_out) status_out[m] = capped ? kStatusMaxStepsExceeded : status_of(err);
        if (root_t_out) root_t_out[m] = rooted ? sv.root_time : nan;
        if (root_idx_out) root_idx_out[m] = rooted ? sv.root_index : -1;
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
