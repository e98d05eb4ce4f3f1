// problem.tsit45() on the host side.  The explicit Runge-Kutta method (crates/diffsol/src/ode_solver/explicit_rk.rs) runs device-resident only
// (dsh_erk_solve_resident: the whole ensemble solve in one launch); a host-driven lock-step ExplicitRk over the trait operations is not provided.  This handle
// carries what the constructor of the reference's solver establishes — the checks of Rk::check_explicit_rk (runge_kutta.rs:232-284) and the initial state
// RkState::new_and_consistent(problem, 4) — and refuses to step.  With forward sensitivities (problem.tsit45_sens()) the same holds: dsh_erk_solve_resident_sens
// integrates them inside the launch, for the models of dsh_erk_model_has_sens (make_solver() refuses the others).
#pragma once
#include "ode.hpp"

namespace diffsol_hip {

constexpr const char* kTsit45HostDriven =
    "Tsit45 is integrated device-resident only: use dshs_solve_dense (ensemble mode auto, per member or wavefront), dshs_solve_dense_adaptive or dshs_solve_adaptive; "
    "the host-driven lock-step path (dshs_step, dshs_solve, dshs_solve_to_points, DSHS_ENSEMBLE_LOCKSTEP) has no explicit Runge-Kutta method — use BDF, TR-BDF2 or ESDIRK34 there";

// problem.tsit45_sens(): why dshs_create_sens refuses a model the plain Tsit45 takes (dsh_erk_model_has_sens: the register-resident kernel with sensitivities keeps
// nstates * (14 + 12 * nparams) doubles per member and admits 112)
inline std::string tsit45_sens_refusal(const OdeEquations& eqn) {
  const int64_t n = eqn.nstates(), np = eqn.nparams(), nr = eqn.nroots();
  return "Tsit45 integrates forward sensitivities device-resident in registers only — models with parameter derivatives, without stop conditions (root functions), whose "
         "states and parameters satisfy nstates * (14 + 12 * nparams) <= 112 (2 states with up to 3 parameters, 4 states with 1, 1 state with up to 8); this model has " +
         std::to_string(n) + " states, " + std::to_string(np) + " parameters (" + std::to_string(n * (14 + 12 * np)) + ") and " + std::to_string(nr) +
         " root functions: use BDF, TR-BDF2 or ESDIRK34 for its sensitivities (dshs_create_sens with one of them)";
}

class ExplicitRkDeviceOnly : public OdeSolverMethod {
 public:
  explicit ExplicitRkDeviceOnly(const OdeSolverProblem& problem) : pr_(problem) {
    if (problem.eqn->has_mass())
      throw LaError(DSH_E_UNSUPPORTED, "MassMatrixNotSupported: Tsit45 is an explicit Runge-Kutta method and takes no mass matrix; use BDF, TR-BDF2 or ESDIRK34 for this model");
    state_ = new_and_consistent(problem, 4);
  }
  [[noreturn]] static void refuse() { throw LaError(DSH_E_UNSUPPORTED, kTsit45HostDriven); }
  OdeSolverStopReason step() override { refuse(); }
  void set_stop_time(double) override { refuse(); }
  void interpolate_inplace(double, HipVec&) const override { refuse(); }
  const HipVec& y() const override { return state_.y; }
  const HipVec& dy() const override { return state_.dy; }
  double t() const override { return state_.t; }
  double h() const override { return state_.h; }
  int order() const override { return 4; }
  const OdeSolverStatistics& get_statistics() const override { return stats_; }
  const OdeSolverProblem& problem() const override { return pr_; }
  void state_mut_back(double) override { refuse(); }
  void apply_reset() override { refuse(); }

 private:
  const OdeSolverProblem& pr_;
  StateCommon state_;
  OdeSolverStatistics stats_;
};

}  // namespace diffsol_hip
