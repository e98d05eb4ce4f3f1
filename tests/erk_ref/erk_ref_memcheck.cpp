// CHECKER — TEST INFRASTRUCTURE ONLY.  Stand-alone memory check of the ensemble driver's buffer arithmetic (ColumnSink, the per-member writes) in erk_ref.cpp: one
// erk_solve_ensemble call per mode with five members in lock-step groups of three (the last group ragged) on two threads, into buffers of exactly the documented
// sizes, plus a steps run whose cap is smaller than the step count (columns counted, not stored).  Build and run on the CPU as an ordinary executable:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -o erk_ref_memcheck erk_ref_memcheck.cpp -ldl && ./erk_ref_memcheck
// (this file includes erk_ref.cpp, so the two are one program and the prototypes cannot drift).  Exit status 0 and "ok" when every call returned what it should.
#include <cstdio>

#include "erk_ref.cpp"

namespace {

constexpr int kNsys = 5, kGroup = 3, kThreads = 2, kN = 2, kNp = 2;
const double kP[kNsys * kNp] = {0.1, 1.0, 1.0, 2.0, 2.0, 0.5, 0.5, 1.5, 0.25, 3.0};  // exponential decay: (k, y0) per member
const double kAtolRows[kNsys * kN] = {1e-6, 1e-6, 1e-7, 1e-7, 1e-5, 1e-5, 3e-6, 3e-6, 3e-7, 3e-7};
const double kAtol[kN] = {1e-6, 1e-6};
const double kTEval[4] = {0.5, 1.0, 2.5, 6.0};

struct Result {
  std::vector<double> y, g, s, t, root_t;
  std::vector<long> stats, calls;
  std::vector<int> status, root_idx, ncols;
  int failed = 0;
};

// width columns per member; buffers of the mode's arrays only, the others null
Result solve(int model, const ErkMode* mode, const double* atol, int natol_rows, const double* t_eval, int nt, int steps_cap, const double* options) {
  const int width = steps_cap > 0 ? steps_cap : nt, nout = erk_model_nout(model, 0);
  Result r;
  r.y.assign((size_t)kNsys * width * kN, 0.0);
  if (mode && mode->kind == ERK_INTEGRATE_OUT) r.g.assign((size_t)kNsys * width * nout, 0.0);
  if (mode && mode->kind == ERK_SENS) r.s.assign((size_t)kNsys * width * kNp * kN, 0.0);
  if (steps_cap > 0) r.t.assign((size_t)kNsys * steps_cap, 0.0);
  r.stats.assign((size_t)kNsys * 5, 0);
  r.calls.assign((size_t)kNsys * 2, 0);
  r.status.assign(kNsys, 0); r.root_idx.assign(kNsys, 0); r.ncols.assign(kNsys, 0);
  r.root_t.assign(kNsys, 0.0);
  r.failed = erk_solve_ensemble(model, 0, kNsys, kP, kNp, 1e-6, atol, natol_rows, 0.0, 1.0, mode, t_eval, nt, kThreads, kGroup, steps_cap, r.y.data(),
                                r.g.empty() ? nullptr : r.g.data(), r.s.empty() ? nullptr : r.s.data(), r.t.empty() ? nullptr : r.t.data(), r.stats.data(), r.status.data(),
                                r.root_t.data(), r.root_idx.data(), r.ncols.data(), r.calls.data(), options);
  return r;
}

int fail(const char* what) { std::printf("FAILED: %s\n", what); return 1; }

}  // namespace

int main() {
  erk_set_det_pow(1);
  const double t_final[1] = {6.0};
  // plain, every accepted step with a cap of 4 columns: every group takes more steps, so columns are counted beyond the stored ones
  const Result steps = solve(MODEL_EXPONENTIAL_DECAY, nullptr, kAtolRows, kNsys, t_final, 1, 4, nullptr);
  if (steps.failed != 0) return fail("plain steps run");
  for (int m = 0; m < kNsys; ++m) if (steps.ncols[(size_t)m] <= 4 || steps.ncols[(size_t)m] != steps.stats[(size_t)m * 5] + 1) return fail("columns beyond the cap are counted");
  // plain on the model with a root, save points, cut by max_steps: the root column, the NaN fill and the capped members
  const double cut[kNumSolveOptions] = {40, 1e-13, 0.5, 0.0, 6};
  const Result root = solve(MODEL_EXPONENTIAL_DECAY_ROOT, nullptr, kAtol, 1, kTEval, 4, 0, cut);
  if (root.failed <= 0 || root.failed > kNsys) return fail("plain run cut by max_steps");
  for (int m = 0; m < kNsys; ++m) if (root.ncols[(size_t)m] < 4 && !std::isnan(root.y[((size_t)m * 4 + 3) * kN])) return fail("NaN behind the last column");
  // sensitivities at the save points, one sens_atol per state
  const double sens_atol[kN] = {1e-6, 1e-7};
  const ErkMode sens{ERK_SENS, 1e-6, sens_atol, kN};
  const Result s = solve(MODEL_EXPONENTIAL_DECAY, &sens, kAtol, 1, kTEval, 4, 0, nullptr);
  if (s.failed != 0 || std::isnan(s.s.back())) return fail("sensitivities");
  if (solve(MODEL_EXPONENTIAL_DECAY_ROOT, &sens, kAtol, 1, kTEval, 4, 0, nullptr).failed != kSensWithRoots) return fail("sensitivities with root functions are refused");
  // integrated outputs, one out_atol per output, at the save points and in steps beyond a cap of 4 columns
  const double out_atol[kN] = {1e-10, 1e-9};
  const ErkMode out{ERK_INTEGRATE_OUT, 1e-8, out_atol, kN};
  const Result g = solve(MODEL_EXPONENTIAL_DECAY_ROOT, &out, kAtolRows, kNsys, kTEval, 4, 0, nullptr);
  if (g.failed < 0) return fail("integrated outputs");
  const Result gs = solve(MODEL_EXPONENTIAL_DECAY, &out, kAtol, 1, t_final, 1, 4, nullptr);
  if (gs.failed != 0 || gs.g[0] != 0.0 || gs.t[0] != 0.0) return fail("integrated outputs in steps");
  std::printf("ok\n");
  return 0;
}
