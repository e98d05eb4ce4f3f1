// The FAST arithmetic variant of the device-resident BDF (k_bdf_adaptive<.., FAST = true>; dsh_adaptive_options::deterministic_pow == 2): the library's
// default arithmetic for Solver.solve_dense (dshs_set_resident_arithmetic / DSH_RESIDENT_ARITH), hence the kernel bench.py times.
//
// This translation unit alone is compiled with -ffp-contract=fast -freciprocal-math -fapprox-func (csrc/Makefile): the same kernel source as the exact
// variant, with multiply-adds fused, divisions by reciprocal + refinement instead of the IEEE sequence, ocml's pow, and the Newton norm's weights as
// reciprocals.  The two powers on the Newton chain have a fixed exponent and skip the general pow (pow_p08, root_k in dsh_adaptive_kernel.hpp): eta^0.8 as
// eta * eta^(-1/5) from a single-precision seed and three division-free Newton steps, the convergence rate's square and cube root by sqrt and cbrt; both within
// a few ulp of the mathematical power, both feeding decisions only, and any argument outside their domain (zero, denormal, negative, infinite, NaN) takes the
// pow call.  In lock-step groups with the default controller constants the order selection's three values x^(-1/(2k)) come from inv_root_2k_group (a single-precision
// seed, two division-free Newton steps; at most 2.1 units of 2^-53 off, the derived bound; they feed the step size); per-member control, the error-test failure's pi_controller_raw and the initial
// step size keep the general pow.
//
// Lock-step groups whose options are the defaults take k_bdf_adaptive<.., FAST, DEFOPT = true>: the options the kernel body reads are compile-time constants there
// (DSH_ADAPTIVE_BODY_OPTIONS, dsh_adaptive_kernel.hpp: the one list behind dsh_adaptive_default_options(), the kernel's constant view and body_options_are_default
// below), so that no option is loaded on the per-step chain.  Bit for bit the general fast kernel's results (profiles/default_options_kernel.md).  This is the instantiation bench.py times.
// It also takes the first Newton iteration's convergence test by ballot: every lane compares its own weighted mean square with a threshold formed ahead of the solve
// (ballot_decide_below, dsh_adaptive_kernel.hpp), so a step that converges in one iteration runs no wavefront reduction, and one that does not reduces that norm in
// the second iteration's block, where its value is first read (behind that iteration's substitution, as the compiler schedules it).  The first two iterations are
// peeled for that; eta^0.8 and the threshold are formed in the first solve's block.  Same values, same decisions: still the general fast kernel's bits (profiles/ballot_decisions.md, tests/test_gpu_ballot_decisions.py).
// Its prediction, its update of the differences and the norms of its order selection have a body per order behind one scalar dispatch on the wavefront-uniform order
// (with_order, dsh_adaptive_kernel.hpp) with that order's Bdf::_new coefficients as constants (dsh_bdf_tables.hpp): the same operations per component, the same bits
// (profiles/order_paths.md, tests/test_gpu_order_paths.py).
// Its wavefront maxima (the Newton norms from the second iteration on, the error norm, the order selection's norms) run a stage written as the instructions it needs:
// two v_mov_b32_dpp and one v_max_f64 (dpp_max_f64_raw, dsh_adaptive_kernel.hpp).  The general stage is __builtin_fmax on a value put together from DPP moves, and in
// IEEE mode the compiler puts a quieting v_max_f64 x, x, x in front of every such maximum: an instruction that is issued, sits on the reduction's serial chain and is
// the identity on what these call sites reduce.  The stage is exact under their conditions: the values are weighted mean squares (never negative), a ballot ahead of
// the chain has excluded a NaN (a wavefront that holds one takes the two-pass bit-pattern maximum, unchanged), and all 64 lanes are active.  IEEE mode stays on, so
// every other fmax / fmin keeps its instructions.  Same values: still the general fast kernel's bits (profiles/wave_max_raw.md, tests/test_gpu_wave_max_raw.py).
// Its step loop reloads nothing from scratch (DSH_STEP_NO_RELOAD, dsh_adaptive_kernel.hpp): the next save point is a wavefront-uniform value that is NaN behind
// the last column, so the save-point test of a step is one comparison on a value in scalar registers, with no scratch reload and no load of n_eval per step, and the
// lane-dependent invariants the compiler formed ahead of the loop and spilled (the lane's role in the order selection's shared pow, the R column of the Newton
// failure's constant factor) are formed where they are read.  Scratch falls from 80 to 32 B in the instantiation bench.py times; the three reloads left are on the
// path that writes a column and behind the loop.  Same values: still the general fast kernel's bits (profiles/pivot_facts.md, tests/test_gpu_pivot_facts.py,
// tests/test_pivot_facts.py).  That document also records the pivot facts that were built, measured slower and left out.
//
// Its results are NOT bit-comparable with the oracle (every other kernel of the library is); north_star asks for 1e-6 relative on the states,
// which the tests hold it to at tight tolerances; at the bench's full size it makes the step decisions of the exact kernel (every member's five counters equal,
// states within 1e-9: tests/test_gpu_adaptive.py).  The bitwise test tier pins the exact kernel (tests/conftest.py).
#include <cstring>

#include "dsh_internal.hpp"
#include "dsh_resident.hpp"
#include "dsh_adaptive_kernel.hpp"

namespace dsh {

// Does every option the kernel body reads (DSH_ADAPTIVE_BODY_OPTIONS) hold its default, bit for bit?  -0.0 for 0.0 is not the default.
static bool body_options_are_default(const dsh_adaptive_options& o) {
  bool same = true;
#define DSH_X(T, name, value) { const T dflt = value; same = same && std::memcmp(&o.name, &dflt, sizeof(T)) == 0; }
  DSH_ADAPTIVE_BODY_OPTIONS(DSH_X)
#undef DSH_X
  return same;
}

// opts: the options as the launch's AdaptiveConsts hold them (host copy).  Lock-step groups whose body options are all defaults take the default-options
// instantiation; every other call the general fast kernel, which reads them from *consts.
bool adaptive_fast_launch(int model, int64_t size, bool ba, bool wave, const dsh_adaptive_options& opts, dim3 grid, hipStream_t stream, int64_t nb, const double* p,
                          const double* atol, const AdaptiveConsts* consts, const double* t_eval, double* y_out, int32_t* stats, int32_t* status, double* t_root,
                          int32_t* root_idx, int32_t* ncols, unsigned long long* totals) {
  const dim3 blk(64);
  bool launched = false;
  const bool defopt = wave && opts.group == 64 && body_options_are_default(opts);
  dispatch_static_model(model, size, [&](auto mdl) {
    using Mdl = decltype(mdl);
    if constexpr (Mdl::N <= 4) {
#define DSH_FAST_LAUNCH(BA, WAVE) \
  hipLaunchKernelGGL((k_bdf_adaptive<Mdl, BA, WAVE, false, false, true>), grid, blk, 0, stream, nb, p, atol, consts, t_eval, y_out, stats, status, t_root, root_idx, ncols, totals)
#define DSH_FAST_DEFOPT_LAUNCH(BA) \
  hipLaunchKernelGGL((k_bdf_adaptive<Mdl, BA, true, false, false, true, true>), grid, blk, 0, stream, nb, p, atol, consts, t_eval, y_out, stats, status, t_root, root_idx, ncols, totals)
      if (defopt) { if (ba) DSH_FAST_DEFOPT_LAUNCH(true); else DSH_FAST_DEFOPT_LAUNCH(false); }
      else if (wave) { if (ba) DSH_FAST_LAUNCH(true, true); else DSH_FAST_LAUNCH(false, true); }
      else { if (ba) DSH_FAST_LAUNCH(true, false); else DSH_FAST_LAUNCH(false, false); }
#undef DSH_FAST_DEFOPT_LAUNCH
#undef DSH_FAST_LAUNCH
      launched = true;
    }
  });
  return launched;
}

}  // namespace dsh
