// The one instantiation bench.py times, alone in a translation unit (tests/test_pivot_facts.py compiles it with the flags of dsh_adaptive_fast.hip and reads the
// compiler's resource remarks and the spill reloads of its listing): seconds, against minutes for the whole of dsh_adaptive_fast.hip.
#include "dsh_internal.hpp"
#include "dsh_resident.hpp"
#include "dsh_adaptive_kernel.hpp"
#include "dsh_models.hpp"

namespace dsh {
template __global__ void k_bdf_adaptive<RobertsonOde1, true, true, false, false, true, true>(int64_t, const double*, const double*, const AdaptiveConsts*, const double*,
                                                                                               double*, int32_t*, int32_t*, double*, int32_t*, int32_t*,
                                                                                               unsigned long long*);
}  // namespace dsh
