// TEST INFRASTRUCTURE ONLY (tests/test_gpu_ballot_decisions.py): the group decision the default-options fast lock-step BDF kernel takes by ballot
// (newton_first_converged in diffsol_amd/csrc/dsh_adaptive_kernel.hpp) beside the reduction-based test it replaces, on caller-supplied values, one wavefront
// per block.  Compiled with the FASTFLAGS of csrc/Makefile, so that sqrt and the division are the fast build's.
#include "../../diffsol_amd/csrc/dsh_internal.hpp"
#include "../../diffsol_amd/csrc/dsh_resident.hpp"
#include "../../diffsol_amd/csrc/dsh_adaptive_kernel.hpp"

// m: 64 weighted mean squares per wavefront; eta08, tol: one value per wavefront.  out[3 w + 0] = the new decision, [3 w + 1] = eta08 * sqrt(wave max) < tol,
// [3 w + 2] = 1 if the new decision came from the undecided path (the reduction).
__global__ __launch_bounds__(64) void k_newton_first(const double* __restrict__ m, const double* __restrict__ eta08, const double* __restrict__ tol, int* __restrict__ out) {
  const int w = blockIdx.x;
  const double mi = m[w * 64 + threadIdx.x];
  const double e08 = dsh::uniform<true>(eta08[w]), tl = dsh::uniform<true>(tol[w]);
  bool undecided = false;
  const bool conv_new = dsh::newton_first_converged(mi, dsh::newton_first_threshold(tl, e08), e08, tl, undecided);
  const bool conv_old = e08 * sqrt(dsh::wave_max_nonneg_f64(mi)) < tl;
  if (threadIdx.x == 0) { out[3 * w + 0] = conv_new ? 1 : 0; out[3 * w + 1] = conv_old ? 1 : 0; out[3 * w + 2] = undecided ? 1 : 0; }
}

// m [64 nw], eta08 [nw], tol [nw] (host); out: 3 nw ints (host).  Returns 0, the HIP error code, or -1 for a bad nw.
extern "C" int newton_first_both(const double* m, const double* eta08, const double* tol, int nw, int* out) {
  if (nw == 0) return 0;
  if (nw < 0) return -1;
  const size_t n = (size_t)nw;
  double *d_v = nullptr, *d_a = nullptr, *d_b = nullptr;
  int* d_out = nullptr;
  hipError_t e = hipMalloc(&d_v, sizeof(double) * 64 * n);
  if (e == hipSuccess) e = hipMalloc(&d_a, sizeof(double) * n);
  if (e == hipSuccess) e = hipMalloc(&d_b, sizeof(double) * n);
  if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(int) * 3 * n);
  if (e == hipSuccess) e = hipMemcpy(d_v, m, sizeof(double) * 64 * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_a, eta08, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_b, tol, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_newton_first, dim3(nw), dim3(64), 0, 0, d_v, d_a, d_b, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(int) * 3 * n, hipMemcpyDeviceToHost);
  (void)hipFree(d_v);
  (void)hipFree(d_a);
  (void)hipFree(d_b);
  (void)hipFree(d_out);
  return (int)e;
}
