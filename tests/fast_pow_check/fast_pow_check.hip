// TEST INFRASTRUCTURE ONLY (tests/test_gpu_fast_pow.py): the fixed-exponent powers of the fast BDF build's Newton chain (pow_p08, root_k in
// diffsol_amd/csrc/dsh_adaptive_kernel.hpp) beside the plain pow call they replace, on caller-supplied arguments, one argument per lane in blocks of one wavefront;
// and the same powers by powl in long double on the host.  Compiled with the FASTFLAGS of csrc/Makefile, like the kernel that uses the helpers.
#include <cmath>

#include "../../diffsol_amd/csrc/dsh_internal.hpp"
#include "../../diffsol_amd/csrc/dsh_resident.hpp"
#include "../../diffsol_amd/csrc/dsh_adaptive_kernel.hpp"

// k[i] == 0: pow_p08(x[i]) beside pow(x[i], 0.8); k[i] > 0: root_k(x[i], k[i]) beside pow(x[i], 1.0 / k[i]) (the exponent as the kernel's call site writes it)
__global__ __launch_bounds__(64) void k_fast_pow_both(const double* __restrict__ x, const int* __restrict__ k, int n, double* __restrict__ out_new, double* __restrict__ out_pow) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double xi = x[i];
  const int ki = k[i];
  if (ki == 0) {
    out_new[i] = dsh::pow_p08(xi);
    out_pow[i] = pow(xi, 0.8);
  } else {
    out_new[i] = dsh::root_k(xi, ki);
    out_pow[i] = pow(xi, 1.0 / (double)ki);
  }
}

// x, k: n arguments (host); out_new / out_pow: n results each (host).  Returns 0, or the HIP error code.
extern "C" int fast_pow_both(const double* x, const int* k, int n, double* out_new, double* out_pow) {
  if (n <= 0) return 0;
  double *d_x = nullptr, *d_out = nullptr;
  int* d_k = nullptr;
  hipError_t e = hipMalloc(&d_x, sizeof(double) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&d_k, sizeof(int) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(double) * 2 * (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(d_x, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_k, k, sizeof(int) * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_fast_pow_both, dim3((n + 63) / 64), dim3(64), 0, 0, d_x, d_k, n, d_out, d_out + n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_new, d_out, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_pow, d_out + n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost);
  (void)hipFree(d_x);
  (void)hipFree(d_k);
  (void)hipFree(d_out);
  return (int)e;
}

// |got - x^(num/den)| / x^(num/den) in units of 2^-53, the power by powl in the host's 80-bit long double with the exponent formed in long double
// (4/5 for pow_p08, 1/k for root_k: the mathematical power the helper is named after, not the power to the double nearest the exponent)
extern "C" void fast_pow_err_ulp(const double* x, const double* got, int n, int num, int den, double* err) {
  const long double y = (long double)num / (long double)den;
  for (int i = 0; i < n; ++i) {
    const long double ref = powl((long double)x[i], y);
    err[i] = (double)(fabsl((long double)got[i] - ref) / ref * 0x1p53L);
  }
}
