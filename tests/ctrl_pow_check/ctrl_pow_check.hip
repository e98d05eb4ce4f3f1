// TEST INFRASTRUCTURE ONLY (tests/test_gpu_default_options.py): the step-size controller's power of the fast BDF build's lock-step groups with the default controller
// constants (inv_root_2k_group in diffsol_amd/csrc/dsh_adaptive_kernel.hpp) beside the pow call it replaces, on caller-supplied (x, k), one pair per lane in blocks of
// one wavefront: like the kernel, a wavefront with an argument outside the helper's domain makes the pow call in every lane.  Compiled with the FASTFLAGS of csrc/Makefile.
#include "../../diffsol_amd/csrc/dsh_internal.hpp"
#include "../../diffsol_amd/csrc/dsh_resident.hpp"
#include "../../diffsol_amd/csrc/dsh_adaptive_kernel.hpp"

// n is a multiple of 64 (the host pads): every lane of every wavefront reaches the ballot inside inv_root_2k_group
__global__ __launch_bounds__(64) void k_ctrl_pow_both(const double* __restrict__ x, const int* __restrict__ k, double* __restrict__ out_new, double* __restrict__ out_pow) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const double xi = x[i];
  const int ki = k[i];
  const double expo = -(0.5 / (double)ki);  // the exponent as the controller writes it: -(pi_control_integral / (double)(order + which))
  out_new[i] = dsh::inv_root_2k_group(xi, ki, expo);
  out_pow[i] = pow(xi, expo);
}

// x, k: n pairs (host), n a multiple of 64; out_new / out_pow: n results each (host).  Returns 0, the HIP error code, or -1 for a bad n.
extern "C" int ctrl_pow_both(const double* x, const int* k, int n, double* out_new, double* out_pow) {
  if (n == 0) return 0;
  if (n < 0 || n % 64 != 0) return -1;
  double *d_x = nullptr, *d_out = nullptr;
  int* d_k = nullptr;
  hipError_t e = hipMalloc(&d_x, sizeof(double) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&d_k, sizeof(int) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(double) * 2 * (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(d_x, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_k, k, sizeof(int) * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_ctrl_pow_both, dim3(n / 64), dim3(64), 0, 0, d_x, d_k, d_out, d_out + n);
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
