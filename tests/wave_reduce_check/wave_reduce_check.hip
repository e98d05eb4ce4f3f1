// TEST INFRASTRUCTURE ONLY (tests/test_gpu_wave_uniform.py): the two wavefront maxima of diffsol_amd/csrc/dsh_device.hpp side by side on caller-supplied
// 64-lane patterns — one wavefront per pattern; wave_max_nonneg_f64 must return the bits of wave_max_u64 on every non-negative double and on NaN.
#include "../../diffsol_amd/csrc/dsh_device.hpp"

__global__ __launch_bounds__(64) void k_wave_max_both(const double* __restrict__ in, unsigned long long* __restrict__ out_f64, unsigned long long* __restrict__ out_u64) {
  const double v = in[(size_t)blockIdx.x * 64 + threadIdx.x];
  const unsigned long long a = dsh::d2u(dsh::wave_max_nonneg_f64(v));
  const unsigned long long b = dsh::wave_max_u64(dsh::d2u(v));
  if (threadIdx.x == 0) { out_f64[blockIdx.x] = a; out_u64[blockIdx.x] = b; }
}

// in: npat x 64 doubles (host); out_f64 / out_u64: npat results each (host).  Returns 0, or the HIP error code.
extern "C" int wave_max_both(const double* in, int npat, unsigned long long* out_f64, unsigned long long* out_u64) {
  if (npat <= 0) return 0;
  double* d_in = nullptr;
  unsigned long long* d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, sizeof(double) * 64 * (size_t)npat);
  if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(unsigned long long) * 2 * (size_t)npat);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, sizeof(double) * 64 * (size_t)npat, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_wave_max_both, dim3(npat), dim3(64), 0, 0, d_in, d_out, d_out + npat);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_f64, d_out, sizeof(unsigned long long) * (size_t)npat, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_u64, d_out + npat, sizeof(unsigned long long) * (size_t)npat, hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return (int)e;
}
