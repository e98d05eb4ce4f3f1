// The element-wise expressions of the vector / matrix kernels (dsh_vec.hip, dsh_mat.hip), one definition each: the immediate kernels and the chain kernel of the
// op queue (dsh_opq.hip) evaluate the same functor, so the two paths cannot drift apart.  Built with -ffp-contract=off: the order written here is the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dsh {
namespace ew {

struct FAdd { __device__ double operator()(double a, double b) const { return a + b; } };
struct FSub { __device__ double operator()(double a, double b) const { return a - b; } };
struct FMul { __device__ double operator()(double a, double b) const { return a * b; } };
struct FDiv { __device__ double operator()(double a, double b) const { return a / b; } };
struct FScale { double s; __device__ double operator()(double a) const { return a * s; } };
struct FConst { double v; __device__ double operator()(int64_t) const { return v; } };
// y = alpha*x + beta*y ; beta == 0 never reads y (nalgebra axcpy / the oracle's axpy)
struct FAxpy { double alpha, beta; __device__ double operator()(double y, double x) const { return alpha * x + beta * y; } };
struct FAxpy0 { double alpha; __device__ double operator()(double, double x) const { return alpha * x; } };
// self = y*beta + x  (dense_nalgebra_serial.rs:325-329 order: copy y, scale by beta, add x)
struct FScaleAdd { double beta; __device__ double operator()(double x, double y) const { return y * beta + x; } };
// column i += alpha*column j  (value = self[k,i] + alpha*self[k,j])
struct FColumnAxpy { double alpha; __device__ double operator()(double ci, double cj) const { return ci + alpha * cj; } };

}  // namespace ew
}  // namespace dsh
