// Deferred element-wise op queue of libdiffsol_hip.so (gfx950): dsh_ctx_set_op_queue / dsh_ctx_flush / dsh_ctx_op_queue_stats and the chain kernel.
//
// A caller that composes diffsol's Bdf / Sdirk from the 1:1 trait operations issues ~44 launches per step, most of them element-wise, same-index operations on
// 2.4 MB vectors whose device time is the dispatch floor.  With the queue on, those entry points record a descriptor (dsh_opq_plan.hpp) and
// the recorded run is launched as ONE kernel by the next call whose result the host or another kernel needs.  Thread idx evaluates every op of the chain at
// element idx, in order, with the functors of the kernels the ops replace (dsh_ew_ops.hpp; -ffp-contract=off): the stored bits are those of the separate launches.
#include "dsh_internal.hpp"
#include "dsh_ew_ops.hpp"

#include <cstdlib>

using namespace dsh;

namespace {

constexpr int kChainBlock = 256;
constexpr int kChainMaxBlocks = 4096;  // the grid cap of ew_grid (dsh_vec.hip)

// The chain is the kernel argument: the descriptors are read with scalar loads from the argument segment and the loop over them is wave-uniform.
// No __restrict__: aliasing between the ops of a chain is the normal case (in-place updates, a column read by the next op), and program order per thread is what
// makes it correct.
// Forwarding: the value an op just stored stays in (fwd_p, fwd_v); an operand of the next op that is the identical full-batch range (same base; the extent is the
// chain's) takes the register instead of the load.  The comparison is on descriptor fields: wave-uniform.  One slot, overwritten by every op: it can never be stale.
// Stores always happen.
__global__ __launch_bounds__(kChainBlock) void k_op_chain(const opq::Chain c) {
  using namespace dsh::opq;
  const int64_t total = c.total, nb = c.nb;
  const int count = c.count;
  const bool any_bcast = c.any_bcast != 0;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t bidx = any_bcast ? idx / nb : 0;  // the state index of broadcast operands: one division per element, whatever the number of broadcasts
    const double* fwd_p = nullptr;
    double fwd_v = 0.0;
    for (int k = 0; k < count; ++k) {
      const OpDesc& d = c.ops[k];
      const int32_t op = d.op;
      double av = 0.0, bv = 0.0;
      if (reads_a(op)) {
        const double* a = d.a;
        av = (!d.bca && a == fwd_p) ? fwd_v : a[d.bca ? bidx : idx];
      }
      if (reads_b(op)) {
        const double* b = d.b;
        bv = (!d.bcb && b == fwd_p) ? fwd_v : b[d.bcb ? bidx : idx];
      }
      double v;
      switch (op) {
        case OP_ADD: v = ew::FAdd{}(av, bv); break;
        case OP_SUB: v = ew::FSub{}(av, bv); break;
        case OP_MUL: v = ew::FMul{}(av, bv); break;
        case OP_DIV: v = ew::FDiv{}(av, bv); break;
        case OP_SCALE: v = ew::FScale{d.s0}(av); break;
        case OP_AXPY: v = ew::FAxpy{d.s0, d.s1}(bv, av); break;
        case OP_AXPY0: v = ew::FAxpy0{d.s0}(0.0, av); break;
        case OP_FILL: v = ew::FConst{d.s0}(idx); break;
        case OP_SCALE_ADD: v = ew::FScaleAdd{d.s0}(av, bv); break;
        case OP_COLUMN_AXPY: v = ew::FColumnAxpy{d.s0}(av, bv); break;
        default: v = av; break;  // OP_COPY
      }
      double* dst = d.dst;
      dst[idx] = v;
      double* dst2 = d.dst2;
      if (dst2) dst2[idx] = av;
      fwd_p = dst;
      fwd_v = v;
    }
  }
}

inline dim3 chain_grid(int64_t total) {
  int64_t blocks = (total + kChainBlock - 1) / kChainBlock;
  if (blocks > kChainMaxBlocks) blocks = kChainMaxBlocks;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

}  // namespace

namespace dsh {

int opq_flush(dsh_ctx* ctx, int why) {
  opq::Chain& c = ctx->opq;
  if (c.count == 0) return DSH_OK;
  hipLaunchKernelGGL(k_op_chain, chain_grid(c.total), dim3(kChainBlock), 0, ctx->stream, c);
  c.count = 0;  // whatever the launch returned: a chain that failed is reported once, by this call, and not launched again
  ctx->opq_stats[1] += 1;
  if (why == kOpqFlushHazard || why == kOpqFlushEntry) ctx->opq_stats[why] += 1;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(std::string("k_op_chain launch failed: ") + hipGetErrorString(e));
    return DSH_E_HIP;
  }
  return DSH_OK;
}

int opq_enqueue(dsh_ctx* ctx, int32_t op, int64_t n, int64_t nb, double* dst, double* dst2, const double* a, int64_t anb, const double* b, int64_t bnb, double s0,
                double s1) {
  opq::OpDesc d;
  d.total = n * nb;
  if (d.total == 0) return DSH_OK;  // as the immediate kernels: nothing to do
  d.nb = nb;
  d.op = op;
  d.dst = dst; d.dst2 = dst2; d.a = a; d.b = b;
  d.s0 = s0; d.s1 = s1;
  d.bca = anb == 1 && nb != 1;
  d.bcb = bnb == 1 && nb != 1;
  if (opq::must_flush_before(ctx->opq, d)) {
    const int rc = opq_flush(ctx, kOpqFlushHazard);
    if (rc != DSH_OK) return rc;
  }
  opq::append(ctx->opq, d);
  ctx->opq_stats[0] += 1;
  return DSH_OK;
}

}  // namespace dsh

extern "C" {

int dsh_ctx_set_op_queue(dsh_ctx* ctx, int on) {
  DSH_ENTER(ctx);  // flushes: switching off leaves nothing queued
  DSH_REQUIRE(ctx != nullptr, "null context");
  ctx->opq_on = on != 0;
  for (int i = 0; i < 4; ++i) ctx->opq_stats[i] = 0;
  return DSH_OK;
}
int dsh_ctx_get_op_queue(const dsh_ctx* ctx) { return ctx ? (ctx->opq_on ? 1 : 0) : -1; }
int dsh_ctx_flush(dsh_ctx* ctx) {
  DSH_ENTER_QUEUE(ctx);
  DSH_REQUIRE(ctx != nullptr, "null context");
  return opq_flush(ctx, kOpqFlushExplicit);
}
int dsh_ctx_op_queue_stats(dsh_ctx* ctx, int64_t* out) {
  DSH_ENTER_QUEUE(ctx);
  DSH_REQUIRE(ctx != nullptr && out != nullptr, "null argument");
  for (int i = 0; i < 4; ++i) out[i] = ctx->opq_stats[i];
  return DSH_OK;
}

}  // extern "C"
