// Hazard planner of the deferred element-wise op queue (dsh_opq.hip).  Pure C++17, no HIP include: tests/opq_plan_check builds it with g++ alone.
//
// With the queue of a context switched on (dsh_ctx_set_op_queue), the element-wise entry points record an OpDesc instead of launching; the recorded run — a
// Chain — is executed by ONE launch of k_op_chain, in which thread idx evaluates every op of the chain, in order, at element idx.  That is only the same as
// launching the ops one after the other when no thread reads or overwrites an element another thread of the same launch writes.  must_flush_before is the
// whole rule; the kernel relies on nothing finer.
#pragma once
#include <cstdint>

namespace dsh {
namespace opq {

// dst (and dst2) = f(a, b, s0, s1); which of a / b an op reads: reads_a / reads_b.  The expressions are those of the kernels the ops replace (dsh_ew_ops.hpp).
enum Opcode : int32_t {
  OP_ADD = 0,      // a + b
  OP_SUB,          // a - b
  OP_MUL,          // a * b
  OP_DIV,          // a / b
  OP_SCALE,        // a * s0
  OP_AXPY,         // s0 * a + s1 * b   (a = x, b = y or y0); dst2, when set, receives a (dsh_vec_axpby_to's copy_x_to)
  OP_AXPY0,        // s0 * a            (beta == 0: y is never read)
  OP_COPY,         // a
  OP_FILL,         // s0
  OP_SCALE_ADD,    // b * s0 + a        (a = x, b = y, s0 = beta)
  OP_COLUMN_AXPY,  // a + s0 * b        (a = the column itself, b = the other column)
  OP_COUNT
};

struct OpDesc {
  double* dst = nullptr;
  double* dst2 = nullptr;  // optional second destination (full batch, like dst)
  const double* a = nullptr;
  const double* b = nullptr;
  double s0 = 0.0, s1 = 0.0;
  int64_t total = 0;  // elements of dst: states * nb
  int64_t nb = 1;
  int32_t op = OP_COPY;
  uint8_t bca = 0, bcb = 0;  // operand is a broadcast: total / nb elements, element idx / nb is read
  uint8_t pad_[2] = {0, 0};
};

// K: the chain travels BY VALUE as the kernel argument (no H2D copy, no device buffer to keep alive).  72 bytes per descriptor, 32 descriptors + 24 bytes of
// header = 2328 bytes, well under the 4 KB the kernel-argument segment holds.
constexpr int kChainMax = 32;

struct Chain {
  int64_t total = 0, nb = 1;
  int32_t count = 0;
  int32_t any_bcast = 0;  // some operand of the chain is a broadcast: the kernel divides idx by nb once per element
  OpDesc ops[kChainMax];
};
static_assert(sizeof(OpDesc) == 72, "OpDesc layout");
static_assert(sizeof(Chain) <= 2560, "the chain must stay well under the 4 KB kernel-argument limit");

constexpr bool reads_a(int32_t op) { return op != OP_FILL; }
constexpr bool reads_b(int32_t op) { return op == OP_ADD || op == OP_SUB || op == OP_MUL || op == OP_DIV || op == OP_AXPY || op == OP_SCALE_ADD || op == OP_COLUMN_AXPY; }

struct Range {
  const double* p;
  int64_t len;  // elements
  bool write, bcast;
};
// the (at most four) ranges an op touches
inline int ranges_of(const OpDesc& d, Range out[4]) {
  int k = 0;
  out[k++] = Range{d.dst, d.total, true, false};
  if (d.dst2) out[k++] = Range{d.dst2, d.total, true, false};
  if (reads_a(d.op)) out[k++] = Range{d.a, d.bca ? d.total / d.nb : d.total, false, d.bca != 0};
  if (reads_b(d.op)) out[k++] = Range{d.b, d.bcb ? d.total / d.nb : d.total, false, d.bcb != 0};
  return k;
}
inline bool overlap(const Range& x, const Range& y) {
  if (x.len <= 0 || y.len <= 0) return false;
  const uintptr_t x0 = (uintptr_t)x.p, x1 = x0 + (uintptr_t)x.len * sizeof(double), y0 = (uintptr_t)y.p, y1 = y0 + (uintptr_t)y.len * sizeof(double);
  return x0 < y1 && y0 < x1;
}
// same base, same extent, both full-batch: thread idx is the only one that touches element idx of either
inline bool identical(const Range& x, const Range& y) { return x.p == y.p && x.len == y.len && !x.bcast && !y.bcast; }

// true when two ranges of ONE launch may not coexist: they overlap, one of them is written, and they are not the identical full-batch range
inline bool conflict(const Range& x, const Range& y) { return (x.write || y.write) && overlap(x, y) && !identical(x, y); }

// Must the chain be launched before `d` may be recorded?
inline bool must_flush_before(const Chain& c, const OpDesc& d) {
  if (c.count == 0) return false;
  if (c.count >= kChainMax) return true;
  if (c.total != d.total || c.nb != d.nb) return true;
  Range nr[4], cr[4];
  const int nn = ranges_of(d, nr);
  // (within the new op itself the entry point's own aliasing rules hold, as for the immediate kernel)
  for (int k = 0; k < c.count; ++k) {
    const int nc = ranges_of(c.ops[k], cr);
    for (int i = 0; i < nc; ++i)
      for (int j = 0; j < nn; ++j)
        if (conflict(cr[i], nr[j])) return true;
  }
  return false;
}

inline void append(Chain& c, const OpDesc& d) {
  if (c.count == 0) { c.total = d.total; c.nb = d.nb; c.any_bcast = 0; }
  if ((d.bca && reads_a(d.op)) || (d.bcb && reads_b(d.op))) c.any_bcast = 1;
  c.ops[c.count++] = d;
}

}  // namespace opq
}  // namespace dsh
