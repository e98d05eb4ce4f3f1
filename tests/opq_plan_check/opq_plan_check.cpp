// Stand-alone check of the hazard planner of the op queue (diffsol_amd/csrc/dsh_opq_plan.hpp): every case asserts an exact flush / no-flush decision.
// Built by tests/test_op_queue_plan.py with g++ -std=c++17 -fsanitize=address,undefined; includes nothing but the planner.  Prints one line per case,
// exits 1 if any decision is wrong.
#include <cstdio>
#include <vector>

#include "dsh_opq_plan.hpp"

using namespace dsh::opq;

static int g_failed = 0;
static void expect(const char* name, bool got, bool want) {
  std::printf("%-64s %s (flush=%d)\n", name, got == want ? "ok" : "WRONG", (int)got);
  if (got != want) ++g_failed;
}

static OpDesc mk(int op, int64_t n, int64_t nb, double* dst, const double* a, bool bca, const double* b, bool bcb, double* dst2 = nullptr) {
  OpDesc d;
  d.op = op; d.total = n * nb; d.nb = nb; d.dst = dst; d.dst2 = dst2; d.a = a; d.b = b; d.bca = bca; d.bcb = bcb;
  return d;
}

int main() {
  const int64_t n = 5, nb = 7, total = n * nb;
  // one arena: the "device" pointers are only compared, never dereferenced
  std::vector<double> arena((size_t)(64 * total));
  double* base = arena.data();
  double *x = base, *y = base + total, *z = base + 2 * total, *w = base + 3 * total, *D = base + 8 * total;  // D: n x 8 matrix, column j at D + j * total
  double* small = base + 40 * total;                                                                        // broadcast operands: n doubles

  {  // identical in-place ranges: x += y; x *= 2; x -= y; z = x + y
    Chain c;
    append(c, mk(OP_ADD, n, nb, x, x, false, y, false));
    expect("in place: same range written again", must_flush_before(c, mk(OP_SCALE, n, nb, x, x, false, nullptr, false)), false);
    append(c, mk(OP_SCALE, n, nb, x, x, false, nullptr, false));
    expect("in place: third op on the same ranges", must_flush_before(c, mk(OP_SUB, n, nb, x, x, false, y, false)), false);
    // a read of a just-written range
    expect("read of a just-written range", must_flush_before(c, mk(OP_ADD, n, nb, z, x, false, y, false)), false);
    // write-after-read of the identical range: y was only read so far
    expect("write after read, identical range", must_flush_before(c, mk(OP_FILL, n, nb, y, nullptr, false, nullptr, false)), false);
  }
  {  // the adjacent-column column_axpy ladder of an n x 8 matrix stays one chain: D[:,i] += D[:,i+1] for i = 6 .. 0, then y += D[:,0]
    Chain c;
    bool any = false;
    for (int i = 6; i >= 0; --i) {
      const OpDesc d = mk(OP_COLUMN_AXPY, n, nb, D + i * total, D + i * total, false, D + (i + 1) * total, false);
      any = any || must_flush_before(c, d);
      append(c, d);
    }
    const OpDesc d = mk(OP_ADD, n, nb, y, y, false, D, false);
    any = any || must_flush_before(c, d);
    append(c, d);
    expect("column ladder of an n x 8 matrix + add_assign: one chain", any, false);
    expect("column ladder: 8 ops recorded", c.count != 8, false);
  }
  {  // shifted ranges must flush
    Chain c;
    append(c, mk(OP_ADD, n, nb, x, x, false, y, false));
    expect("read shifted by one element over a written range", must_flush_before(c, mk(OP_COPY, n, nb, z, x + 1, false, nullptr, false)), true);
    expect("write shifted by one element over a written range", must_flush_before(c, mk(OP_FILL, n, nb, x + 1, nullptr, false, nullptr, false)), true);
    expect("write over the last element of a written range", must_flush_before(c, mk(OP_FILL, n, nb, x - 1 + total, nullptr, false, nullptr, false)), true);
    Chain m;
    append(m, mk(OP_COLUMN_AXPY, n, nb, D + total, D + total, false, D + 2 * total, false));
    expect("read shifted by one column minus one element", must_flush_before(m, mk(OP_COPY, n, nb, z, D + 1, false, nullptr, false)), true);
    expect("read shifted by exactly one column (adjacent, disjoint)", must_flush_before(m, mk(OP_COPY, n, nb, z, D, false, nullptr, false)), false);
    expect("read-read overlap, shifted: no hazard", must_flush_before(m, mk(OP_COPY, n, nb, z, D + 2 * total + 1, false, nullptr, false)), false);
  }
  {  // write-after-read overlap, not identical
    Chain c;
    append(c, mk(OP_COPY, n, nb, z, x, false, nullptr, false));  // reads x
    expect("write after read, shifted overlap", must_flush_before(c, mk(OP_FILL, n, nb, x + 3, nullptr, false, nullptr, false)), true);
    expect("second destination over a read range, shifted", must_flush_before(c, mk(OP_AXPY, n, nb, w, y, false, y, false, x + 2)), true);
    expect("second destination identical to a read range", must_flush_before(c, mk(OP_AXPY, n, nb, w, y, false, y, false, x)), false);
  }
  {  // broadcast operands
    Chain c;
    append(c, mk(OP_FILL, n, nb, x, nullptr, false, nullptr, false));  // writes x[0 .. total)
    expect("broadcast operand at the base of a written range", must_flush_before(c, mk(OP_ADD, n, nb, z, y, false, x, true)), true);
    expect("broadcast operand inside a written range", must_flush_before(c, mk(OP_ADD, n, nb, z, y, false, x + total - n, true)), true);
    expect("broadcast operand elsewhere", must_flush_before(c, mk(OP_ADD, n, nb, z, y, false, small, true)), false);
    Chain b;
    append(b, mk(OP_ADD, n, nb, z, y, false, small, true));  // reads the broadcast `small`
    expect("write over a broadcast operand read earlier", must_flush_before(b, mk(OP_FILL, n, nb, small - total + 1, nullptr, false, nullptr, false)), true);
    expect("broadcast read twice", must_flush_before(b, mk(OP_MUL, n, nb, z, z, false, small, true)), false);
    expect("the unused operand of an op is not a range (fill ignores a)", must_flush_before(c, mk(OP_FILL, n, nb, z, x + 1, false, nullptr, false)), false);
    expect("beta == 0 axpy does not read y", must_flush_before(c, mk(OP_AXPY0, n, nb, z, y, false, x + 1, false)), false);
  }
  {  // shape
    Chain c;
    append(c, mk(OP_FILL, n, nb, x, nullptr, false, nullptr, false));
    expect("differing total", must_flush_before(c, mk(OP_FILL, n + 1, nb, D, nullptr, false, nullptr, false)), true);
    expect("differing nb, equal total", must_flush_before(c, mk(OP_FILL, nb, n, D, nullptr, false, nullptr, false)), true);
    expect("same shape, disjoint", must_flush_before(c, mk(OP_FILL, n, nb, D, nullptr, false, nullptr, false)), false);
  }
  {  // the K+1-th op
    Chain c;
    for (int k = 0; k < kChainMax; ++k) {
      const OpDesc d = mk(OP_SCALE, n, nb, x, x, false, nullptr, false);
      if (must_flush_before(c, d)) { expect("ops 1 .. K join the chain", true, false); break; }
      append(c, d);
    }
    expect("K ops recorded", c.count != kChainMax, false);
    expect("the K+1-th op", must_flush_before(c, mk(OP_SCALE, n, nb, x, x, false, nullptr, false)), true);
    expect("the chain is small enough to travel as a kernel argument (< 4 KB)", sizeof(Chain) >= 4096, false);
  }
  {  // zero-length ops
    Chain c;
    expect("zero-length op on an empty chain", must_flush_before(c, mk(OP_FILL, 0, nb, x, nullptr, false, nullptr, false)), false);
    append(c, mk(OP_FILL, 0, nb, x, nullptr, false, nullptr, false));
    expect("zero-length ops never overlap", must_flush_before(c, mk(OP_COPY, 0, nb, x + 1, x, false, nullptr, false)), false);
    expect("a non-empty op after zero-length ones: another total", must_flush_before(c, mk(OP_FILL, n, nb, x, nullptr, false, nullptr, false)), true);
    Chain e;
    expect("anything on an empty chain", must_flush_before(e, mk(OP_COPY, n, nb, x + 1, x, false, nullptr, false)), false);
  }
  std::printf("%s\n", g_failed ? "FAILED" : "ALL OK");
  return g_failed ? 1 : 0;
}
