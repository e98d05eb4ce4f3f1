// Stand-alone check of the owner of a call's device blocks (diffsol_amd/csrc/dsh_ctx_blocks.hpp): every block taken is given back exactly once, to the context it
// came from, on every way out of a scope — normal end, a failing k-th allocation, an early return.  Built by tests/test_ctx_blocks.py with
// g++ -std=c++17 -fsanitize=address,undefined; includes nothing but the header.  dsh_malloc / dsh_free are counting fakes over malloc with an opaque context; the
// sanitizer sees a block that is never returned (leak) or returned twice.  Prints one line per case, exits 1 if any is wrong.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <type_traits>

#include "dsh_ctx_blocks.hpp"

struct dsh_ctx { int id; };

namespace {
struct Fake {
  std::map<void*, dsh_ctx*> live;  // block -> the context it was taken from
  int mallocs = 0, frees = 0, bad_frees = 0, calls = 0, fail_at = 0;  // fail_at = k > 0: the k-th dsh_malloc from now fails
  void reset(int k) { mallocs = frees = bad_frees = calls = 0; fail_at = k; }
} g;
int g_failed = 0;
void expect(const char* name, bool ok) {
  std::printf("%-72s %s\n", name, ok ? "ok" : "WRONG");
  if (!ok) ++g_failed;
}
}  // namespace

extern "C" int dsh_malloc(dsh_ctx* ctx, int64_t nbytes, int zero, void** out) {
  if (++g.calls == g.fail_at) return DSH_E_HIP;
  void* p = zero ? std::calloc(1, (size_t)nbytes) : std::malloc((size_t)nbytes);
  if (!p) return DSH_E_HIP;
  g.live[p] = ctx;
  ++g.mallocs;
  *out = p;
  return DSH_OK;
}
extern "C" int dsh_free(dsh_ctx* ctx, void* p) {
  auto it = g.live.find(p);
  if (it == g.live.end() || it->second != ctx) { ++g.bad_frees; return DSH_E_INVALID; }  // unknown, returned twice, or the wrong context
  g.live.erase(it);
  std::free(p);
  ++g.frees;
  return DSH_OK;
}

// the shape of a driver: up to four blocks, return at the first failure; `held` = the owner's count on the way out
static int take_four(dsh_ctx* ctx, int* held, bool leave_after_two = false) {
  dsh::CtxBlocks blocks(ctx);
  double *a = nullptr, *b = nullptr, *d = nullptr;
  unsigned long long* c = nullptr;
  struct Out { dsh::CtxBlocks& bl; int* held; ~Out() { *held = bl.count(); } } out{blocks, held};
  int rc = blocks.take(64, 0, &a);
  if (rc != DSH_OK) return a == nullptr ? rc : -100;
  a[7] = 1.0;
  rc = blocks.take(24, 0, &b);
  if (rc != DSH_OK) return b == nullptr ? rc : -100;
  b[2] = 2.0;
  if (leave_after_two) return 77;
  rc = blocks.take(64, 1, &c);
  if (rc != DSH_OK) return c == nullptr ? rc : -100;
  if (c[0] != 0 || c[7] != 0) return -101;  // zero = 1 reached dsh_malloc
  rc = blocks.take(800, 0, &d);
  if (rc != DSH_OK) return d == nullptr ? rc : -100;
  d[99] = 3.0;
  return DSH_OK;
}

int main() {
  dsh_ctx c1{1}, c2{2};
  int held = -1;
  {
    g.reset(0);
    const int rc = take_four(&c1, &held);
    expect("normal use: four blocks taken", rc == DSH_OK && held == 4 && g.mallocs == 4);
    expect("normal use: every block returned once, to its context", g.frees == 4 && g.bad_frees == 0 && g.live.empty());
  }
  {  // two owners on two contexts, interleaved: each block goes back to the context it came from
    g.reset(0);
    {
      dsh::CtxBlocks b1(&c1), b2(&c2);
      double *x = nullptr, *y = nullptr, *z = nullptr;
      const bool took = b1.take(8, 0, &x) == DSH_OK && b2.take(8, 0, &y) == DSH_OK && b1.take(16, 0, &z) == DSH_OK;
      expect("two contexts: blocks are booked under their own context", took && g.live[x] == &c1 && g.live[y] == &c2 && g.live[z] == &c1);
    }
    expect("two contexts: every block returned by the right context pointer", g.frees == 3 && g.bad_frees == 0 && g.live.empty());
  }
  for (int k = 1; k <= 4; ++k) {
    g.reset(k);
    const int rc = take_four(&c1, &held);
    char name[96];
    std::snprintf(name, sizeof name, "allocation %d fails: code passed on, %d earlier blocks held", k, k - 1);
    expect(name, rc == DSH_E_HIP && held == k - 1 && g.mallocs == k - 1);
    std::snprintf(name, sizeof name, "allocation %d fails: earlier blocks returned, none twice", k);
    expect(name, g.frees == k - 1 && g.bad_frees == 0 && g.live.empty());
  }
  {  // a failure leaves the object valid: it takes further blocks and returns all of them
    g.reset(2);
    {
      dsh::CtxBlocks blocks(&c1);
      double *x = nullptr, *y = nullptr, *z = nullptr;
      const int r1 = blocks.take(8, 0, &x), r2 = blocks.take(8, 0, &y), r3 = blocks.take(8, 0, &z);
      expect("after a failure the owner still takes blocks", r1 == DSH_OK && r2 == DSH_E_HIP && y == nullptr && r3 == DSH_OK && z != nullptr && blocks.count() == 2);
    }
    expect("after a failure: both blocks returned", g.frees == 2 && g.bad_frees == 0 && g.live.empty());
  }
  {
    g.reset(0);
    const int rc = take_four(&c2, &held, true);
    expect("scope left early with two blocks held", rc == 77 && held == 2 && g.mallocs == 2);
    expect("scope left early: both returned", g.frees == 2 && g.bad_frees == 0 && g.live.empty());
  }
  {
    g.reset(0);
    { dsh::CtxBlocks blocks(&c1); expect("zero blocks: nothing held", blocks.count() == 0); }
    expect("zero blocks: dsh_malloc / dsh_free never called", g.calls == 0 && g.frees == 0 && g.bad_frees == 0);
  }
  {  // more blocks than the owner has room for: refused without a request, the held ones still returned
    g.reset(0);
    {
      dsh::CtxBlocks blocks(&c1);
      double* x = nullptr;
      bool ok = true;
      for (int k = 0; k < dsh::CtxBlocks::kMaxBlocks; ++k) ok = ok && blocks.take(8, 0, &x) == DSH_OK;
      const int rc = blocks.take(8, 0, &x);
      expect("a block beyond the capacity is refused, not requested", ok && rc == DSH_E_INVALID && x == nullptr && g.calls == dsh::CtxBlocks::kMaxBlocks);
    }
    expect("capacity: every held block returned", g.frees == dsh::CtxBlocks::kMaxBlocks && g.bad_frees == 0 && g.live.empty());
  }
  static_assert(!std::is_copy_constructible<dsh::CtxBlocks>::value && !std::is_copy_assignable<dsh::CtxBlocks>::value, "the owner must not be copyable");
  if (g_failed) { std::printf("%d FAILED\n", g_failed); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
