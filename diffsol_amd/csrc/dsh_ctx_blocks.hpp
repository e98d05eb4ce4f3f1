// The device blocks of one call: taken from a context with dsh_malloc, given back with dsh_free when the owner goes out of scope — on every way out of the call,
// the early error returns included.  The device-resident solve drivers take all their blocks through one of these and never call dsh_free themselves.
// Plain C++ over the C ABI alone (no HIP): tests/ctx_blocks_check builds it on the host against counting fakes of dsh_malloc / dsh_free.
#pragma once
#include "../../include/diffsol_hip.h"

namespace dsh {

class CtxBlocks {
 public:
  static constexpr int kMaxBlocks = 8;
  explicit CtxBlocks(dsh_ctx* ctx) : ctx_(ctx) {}
  ~CtxBlocks() {
    while (count_ > 0) (void)dsh_free(ctx_, held_[--count_]);
  }
  CtxBlocks(const CtxBlocks&) = delete;
  CtxBlocks& operator=(const CtxBlocks&) = delete;

  // dsh_malloc(ctx, bytes, zero, out), the block owned by this object.  On failure *out is null, the code is dsh_malloc's (DSH_E_INVALID for a block beyond
  // kMaxBlocks, which is not requested at all) and the blocks taken before stay held.
  template <class T>
  int take(int64_t bytes, int zero, T** out) {
    *out = nullptr;
    if (count_ == kMaxBlocks) return DSH_E_INVALID;
    void* p = nullptr;
    const int rc = dsh_malloc(ctx_, bytes, zero, &p);
    if (rc != DSH_OK) return rc;
    held_[count_++] = p;
    *out = static_cast<T*>(p);
    return DSH_OK;
  }
  int count() const { return count_; }

 private:
  dsh_ctx* ctx_;
  void* held_[kMaxBlocks] = {};
  int count_ = 0;
};

}  // namespace dsh
