// scratch.h -- the device scratch of the batched calls (host code only): a grow-only pool; with it, from
// block_layout.h, the carver that lays typed arrays out in one block (BlockLayout) and the descriptor of the arrays a
// call brings back from it (ResultBlock).  Included by fuelmi_internal.h, below HIPCHK.
#ifndef FUELMI_SCRATCH_H_
#define FUELMI_SCRATCH_H_

#include <cstddef>

#include "block_layout.h"

// One grow-only device block.  A call sizes its arrays (BlockLayout on a null base), reserves, and carves; what it
// carved is valid until the next reserve of the same pool.
struct DevScratch {
  void* p = nullptr;
  size_t bytes = 0;
  // at least `need` bytes: when the block is too small, the work queued on `st` (the only user of the block) is waited
  // for, the block freed and a new one allocated -- one allocation per call at most.  A failed allocation leaves the
  // pool empty.
  int reserve(hipStream_t st, size_t need) {
    if (need <= bytes) return FUELMI_OK;
    HIPCHK(hipStreamSynchronize(st));
    release();
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, need));
    p = q;
    bytes = need;
    return FUELMI_OK;
  }
  void release() {  // also for destructors: the result of the free is not looked at
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  unsigned char* base() const { return static_cast<unsigned char*>(p); }
  // `layout(base)` carves a call's arrays and returns their size: sized on a null base, reserved, carved on the block
  template <class F>
  int carve(hipStream_t st, F&& layout) {
    const int rc = reserve(st, layout(nullptr));
    if (rc) return rc;
    layout(base());
    return FUELMI_OK;
  }
};

#endif
