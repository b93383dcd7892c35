// scratch.h -- the device scratch of the batched calls (host code only): a grow-only pool, and the carver that lays
// typed arrays out in one block.  Included by fuelmi_internal.h, below HIPCHK.
#ifndef FUELMI_SCRATCH_H_
#define FUELMI_SCRATCH_H_

#include <cstddef>

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
};

// Arrays taken one after the other from a block whose base is aligned to `align` (a power of two); every array's
// size is padded to `align`, so every array starts aligned.  A null base is the sizing pass: take() returns null and
// size() is what the same takes need.
struct BlockLayout {
  unsigned char* base;
  size_t align;
  size_t at = 0;
  BlockLayout(unsigned char* base_, size_t align_) : base(base_), align(align_) {}
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
    at += (count * sizeof(T) + align - 1) & ~(align - 1);
    return p;
  }
  size_t size() const { return at; }
};

#endif
