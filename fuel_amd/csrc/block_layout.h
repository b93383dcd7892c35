// block_layout.h -- how the batched calls lay typed arrays out in one block, and how their results come back out of it
// (host code only, no HIP: it builds stand-alone).  Included by scratch.h.
#ifndef FUELMI_BLOCK_LAYOUT_H_
#define FUELMI_BLOCK_LAYOUT_H_

#include <cstddef>
#include <cstring>

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

// The result arrays of one batched call, each declared once: the kernel-args field the device writes through, the
// caller's array, the element count.  From the declarations: size() (BlockLayout's padding rule), bind() (every field
// to its address in a block at `base`, device or host; null base: every field null) and scatter() (a host-readable
// image of the block into the caller's arrays).  Three kinds of entry: add() with a destination is in the block and
// copied; add() with a null destination (or hold()) is in the block and not copied; opt() with a null destination is
// absent: its field is null and it takes no bytes.  The fields are remembered by address, so the args struct stays
// where it is between the declarations and the last bind().
struct ResultBlock {
  static constexpr int CAP = 18;  // the largest user: the kinodynamic search
  struct Entry {
    void* field;  // the address of a T* in the args struct
    void* dst;    // the caller's array, or null: not copied
    size_t bytes, off;
  };
  Entry e[CAP];
  int n = 0;
  bool overflow = false;  // a declaration beyond CAP: dropped, its field null; callers ARGCHK(!overflow)
  size_t align, at = 0;
  unsigned char* base = nullptr;  // where bind() last put the block
  explicit ResultBlock(size_t align_) : align(align_) {}

  template <class T>
  void add(T*& field, T* dst, size_t count) {
    field = nullptr;
    if (n == CAP) {
      overflow = true;
      return;
    }
    e[n++] = {&field, dst, count * sizeof(T), at};
    at += (count * sizeof(T) + align - 1) & ~(align - 1);
  }
  template <class T>
  void hold(T*& field, size_t count) {
    add(field, static_cast<T*>(nullptr), count);
  }
  template <class T>
  void opt(T*& field, T* dst, size_t count) {
    if (dst)
      add(field, dst, count);
    else
      field = nullptr;
  }

  size_t size() const { return at; }
  void bind(unsigned char* base_) {
    base = base_;
    for (int i = 0; i < n; ++i) {
      unsigned char* p = base ? base + e[i].off : nullptr;
      memcpy(e[i].field, &p, sizeof(p));
    }
  }
  // as one region of a larger block
  void place(BlockLayout& L) { bind(L.take<unsigned char>(at)); }
  void scatter(const unsigned char* host) const {
    for (int i = 0; i < n; ++i)
      if (e[i].dst && e[i].bytes) memcpy(e[i].dst, host + e[i].off, e[i].bytes);
  }
};

// the first problem a batched kernel stopped at one of its limits (status -1), or -1
inline int first_over_limit(const int* status, int n_prob) {
  for (int b = 0; b < n_prob; ++b)
    if (status[b] == -1) return b;
  return -1;
}

#endif
