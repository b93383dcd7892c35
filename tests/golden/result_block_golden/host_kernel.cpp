// ResultBlock and BlockLayout (fuel_amd/csrc/block_layout.h) on host memory only, as a stand-alone program under the
// address and undefined-behaviour sanitizers: sizing against binding, alignment, the three kinds of entry, the scatter
// between guard bytes, element counts 0 and 1, a block embedded in a larger BlockLayout, and the overflow of the table.
// Prints one line per failed check and, last, the verdict; the exit status is 1 when a check failed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "block_layout.h"

namespace {

int g_checks = 0, g_bad = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    ++g_checks;                                                     \
    if (!(cond)) {                                                  \
      ++g_bad;                                                      \
      printf("FAILED %s:%d (align %zu): %s\n", __FILE__, __LINE__, g_align, #cond); \
    }                                                               \
  } while (0)
size_t g_align = 0;

struct Args {  // as a kernel's: scalars among the result pointers
  int n_prob;
  int* status;
  double* cost;
  double scale;
  double* ctrl;
  double* dctrl;  // optional
  int* skip;      // the kernel's own
  unsigned char* mask;
  int* none;  // count 0
  int* one;   // count 1
};

constexpr size_t GUARD = 32;
constexpr unsigned char GUARD_BYTE = 0xA5, UNSET = 0x5A;

// a destination of `bytes` bytes between two guard zones
struct Guarded {
  std::vector<unsigned char> mem;
  size_t bytes;
  explicit Guarded(size_t bytes_) : mem(bytes_ + 2 * GUARD, GUARD_BYTE), bytes(bytes_) { memset(mem.data() + GUARD, UNSET, bytes); }
  template <class T>
  T* p() {
    return reinterpret_cast<T*>(mem.data() + GUARD);
  }
  bool guards_whole() const {
    for (size_t i = 0; i < GUARD; ++i)
      if (mem[i] != GUARD_BYTE || mem[GUARD + bytes + i] != GUARD_BYTE) return false;
    return true;
  }
  // every byte is the block's pattern at offset `off`
  bool holds(size_t off) const {
    for (size_t i = 0; i < bytes; ++i)
      if (mem[GUARD + i] != (unsigned char)((off + i) * 7 + 1)) return false;
    return true;
  }
  bool untouched() const {
    for (size_t i = 0; i < bytes; ++i)
      if (mem[GUARD + i] != UNSET) return false;
    return true;
  }
};

size_t padded(size_t bytes, size_t align) { return (bytes + align - 1) / align * align; }

void run(size_t align, bool with_dctrl) {
  g_align = align;
  const size_t n = 3, row = 5;
  Args A;
  memset(&A, 0xFF, sizeof(A));  // (no field is null before it is declared)
  A.n_prob = 3, A.scale = 2.5;
  Guarded status(n * sizeof(int)), cost(n * sizeof(double)), ctrl(n * row * sizeof(double)), dctrl(n * (row - 1) * sizeof(double)),
      mask(7), none(0), one(sizeof(int));
  ResultBlock R(align);
  R.add(A.status, status.p<int>(), n);
  R.add(A.cost, cost.p<double>(), n);
  R.add(A.ctrl, ctrl.p<double>(), n * row);
  R.opt(A.dctrl, with_dctrl ? dctrl.p<double>() : nullptr, n * (row - 1));
  R.hold(A.skip, n);
  R.add(A.mask, mask.p<unsigned char>(), 7);
  R.add(A.none, none.p<int>(), 0);
  R.add(A.one, one.p<int>(), 1);
  CHECK(!R.overflow);
  CHECK(R.n == (with_dctrl ? 8 : 7));

  // the size: every present array padded to the alignment, an absent one nothing, a count of 0 nothing
  const size_t want = padded(n * 4, align) + padded(n * 8, align) + padded(n * row * 8, align) +
                      (with_dctrl ? padded(n * (row - 1) * 8, align) : 0) + padded(n * 4, align) + padded(7, align) + 0 +
                      padded(4, align);
  CHECK(R.size() == want);
  // the same takes by BlockLayout: the same size
  {
    BlockLayout L(nullptr, align);
    L.take<int>(n), L.take<double>(n), L.take<double>(n * row);
    if (with_dctrl) L.take<double>(n * (row - 1));
    L.take<int>(n), L.take<unsigned char>(7), L.take<int>(0), L.take<int>(1);
    CHECK(L.size() == R.size());
  }
  // the sizing pass of a block it is a region of: every field null, the scalars as they were
  R.bind(nullptr);
  CHECK(!A.status && !A.cost && !A.ctrl && !A.dctrl && !A.skip && !A.mask && !A.none && !A.one);
  CHECK(A.n_prob == 3 && A.scale == 2.5);

  // bound inside a larger block, behind an input array and in front of a workspace: where the outer layout says
  std::vector<unsigned char> raw(3 * 256 + R.size() + 2 * 256);
  unsigned char* base = raw.data() + (256 - reinterpret_cast<uintptr_t>(raw.data()) % 256) % 256;
  unsigned char *in = nullptr, *work = nullptr;
  auto layout = [&](unsigned char* b) {
    BlockLayout L(b, align);
    in = L.take<unsigned char>(37);
    R.place(L);
    work = L.take<unsigned char>(11);
    return L.size();
  };
  const size_t outer = layout(nullptr);
  CHECK(outer == padded(37, align) + R.size() + padded(11, align));
  CHECK(R.base == nullptr && !A.status);
  CHECK(layout(base) == outer);
  CHECK(in == base && R.base == base + padded(37, align) && work == R.base + R.size());
  CHECK(A.n_prob == 3 && A.scale == 2.5);

  // every array on the alignment, inside the block, in the order declared, none overlapping the next
  struct Span {
    const void* p;
    size_t bytes;
  };
  std::vector<Span> spans = {{A.status, n * 4}, {A.cost, n * 8}, {A.ctrl, n * row * 8}};
  if (with_dctrl) spans.push_back({A.dctrl, n * (row - 1) * 8});
  spans.push_back({A.skip, n * 4}), spans.push_back({A.mask, 7}), spans.push_back({A.none, 0}), spans.push_back({A.one, 4});
  const unsigned char* at = R.base;
  for (const Span& s : spans) {
    const unsigned char* p = static_cast<const unsigned char*>(s.p);
    CHECK(p != nullptr);
    CHECK(reinterpret_cast<uintptr_t>(p) % align == 0);
    CHECK(p >= at && p + s.bytes <= R.base + R.size());
    at = p + s.bytes;
  }
  if (!with_dctrl) CHECK(A.dctrl == nullptr);
  CHECK(static_cast<const unsigned char*>(spans.back().p) + padded(4, align) == R.base + R.size());  // sizing == binding

  // the scatter: exactly count * sizeof(T) bytes of each array into its destination, nothing into the guards, nothing
  // for the held entry and the absent one
  for (size_t i = 0; i < R.size(); ++i) R.base[i] = (unsigned char)(i * 7 + 1);
  R.scatter(R.base);
  auto off = [&](const void* p) { return (size_t)(static_cast<const unsigned char*>(p) - R.base); };
  CHECK(status.holds(off(A.status)) && cost.holds(off(A.cost)) && ctrl.holds(off(A.ctrl)) && mask.holds(off(A.mask)) &&
        one.holds(off(A.one)));
  if (with_dctrl)
    CHECK(dctrl.holds(off(A.dctrl)));
  else
    CHECK(dctrl.untouched());
  CHECK(status.guards_whole() && cost.guards_whole() && ctrl.guards_whole() && dctrl.guards_whole() && mask.guards_whole() &&
        none.guards_whole() && one.guards_whole());

  // bound again on another base (a host image of a device block): the fields follow, the scatter reads the image given
  std::vector<unsigned char> image(R.size() + 256);
  unsigned char* himg = image.data() + (256 - reinterpret_cast<uintptr_t>(image.data()) % 256) % 256;
  const size_t status_off = off(A.status), one_off = off(A.one);
  R.bind(himg);
  CHECK(reinterpret_cast<unsigned char*>(A.status) == himg + status_off && reinterpret_cast<unsigned char*>(A.one) == himg + one_off);
}

void overflow() {
  g_align = 16;
  struct Many {
    int* f[ResultBlock::CAP + 2];
    int tail;
  } M;
  memset(&M, 0xFF, sizeof(M));
  M.tail = 77;
  std::vector<Guarded> dst(ResultBlock::CAP + 2, Guarded(4));
  ResultBlock R(16);
  for (int i = 0; i < ResultBlock::CAP; ++i) R.add(M.f[i], dst[i].p<int>(), 1);
  CHECK(!R.overflow && R.n == ResultBlock::CAP && R.size() == 16u * ResultBlock::CAP);
  R.add(M.f[ResultBlock::CAP], dst[ResultBlock::CAP].p<int>(), 1);
  R.opt(M.f[ResultBlock::CAP + 1], dst[ResultBlock::CAP + 1].p<int>(), 1);
  // reported; the table and the size as they were; the dropped fields null, so that nothing writes through them
  CHECK(R.overflow && R.n == ResultBlock::CAP && R.size() == 16u * ResultBlock::CAP);
  alignas(16) unsigned char block[16 * ResultBlock::CAP];
  for (size_t i = 0; i < sizeof(block); ++i) block[i] = (unsigned char)(i * 7 + 1);
  R.bind(block);
  CHECK(M.f[ResultBlock::CAP] == nullptr && M.f[ResultBlock::CAP + 1] == nullptr && M.tail == 77);
  R.scatter(block);
  for (int i = 0; i < ResultBlock::CAP; ++i) CHECK(dst[i].holds(16u * i) && dst[i].guards_whole());
  CHECK(dst[ResultBlock::CAP].untouched() && dst[ResultBlock::CAP + 1].untouched());
}

void limit_scan() {
  const int st[5] = {0, 2, -1, -2, -1};
  CHECK(first_over_limit(st, 5) == 2);
  CHECK(first_over_limit(st, 2) == -1);
  CHECK(first_over_limit(st + 3, 2) == 1);
  CHECK(first_over_limit(st, 0) == -1);
}

}  // namespace

int main() {
  for (size_t align : {(size_t)16, (size_t)256})
    for (bool with_dctrl : {true, false}) run(align, with_dctrl);
  overflow();
  limit_scan();
  printf("%d checks: %s\n", g_checks, g_bad ? "FAILED" : "all passed, sanitizers silent");
  return g_bad ? 1 : 0;
}
