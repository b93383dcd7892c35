// host_lanes.h -- what the host builds of kernel text under tests/golden share: a kernel's own text (cut out of its .hip
// into kernel.inc by the driver's check script) compiled by plain g++ and run with a thread per lane.
//   threadIdx / blockIdx / blockDim   thread-local
//   __syncthreads()                   a barrier over the workgroup; a lane that leaves the kernel drops out of it
//   __shfl, __shfl_up, __ballot       exchanges through a per-wave block behind a per-wave barrier (wave_barrier())
//   __shared__ arrays                 statics (the address sanitizer puts red zones round them)
//   dynamic LDS                       g_lds: a heap block of exactly the launch's size between two guard zones
// Meant for -fsanitize=address,undefined with every array the kernel sees a heap block of its exact size: a read or write
// past one is reported by the sanitizer, a write inside a guard zone by launch().  A driver includes this file, then
// spline_internal.h if its kernel does, then kernel.inc, and keeps what is its own: the arguments it reads, the arrays,
// what it prints.
#ifndef FUELMI_TESTS_HOST_LANES_H_
#define FUELMI_TESTS_HOST_LANES_H_

#define __HIP_PLATFORM_AMD__ 1
#include "fuelmi_internal.h"
#include <barrier>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <thread>
#include <vector>
using namespace std;

#undef __launch_bounds__
#define __launch_bounds__(x)
#undef __shared__
#define __shared__ static
struct Idx { int x; };
static thread_local Idx threadIdx_, blockIdx_, blockDim_;
#define threadIdx threadIdx_
#define blockIdx blockIdx_
#define blockDim blockDim_

using Barrier = std::barrier<>;
static std::unique_ptr<Barrier>* g_bars;  // the running launch's, one per workgroup
#define __syncthreads() g_bars[blockIdx_.x]->arrive_and_wait()

struct WaveBlock {
  Barrier bar{64};
  u64 slot[64];
};
static WaveBlock* g_waves;  // the running workgroup's, one per wave
static inline WaveBlock& my_wave() { return g_waves[threadIdx_.x >> 6]; }
static inline void wave_barrier() { my_wave().bar.arrive_and_wait(); }

// every lane of the wave posts v, then takes read(the 64 posted values, its lane)
template <class T, class F>
static auto wave_exchange(T v, F read) {
  static_assert(sizeof(T) <= sizeof(u64), "a slot holds 8 bytes");
  WaveBlock& w = my_wave();
  const int lane = threadIdx_.x & 63;
  memcpy(&w.slot[lane], &v, sizeof(T));
  w.bar.arrive_and_wait();
  const auto r = read(w.slot, lane);
  w.bar.arrive_and_wait();
  return r;
}
template <class T>
static T slot_as(u64 s) {
  T v;
  memcpy(&v, &s, sizeof(T));
  return v;
}
template <class T>
static T host_shfl(T v, int src) {
  return wave_exchange(v, [&](const u64* s, int) { return slot_as<T>(s[src]); });
}
template <class T>
static T host_shfl_up(T v, int delta) {
  return wave_exchange(v, [&](const u64* s, int lane) { return lane >= delta ? slot_as<T>(s[lane - delta]) : v; });
}
static u64 host_ballot(bool p) {
  return wave_exchange(p ? 1 : 0, [](const u64* s, int) {
    u64 m = 0;
    for (int i = 0; i < 64; ++i) m |= (u64)slot_as<int>(s[i]) << i;
    return m;
  });
}
#define __shfl host_shfl
#define __shfl_up host_shfl_up
#define __ballot host_ballot
#define __popcll __builtin_popcountll

void fuelmi_set_error(const char*, ...) {}

static thread_local unsigned char* g_lds;  // the lane's workgroup's LDS block (kernel.inc: `unsigned char* smem_raw = g_lds;`)

// `blocks` workgroups of `threads` lanes (a multiple of 64); kernel() is the call with its arguments.  The lanes are
// created once and walk the workgroups together, one workgroup after the other.  lds > 0: every workgroup has a heap
// block of its own of that many bytes, filled with 0xA5 like the two guard zones round it; a guard byte that changed
// prints GUARD HIT and returns 9.
template <class K>
static int launch(int blocks, int threads, size_t lds, K kernel) {
  constexpr size_t GUARD = 256;
  std::vector<std::unique_ptr<unsigned char[]>> block(lds ? blocks : 0);
  for (auto& b : block) {
    b.reset(new unsigned char[lds + 2 * GUARD]);
    memset(b.get(), 0xA5, lds + 2 * GUARD);
  }
  std::vector<std::unique_ptr<Barrier>> bars(blocks);
  for (auto& b : bars) b.reset(new Barrier(threads));
  g_bars = bars.data();
  Barrier over(threads);
  std::unique_ptr<WaveBlock[]> waves(new WaveBlock[threads / 64]);
  g_waves = waves.get();
  std::vector<std::thread> th;
  for (int t = 0; t < threads; ++t)
    th.emplace_back([&, t] {
      threadIdx_.x = t, blockDim_.x = threads;
      for (int blk = 0; blk < blocks; ++blk) {
        blockIdx_.x = blk;
        g_lds = lds ? block[blk].get() + GUARD : nullptr;
        kernel();
        bars[blk]->arrive_and_drop();  // a lane that has left the kernel is not waited for at its __syncthreads
        over.arrive_and_wait();        // the workgroup is over: its statics are free for the next one
      }
    });
  for (auto& x : th) x.join();
  for (auto& b : block)
    for (size_t i = 0; i < GUARD; ++i)
      if (b[i] != 0xA5 || b[GUARD + lds + i] != 0xA5) {
        std::printf("GUARD HIT\n");
        return 9;
      }
  return 0;
}

static unsigned long long bits(double v) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  return b;
}
// the next number of a text file, decimal or a hexadecimal float
static double num(std::ifstream& in) {
  std::string s;
  in >> s;
  return strtod(s.c_str(), nullptr);
}

#endif
