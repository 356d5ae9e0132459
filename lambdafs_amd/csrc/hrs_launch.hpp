// Host-side launch geometry shared by the kernel translation units
// (hrs_kernels.hip, hrs_runtime.hip, hrs_batch.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "hrs_internal.hpp"
#include "hrs_window_map.hpp"

namespace hrs {

// note_kernel with the template arguments spelled as rocprofv3 prints them:
// note_kernel_t("bitsliced_pipe_kernel", 1, 12) -> "bitsliced_pipe_kernel<1, 12>".
inline void kname_arg(std::string& s, int v) { s += std::to_string(v); }
inline void kname_arg(std::string& s, bool v) { s += v ? "true" : "false"; }
inline void kname_arg(std::string& s, const char* v) { s += v; }
template <typename... T>
inline void note_kernel_t(const char* base, T... v) {
  std::string s(base);
  if constexpr (sizeof...(T) > 0) {
    const char* sep = "<";
    ((s += sep, kname_arg(s, v), sep = ", "), ...);
    s += '>';
  }
  note_kernel(s.c_str());
}

// The parity size as a template argument: f(std::integral_constant<int, p>)
// for p in [Lo, Hi], hipErrorInvalidValue outside. f returns a hipError_t
// (the launchers) or nothing (host loops: hipSuccess). The call of f stands
// before the recursion, so the kernels it names are instantiated in ascending
// p, the order of the case ladders this replaces.
template <int Lo, int Hi, class F>
inline hipError_t dispatch_p(int p, F&& f) {
  if constexpr (Lo > Hi) {
    return hipErrorInvalidValue;
  } else {
    constexpr std::integral_constant<int, Lo> P{};
    if (p == Lo) {
      if constexpr (std::is_void_v<decltype(f(P))>) {
        f(P);
        return hipSuccess;
      } else {
        return f(P);
      }
    }
    return dispatch_p<Lo + 1, Hi>(p, f);
  }
}

// CU count per device, cached; handles on several host threads may race to
// fill it (same value), hence the relaxed atomics.
inline int device_cus() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  static std::atomic<int> cus_of[64];
  if (dev < 0 || dev >= 64) return 256;
  int cus = cus_of[dev].load(std::memory_order_relaxed);
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cus_of[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

// Window -> wave order of a streaming kernel launch (hrs_device.hpp
// wave_tasks): C >= 1 = block-cyclic chunks of C windows per wave (1 = grid-
// stride), 0 = block range. Each kernel family passes its measured default;
// HRS_TASK_ORDER=<C> overrides every family (A/B runs), read per launch so
// one process can sweep it (tools/bench_order.py).
inline int task_order(int dflt) {
  const char* e = getenv("HRS_TASK_ORDER");
  if (e && *e) {
    const int c = atoi(e);
    if (c >= 0 && c <= 4096) return c;
  }
  return dflt;
}

// Defaults per family: grid-stride throughout (hrs_device.hpp wave_tasks,
// profiles/r04/q/order_sweep.jsonl, r/ and s/order_shapes.jsonl).
constexpr int kOrderStaticEncode = 1;  // encode_static / encode_cauchy / xor
constexpr int kOrderRuntime = 1;       // bitsliced (plain, pipelined, streaming) repairs
constexpr int kOrderBatch = 1;         // heterogeneous repair batches
constexpr int kOrderFusedEncode = 1;   // encode + CRC-32
constexpr int kOrderDecodeCrc = 1;     // repair + CRC-32
constexpr int kOrderCrc = 1;           // CRC-32 windows
constexpr int kOrderScrub = 1;         // scrub windows (not swept: the encode's order)

template <class A>
inline A with_order(A a, int dflt) {
  a.order = task_order(dflt);
  return a;
}

// Window map of the plain static encode and the runtime-matrix kernels
// (hrs_window_map.hpp): the half distance in bytes between a wave task's two
// 1 KiB pieces, 1024 = contiguous windows. Each family passes its measured
// default (tools/bench_split.py, profiles/window_split/NOTES.md);
// HRS_WINDOW_SPLIT=<bytes> overrides both families (A/B runs, tests), read per
// launch like HRS_TASK_ORDER. A value that is not a power of two in
// [1 KiB, 1 MiB] is ignored. Returns log2(bytes / 1 KiB), the kernels' form.
inline int window_split(int dflt_bytes) {
  const char* e = getenv("HRS_WINDOW_SPLIT");
  if (e && *e) {
    const int s = split_of_bytes(atoll(e));
    if (s >= 0) return s;
  }
  return split_of_bytes(dflt_bytes);
}

// Measured (profiles/window_split/): 32 KiB and 64 KiB both run bench.py's
// RS(10,4) 1 MiB x 1,024 encode 11 % and its 1-loss repair 10 % faster than
// contiguous windows; 4, 16, 128 and 256 KiB do nothing. 32 KiB also reaches
// 64 KiB cells (a row shorter than 2H has no strided group) and lost on no
// shape swept, so both families take it without a row-length rule.
constexpr int kSplitStaticEncode = 32768;  // encode_static / encode_cauchy
constexpr int kSplitRuntime = 32768;       // bitsliced (plain, pipelined, streaming) repairs

template <class A>
inline A with_split(A a, int dflt_bytes) {
  a.split = window_split(dflt_bytes);
  return a;
}

// Streaming kernels: a fixed number of resident blocks per CU, grid-striding
// over the tasks. 2 x 256-thread blocks per CU (8 waves, each with a whole
// window's rows in flight) measured fastest for both the static and the
// runtime kernels (tools/kernel_lab.hip sweep, 256..1024 blocks); override
// with HRS_BLOCKS_PER_CU for experiments.
// VALU-bound shapes (the rolled bit loop: 3-4 erasure repairs, wide
// matrices) take 3 blocks per CU: the extra wave per SIMD hides more of the
// math (RS(10,4) 4-erasure decode +13%, profiles/r01/pipe/).
inline int blocks_per_cu(int dflt = 2) {
  static int v = [] {
    const char* e = getenv("HRS_BLOCKS_PER_CU");
    int x = e ? atoi(e) : 0;
    return (x >= 1 && x <= 32) ? x : 0;
  }();
  return v ? v : dflt;
}

// Zero-copy launches (kernels reading and writing pinned host memory across
// the host link, hrs_hostbatch_api.cpp / hrs_hostpath.cpp) cap their grid: the
// link, not the CUs, bounds them, so a capped grid leaves the rest of the chip
// to other work. Set for the calling thread by a GridCap around the launch;
// every launcher sizes its grid through capped_grid (stream_grid, grid_for,
// and the fused / CRC launchers, whose 1,024- or 512-thread blocks take one
// CU each, so the cap in blocks is a cap in CUs there).
inline thread_local unsigned t_grid_cap = 0;

struct GridCap {
  unsigned prev;
  explicit GridCap(unsigned cap) : prev(t_grid_cap) { t_grid_cap = cap; }
  ~GridCap() { t_grid_cap = prev; }
};

inline unsigned capped_grid(uint64_t g) {
  if (t_grid_cap && g > t_grid_cap) g = t_grid_cap;
  return static_cast<unsigned>(g == 0 ? 1 : g);
}

inline unsigned stream_grid(uint64_t ntasks, int per_cu = 2) {
  const uint64_t want = static_cast<uint64_t>(blocks_per_cu(per_cu)) * device_cus();
  const uint64_t needed = (ntasks + kWavesPerBlock - 1) / kWavesPerBlock;
  uint64_t g = needed < want ? needed : want;
  return capped_grid(g);
}

template <typename Kernel>
inline unsigned grid_for(Kernel kernel, uint64_t work_items_per_block, uint64_t ntasks) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlockThreads, 0) != hipSuccess ||
      per_cu <= 0)
    per_cu = 2;
  const uint64_t resident = static_cast<uint64_t>(per_cu) * device_cus();
  const uint64_t needed = (ntasks + work_items_per_block - 1) / work_items_per_block;
  uint64_t g = needed < resident ? needed : resident;
  return capped_grid(g);
}

}  // namespace hrs
