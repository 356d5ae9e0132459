// Checked repair on gfx950 (include/hrs.h, hrs_repair_checked_dev): the
// kernels between and after its two passes. Pass 1 is the scrub + CRC call as
// it is; pass 2 is the listed form of the heal with known erasures
// (hrs_heal_erased.hip). Here:
//
//  - repair_plan_kernel: one thread per stripe reads pass 1's report and CRCs
//    and the stored checksums, applies steps 1-3 of the rule
//    (hrs_repair_rule.hpp), writes the verdict and the erased_out row, and for
//    a stripe that goes on builds its ErasePattern in the table (the shared
//    fill_pattern, its working room in LDS), empties its report for pass 2 and
//    appends it to the list: one atomic per wave (ballot, the leader adds the
//    count, every listed lane takes its rank).
//  - repair_crc_window_kernel: the 32 KiB window walk of crc_window_kernel
//    (crc_window_raw, hrs_device.hpp) over the cells of the listed stripes, as
//    pass 2 left them.
//  - repair_fold_verdict_kernel: one wave per listed stripe folds its cells'
//    window CRCs, overwrites the stripe's crc_out words and applies step 6.
//
// The task ranges of the last two, like pass 2's, come from device memory:
// the count is clamped to nstripes, an entry >= nstripes is skipped and never
// indexed with, and the host zeroes the count on the stream before every call.
// No order of the list shows in any output: the raw words are private to a
// place in the list, everything else is addressed by the stripe.
#include <hip/hip_runtime.h>

#include "hrs_device.hpp"
#include "hrs_heal_erased_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_repair.hpp"
#include "hrs_repair_rule.hpp"
#include "hrs_scrub_device.hpp"

namespace hrs {
namespace {

constexpr int kPlanThreads = 64;  // one wave: PatternWork per thread in LDS (12 KiB)

__global__ void __launch_bounds__(kPlanThreads) repair_plan_kernel(const RepairPlanArgs a) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  __shared__ repair::PatternWork s_work[kPlanThreads];
  load_field_tables(s_exp, s_log, kPlanThreads);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const int lane = threadIdx.x;
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * kPlanThreads + lane;
  const bool valid = s < a.nstripes;
  bool listed = false;
  if (valid) {
    uint32_t* rep = a.reports + s * a.report_stride;
    const uint32_t* crc = a.crcs + s * a.n;
    const uint32_t* stored = a.stored + s * a.n;
    int nd = 0, nb = 0;
    for (int l = 0; l < a.n; ++l) {
      nd += repair::doubted(crc[l], stored[l]) ? 1 : 0;
      nb += repair::suspected(crc[l], stored[l], rep[kScrubHead + l], a.flags) ? 1 : 0;
    }
    const uint32_t verdict = repair::plan_verdict(nd, nb, a.p, rep[0], rep[1]);
    listed = verdict == repair::kListed;
    // a listed stripe's verdict is pass 2's to give; until then it has failed
    a.verdicts[s] = listed ? static_cast<uint32_t>(repair::kFailed) : verdict;
    if (a.erased_out)
      for (int m = 0; m < a.p; ++m) a.erased_out[s * a.p + m] = -1;
    if (listed) {
      ErasePattern& pt = a.pats[s];
      uint32_t* words = reinterpret_cast<uint32_t*>(&pt);
      for (int i = 0; i < static_cast<int>(sizeof(ErasePattern) / 4); ++i) words[i] = 0u;
      int e = 0;
      for (int l = 0; l < a.n; ++l)
        if (repair::suspected(crc[l], stored[l], rep[kScrubHead + l], a.flags) && e < a.p) {  // nb <= p: all of B
          pt.loc[e] = static_cast<uint8_t>(l);
          if (a.erased_out) a.erased_out[s * a.p + e] = l;
          ++e;
        }
      pt.e = e;
      repair::fill_pattern(f, a.p, pt, s_work[lane]);
      for (int w = 0; w < kScrubHead + a.n; ++w) rep[w] = w == 2 ? kScrubNone : 0u;
    }
  }
  // one atomic per wave: the leader reserves the wave's places
  const uint64_t mask = __ballot(listed);
  if (mask != 0ull) {
    const int leader = __ffsll(static_cast<unsigned long long>(mask)) - 1;
    uint32_t base = 0u;
    if (lane == leader) base = atomicAdd(&a.list[0], static_cast<uint32_t>(__popcll(mask)));
    base = static_cast<uint32_t>(__shfl(static_cast<int>(base), leader, 64));
    if (listed) {
      const uint32_t place = base + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
      if (place < a.nstripes) a.list[1 + place] = static_cast<uint32_t>(s);  // always true: each stripe lists itself once
    }
  }
}

// ---- CRCs of the listed stripes

// crc_window_kernel's tasks (hrs_crc.hip) with the stripe taken from the list: task
// t = ((i * n + l) * wpr + w) for window w of cell l of the i-th listed stripe.
template <bool ALIGNED>
__global__ void __launch_bounds__(kCrcBlockThreads) repair_crc_window_kernel(const RepairCrcArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint64_t nwin = a.len / kCrcWindow;
  const uint64_t tail = a.len - nwin * kCrcWindow;
  const uint64_t wpr = nwin + (tail ? 1 : 0);
  const uint64_t ntasks = static_cast<uint64_t>(listed_count(a.list, a.nstripes)) * a.n * wpr;
  const WaveTasks wt = wave_tasks(ntasks, a.order);
  if (wt.t0 - (threadIdx.x >> 6) >= wt.end) return;  // block-uniform: nothing listed for this block
  for (int i = threadIdx.x; i < kCrcLdsWordsA; i += blockDim.x) lds[i] = a.tables[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const SliceTab slices = slice_tab(lane);
  const uint32_t* zchunk = lds + kCrcSliceWords;
  const uint32_t* tree = zchunk + 1024;
  for (uint32_t j = 0; j < 0xFFFFFFFFu; ++j) {
    const uint64_t t = wt.at(j);
    if (t >= wt.end) break;
    const uint64_t sr = t / wpr;
    const uint64_t w = t - sr * wpr;
    const uint64_t place = sr / a.n;
    const int row = static_cast<int>(sr - place * a.n);
    const uint64_t stripe = a.list[1 + place];
    if (stripe >= a.nstripes) continue;  // no stripe of this batch: nothing is indexed with it
    const uint8_t* base = a.rows[row] + stripe * a.stride;
    const uint32_t c = crc_window_raw<ALIGNED>(base, w, nwin, a.len, lane, slices, zchunk, tree);
    if (lane == 0) a.raw[sr * wpr + w] = c;
  }
}

// The fold of crc_fold_kernel (fold_row, hrs_device.hpp), one wave per listed
// stripe over its n cells in turn; lane 0 then knows F and F ∩ D of the whole
// stripe.
__global__ void __launch_bounds__(256) repair_fold_verdict_kernel(const RepairFoldArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint32_t count = listed_count(a.list, a.nstripes);
  if (blockIdx.x * (blockDim.x >> 6) >= count) return;  // block-uniform: nothing listed for this block
  for (int i = threadIdx.x; i < kCrcLdsWordsB; i += blockDim.x) lds[i] = a.tables[i];
  __syncthreads();
  const uint32_t* zw = lds;                // Z_window
  const uint32_t* ztree = lds + 1024;      // Z_{window*G*2^t}, t = 0..5
  const uint32_t* ztail = lds + 7 * 1024;  // Z_tail
  const uint32_t* zlen = lds + 8 * 1024;   // Z_len
  const int lane = threadIdx.x & 63;
  const uint64_t wpr = a.nwin + (a.tail ? 1 : 0);
  const uint64_t pad = static_cast<uint64_t>(a.G) * 64 - a.nwin;
  const uint32_t nwaves = gridDim.x * (blockDim.x / 64);
  for (uint32_t place = wave_id_in_grid(); place < count; place += nwaves) {
    const uint64_t stripe = a.list[1 + place];
    if (stripe >= a.nstripes) continue;  // no stripe of this batch: nothing is indexed with it
    bool any_f = false, any_fd = false;
    for (int l = 0; l < a.n; ++l) {
      const uint32_t* raw = a.raw + (static_cast<uint64_t>(place) * a.n + l) * wpr;
      const uint32_t c = fold_row(raw, a.nwin, a.G, pad, a.tail, zw, ztree, ztail, lane);
      if (lane == 0) {
        const uint32_t now = zmul(zlen, 0xFFFFFFFFu) ^ c ^ 0xFFFFFFFFu;
        const uint64_t at = stripe * a.n + l;
        const uint32_t stored = a.stored[at];
        const bool in_f = repair::doubted(now, stored);
        any_f |= in_f;
        any_fd |= in_f && repair::doubted(a.crc_out[at], stored);  // crc_out still holds pass 1's value
        a.crc_out[at] = now;
      }
    }
    if (lane == 0) a.verdicts[stripe] = repair::final_verdict(any_f, any_fd, a.reports[stripe * a.report_stride + 1]);
  }
}

}  // namespace

hipError_t launch_repair_plan(const RepairPlanArgs& a, hipStream_t s) {
  const unsigned g = (a.nstripes + kPlanThreads - 1) / kPlanThreads;
  hipLaunchKernelGGL(repair_plan_kernel, dim3(g ? g : 1), dim3(kPlanThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_repair_crc_windows(const RepairCrcArgs& a, bool aligned, int cus, hipStream_t s) {
  // one 1024-thread block per CU (the 156 KiB table image fills its LDS), sized for every stripe listed
  const uint64_t wpr = (a.len + kCrcWindow - 1) / kCrcWindow;
  const uint64_t waves = static_cast<uint64_t>(a.nstripes) * a.n * wpr;
  const uint64_t per_block = kCrcBlockThreads / 64;
  uint64_t g = (waves + per_block - 1) / per_block;
  if (g > static_cast<uint64_t>(cus)) g = cus;
  g = capped_grid(g);
  const size_t shm = static_cast<size_t>(kCrcLdsWordsA) * 4;
  auto k = aligned ? repair_crc_window_kernel<true> : repair_crc_window_kernel<false>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(shm));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3(static_cast<unsigned>(g)), dim3(kCrcBlockThreads), shm, s, with_order(a, kOrderCrc));
  return hipGetLastError();
}

hipError_t launch_repair_fold_verdict(const RepairFoldArgs& a, int cus, hipStream_t s) {
  uint64_t g = (static_cast<uint64_t>(a.nstripes) + 3) / 4;
  const uint64_t cap = static_cast<uint64_t>(cus) * kCrcFoldBlocksPerCU;
  if (g > cap) g = cap;
  const size_t shm = static_cast<size_t>(kCrcLdsWordsB) * 4;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(repair_fold_verdict_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(shm));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(repair_fold_verdict_kernel, dim3(static_cast<unsigned>(g ? g : 1)), dim3(256), shm, s, a);
  return hipGetLastError();
}

}  // namespace hrs
