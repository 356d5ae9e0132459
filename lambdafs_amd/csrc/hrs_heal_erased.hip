// Heal with known erasures on gfx950 (include/hrs.h, hrs_heal_erased_dev):
// every stripe of a batch has its own set of lost cells; one pass rebuilds
// them and locates and fixes silent errors in the survivors.
//
// The walk is the scrub's (hrs_scrub.hip): one wave per 2 KiB window, Horner
// over the rows from location n - 1 down to 0 in the bit-sliced domain. An
// erased row is not loaded (a wave-uniform test on the pattern's mask) and
// takes the xtime-only step, so S holds the syndromes of the survivors alone.
// The modified syndromes T (p - e of them) and the erased values v (e of
// them) are both GF(2^8)-linear in S with wave-uniform coefficients
// (ErasePattern::cw, hrs_heal_erased.hpp): one P x P constant multiply of
// sliced planes, tv = M S. A window whose T planes are zero in every lane (one
// ballot) un-slices v and stores the e erased rows: no LDS access, no atomics.
// Any other window un-slices S and tv; the lane that owns a bad column runs
// locator::locate_errata on it, patches the survivors byte by byte as the
// heal does and replaces the column's erased bytes in its registers before
// the row stores, so each byte is stored once, by the lane that owns it.
//
// Each walk has one body (heal_window, heal_one_column; the tail from tv = M S
// on is heal_tail of hrs_heal_erased_device.hpp, shared with the fused CRC
// form) and two kernels that call it: over every stripe of a batch, and over
// the stripes a device list names.
#include <hip/hip_runtime.h>

#include "hrs_device.hpp"
#include "hrs_heal_erased.hpp"
#include "hrs_heal_erased_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_locator.hpp"
#include "hrs_scrub_device.hpp"

namespace hrs {
namespace {

constexpr int kErasedGroup = 8;  // rows of a window in flight per wave; groups are aligned, one mask byte each
constexpr int kHistWords = kScrubHead + kScrubMaxRows;  // per wave

// The block's prologue keeps this unit's own text, not load_field_tables and
// hist_init of hrs_scrub_device.hpp: with those the compiler allocates the
// window kernels' registers differently (heal_erased_kernel<1> 111 -> 96
// VGPRs, <3> 134 -> 112), code the batch calls were not measured with.
__constant__ gf::Tables d_erased_tables = gf::make_tables();

__device__ __forceinline__ void load_tables(uint8_t* s_exp, uint8_t* s_log) {
  for (int i = threadIdx.x; i < 512; i += blockDim.x) s_exp[i] = d_erased_tables.exp[i];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_log[i] = d_erased_tables.log[i];
}

// Every wave's histogram at rest: a report's layout, word 2 is a minimum.
__device__ __forceinline__ void init_hist(uint32_t (&s_hist)[kWavesPerBlock][kHistWords]) {
  for (int i = threadIdx.x; i < kWavesPerBlock * kHistWords; i += blockDim.x) {
    const int e = i % kHistWords;
    s_hist[i / kHistWords][e] = e == 2 ? kScrubNone : 0u;
  }
}

// ------------------------------------------------------ vector kernels

// One window: the 2 KiB at `off` of the rows of `stripe` (base = stripe *
// stride + off), whose pattern the wave holds in pv. pat_index() is the
// pattern's index in the table; it is called for a bad column only.
template <int P, class PatIndex>
__device__ __forceinline__ void heal_window(const HealErasedArgs& ha, const locator::Field& f, uint32_t pv,
                                            uint64_t stripe, uint64_t off, uint64_t base, int lane, uint32_t* hist,
                                            int nwords, PatIndex&& pat_index) {
  const ScrubArgs& a = ha.s;
  const int spare = static_cast<int>(pattern_word(pv, kPatSpare));
  uint32_t acc[P][8];
#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[i][q] = 0u;
  for (int l0 = (a.n - 1) & ~(kErasedGroup - 1); l0 >= 0; l0 -= kErasedGroup) {
    // locations l0 + 7 .. l0; bit g of `gone`: l0 + g is erased
    const uint32_t gone = (pattern_word(pv, kPatMask + (l0 >> 5)) >> (l0 & 31)) & ((1u << kErasedGroup) - 1u);
    uint32_t w[kErasedGroup][8];
    // Every slot loads, in one straight run, so that the loads of a group are
    // in flight together (a load behind a branch of its own waits for the
    // ones before it). A slot with no survivor row (erased, or past n - 1)
    // reads one 16-byte piece of a survivor's window in every lane instead:
    // one cache line, never an erased cell, and the result is not used.
#pragma unroll
    for (int g = kErasedGroup - 1; g >= 0; --g) {
      const bool take = l0 + g < a.n && !((gone >> g) & 1u);
      const uint8_t* p = a.rows[take ? l0 + g : spare] + base;
      const uint32_t lo = take ? lane * 16u : 0u, hi = take ? 1024u : 0u;
      const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + lo));
      const u32x4 y = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + lo + hi));
      w[g][0] = x[0]; w[g][1] = x[1]; w[g][2] = x[2]; w[g][3] = x[3];
      w[g][4] = y[0]; w[g][5] = y[1]; w[g][6] = y[2]; w[g][7] = y[3];
    }
#pragma unroll
    for (int g = kErasedGroup - 1; g >= 0; --g)
      if (l0 + g < a.n) {
        const bool live = !((gone >> g) & 1u);
        if (live) bitslice(w[g]);
#pragma unroll
        for (int i = 0; i < P; ++i) {
#pragma unroll
          for (int r = 0; r < i; ++r) xtime(acc[i]);
          if (live) {
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[i][q] ^= w[g][q];
          }
        }
      }
  }
  const bool dirty = heal_tail<P>(f, a.n, a.rows, ha.pats, pv, stripe * a.stride, static_cast<uint32_t>(off), lane,
                                  hist, acc, pat_index, [&](int l, const uint32_t(&row)[8], bool) {
                                    store_row(const_cast<uint8_t*>(a.rows[l]) + base, lane, row);
                                  });
  // this window's counts to its stripe
  if (dirty) hist_flush(hist, a.reports + stripe * a.report_stride, nwords, lane);
}

template <int P>
__global__ void __launch_bounds__(kBlockThreads) heal_erased_kernel(const HealErasedArgs ha) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  __shared__ uint32_t s_hist[kWavesPerBlock][kHistWords];
  const ScrubArgs& a = ha.s;
  load_tables(s_exp, s_log);
  init_hist(s_hist);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const int lane = threadIdx.x & 63;
  uint32_t* hist = s_hist[threadIdx.x >> 6];
  const int nwords = kScrubHead + a.n;
  const WaveTasks wt = wave_tasks(a.ntasks, a.order);
  // Two loads lead to a window's pattern (its stripe's index, then the table
  // entry); both run ahead of the windows so that neither is waited for: while
  // window j runs, the entry of window j + 1 and the index of window j + 2
  // are in flight. One 64-bit division per window, as in the scrub.
  uint64_t stripe_cur = 0, stripe_next = 0;
  uint32_t pv_next = 0u;
  int32_t pi_next = 0;
  if (wt.at(0) < wt.end) {
    stripe_cur = wt.at(0) / a.nwin;
    pv_next = load_pattern(ha.pats, ha.pat[stripe_cur], lane);
  }
  if (wt.at(1) < wt.end) {
    stripe_next = wt.at(1) / a.nwin;
    pi_next = ha.pat[stripe_next];
  }
  for (uint32_t j = 0; j < 0xFFFFFFFFu; ++j) {
    const uint64_t t = wt.at(j);
    if (t >= wt.end) break;
    const uint64_t stripe = stripe_cur;
    const uint64_t off = (t - stripe * a.nwin) * kWindowBytes;
    const uint64_t base = stripe * a.stride + off;
    const uint32_t pv = pv_next;
    stripe_cur = stripe_next;
    if (wt.at(j + 1) < wt.end) pv_next = load_pattern(ha.pats, pi_next, lane);
    if (wt.at(j + 2) < wt.end) {
      stripe_next = wt.at(j + 2) / a.nwin;
      pi_next = ha.pat[stripe_next];
    }
    heal_window<P>(ha, f, pv, stripe, off, base, lane, hist, nwords, [&] { return ha.pat[stripe]; });
  }
}

// ------------------------------------------- byte-granular kernels (any alignment)

// One column per lane, tables in LDS: rows or strides that are not 16-byte
// aligned, the row tail (len % 2 KiB) and kernel mode 2. Counts go straight
// into the report. This is the column at rows[l][at] of `stripe`, pattern pt.
template <int P>
__device__ __forceinline__ void heal_one_column(const locator::Field& f, const ScrubArgs& a, const ErasePattern& pt,
                                                uint64_t stripe, uint64_t col, uint64_t at) {
  uint8_t s[P];
#pragma unroll
  for (int i = 0; i < P; ++i) s[i] = 0;
  for (int l = a.n - 1; l >= 0; --l) {
    const bool gone = (pt.mask[l >> 5] >> (l & 31)) & 1u;
    locator::horner_step<P>(f, s, gone ? uint8_t{0} : a.rows[l][at]);
  }
  uint8_t v[locator::kMaxErased];
  heal_column<P>(f, a.n, s, pt, static_cast<uint32_t>(col), a.reports + stripe * a.report_stride, a.rows, at, v);
  const int e = pt.e;
  for (int m = 0; m < e; ++m) const_cast<uint8_t*>(a.rows[pt.loc[m]])[at] = v[m];
}

// Task idx = stripe * (len - col0) + (column - col0).
template <int P>
__global__ void __launch_bounds__(kBlockThreads) heal_erased_bytewise_kernel(const HealErasedArgs ha) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  const ScrubArgs& a = ha.s;
  load_tables(s_exp, s_log);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const uint64_t wlen = a.len - a.col0;
  const uint64_t nthreads = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < a.ntasks;
       idx += nthreads) {
    const uint64_t stripe = idx / wlen;
    const uint64_t col = a.col0 + (idx - stripe * wlen);
    heal_one_column<P>(f, a, ha.pats[ha.pat[stripe]], stripe, col, stripe * a.stride + col);
  }
}

template <int P>
hipError_t launch_windows(const HealErasedArgs& a, hipStream_t s) {
  auto kern = heal_erased_kernel<P>;
  note_kernel_t("heal_erased_kernel", P);
  HealErasedArgs b = a;
  b.s.order = task_order(kOrderScrub);
  hipLaunchKernelGGL(kern, dim3(stream_grid(a.s.ntasks)), dim3(kBlockThreads), 0, s, b);
  return hipGetLastError();
}

template <int P>
hipError_t launch_columns(const HealErasedArgs& a, hipStream_t s) {
  auto kern = heal_erased_bytewise_kernel<P>;
  note_kernel_t("heal_erased_bytewise_kernel", P);
  const unsigned g = grid_for(kern, kBlockThreads, a.s.ntasks);
  hipLaunchKernelGGL(kern, dim3(g), dim3(kBlockThreads), 0, s, a);
  return hipGetLastError();
}

// ------------------------------------------------------ the listed form
//
// Checked repair (hrs_repair_checked_dev) runs the two walks above over the
// stripes a device list names (HealListedArgs, hrs_heal_erased.hpp). The
// kernels are instantiations of their own, not a template flag on the two
// above: with the flag the compiler allocated the existing kernels' registers
// differently (111 -> 96 VGPRs at P = 1, another occupancy at P = 1 and 3),
// and the batch calls keep the code they were measured with. What differs is
// the prologue: the task range is count * nwin, the count read from device
// memory at kernel entry and clamped to nstripes; a task's stripe is the
// list's entry, which is also its pattern's index; an entry that is no stripe
// of the batch is skipped and never indexed with; a block with no task leaves
// before it loads anything.

// The stripe at a place of the list; the caller tests it against nstripes
// before it indexes anything with it.
__device__ __forceinline__ uint64_t listed_stripe(const HealListedArgs& a, uint64_t place) { return a.list[1 + place]; }

// A listed stripe's table entry is its own; an entry that is no stripe reads
// entry 0 and its window is skipped.
__device__ __forceinline__ int32_t listed_pattern(const HealListedArgs& a, uint64_t stripe) {
  return stripe < a.nstripes ? static_cast<int32_t>(stripe) : 0;
}

template <int P>
__global__ void __launch_bounds__(kBlockThreads) heal_listed_kernel(const HealListedArgs la) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  __shared__ uint32_t s_hist[kWavesPerBlock][kHistWords];
  const HealErasedArgs& ha = la.h;
  const ScrubArgs& a = ha.s;
  // the task range comes from device memory (a.ntasks is only the bound the
  // grid was sized for); a block whose first wave has no window leaves before
  // it loads anything (block-uniform)
  const uint64_t ntasks = static_cast<uint64_t>(listed_count(la.list, la.nstripes)) * a.nwin;
  {
    const WaveTasks w0 = wave_tasks(ntasks, a.order);
    if (w0.t0 - (threadIdx.x >> 6) >= w0.end) return;
  }
  load_tables(s_exp, s_log);
  init_hist(s_hist);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const int lane = threadIdx.x & 63;
  uint32_t* hist = s_hist[threadIdx.x >> 6];
  const int nwords = kScrubHead + a.n;
  const WaveTasks wt = wave_tasks(ntasks, a.order);
  // The pattern's prefetch chain of heal_erased_kernel; here the first load is
  // the list's entry, which is the index.
  uint64_t pos_cur = 0, pos_next = 0, stripe_cur = 0, stripe_next = 0;
  uint32_t pv_next = 0u;
  int32_t pi_next = 0;
  if (wt.at(0) < wt.end) {
    pos_cur = wt.at(0) / a.nwin;
    stripe_cur = listed_stripe(la, pos_cur);
    pv_next = load_pattern(ha.pats, listed_pattern(la, stripe_cur), lane);
  }
  if (wt.at(1) < wt.end) {
    pos_next = wt.at(1) / a.nwin;
    stripe_next = listed_stripe(la, pos_next);
    pi_next = listed_pattern(la, stripe_next);
  }
  for (uint32_t j = 0; j < 0xFFFFFFFFu; ++j) {
    const uint64_t t = wt.at(j);
    if (t >= wt.end) break;
    const uint64_t stripe = stripe_cur;
    const uint64_t off = (t - pos_cur * a.nwin) * kWindowBytes;
    const uint64_t base = stripe * a.stride + off;
    const uint32_t pv = pv_next;
    pos_cur = pos_next;
    stripe_cur = stripe_next;
    if (wt.at(j + 1) < wt.end) pv_next = load_pattern(ha.pats, pi_next, lane);
    if (wt.at(j + 2) < wt.end) {
      pos_next = wt.at(j + 2) / a.nwin;
      stripe_next = listed_stripe(la, pos_next);
      pi_next = listed_pattern(la, stripe_next);
    }
    if (stripe >= la.nstripes) continue;  // no stripe of this batch: nothing is indexed with it
    heal_window<P>(ha, f, pv, stripe, off, base, lane, hist, nwords, [&] { return listed_pattern(la, stripe); });
  }
}

template <int P>
__global__ void __launch_bounds__(kBlockThreads) heal_listed_bytewise_kernel(const HealListedArgs la) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  const HealErasedArgs& ha = la.h;
  const ScrubArgs& a = ha.s;
  const uint64_t wlen = a.len - a.col0;
  const uint64_t ntasks = static_cast<uint64_t>(listed_count(la.list, la.nstripes)) * wlen;
  if (static_cast<uint64_t>(blockIdx.x) * blockDim.x >= ntasks) return;  // block-uniform, before any load
  load_tables(s_exp, s_log);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const uint64_t nthreads = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < ntasks; idx += nthreads) {
    const uint64_t pos = idx / wlen;
    const uint64_t stripe = listed_stripe(la, pos);
    if (stripe >= la.nstripes) continue;  // no stripe of this batch: nothing is indexed with it
    const uint64_t col = a.col0 + (idx - pos * wlen);
    heal_one_column<P>(f, a, ha.pats[listed_pattern(la, stripe)], stripe, col, stripe * a.stride + col);
  }
}

// The listed launches: the grid is sized for the bound a.h.s.ntasks.
template <int P>
hipError_t launch_listed_windows(const HealListedArgs& a, hipStream_t s) {
  auto kern = heal_listed_kernel<P>;
  note_kernel_t("heal_listed_kernel", P);
  HealListedArgs b = a;
  b.h.s.order = task_order(kOrderScrub);
  hipLaunchKernelGGL(kern, dim3(stream_grid(a.h.s.ntasks)), dim3(kBlockThreads), 0, s, b);
  return hipGetLastError();
}

template <int P>
hipError_t launch_listed_columns(const HealListedArgs& a, hipStream_t s) {
  auto kern = heal_listed_bytewise_kernel<P>;
  note_kernel_t("heal_listed_bytewise_kernel", P);
  const unsigned g = grid_for(kern, kBlockThreads, a.h.s.ntasks);
  hipLaunchKernelGGL(kern, dim3(g), dim3(kBlockThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_heal_erased(const HealErasedArgs& a, hipStream_t s) {
  return dispatch_p<1, 8>(a.s.p, [&](auto P) { return launch_windows<P>(a, s); });
}

hipError_t launch_heal_erased_bytewise(const HealErasedArgs& a, hipStream_t s) {
  return dispatch_p<1, 8>(a.s.p, [&](auto P) { return launch_columns<P>(a, s); });
}

hipError_t launch_heal_listed(const HealListedArgs& a, hipStream_t s) {
  return dispatch_p<1, 8>(a.h.s.p, [&](auto P) { return launch_listed_windows<P>(a, s); });
}

hipError_t launch_heal_listed_bytewise(const HealListedArgs& a, hipStream_t s) {
  return dispatch_p<1, 8>(a.h.s.p, [&](auto P) { return launch_listed_columns<P>(a, s); });
}

}  // namespace hrs
