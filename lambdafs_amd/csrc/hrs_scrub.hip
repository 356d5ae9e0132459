// Stripe scrubbing on gfx950: ReedSolomonCode.computeErrorLocations
// (ReedSolomonCode.java:243-287) over every byte column of every stripe of a
// batch, aggregated into one report per stripe (include/hrs.h, hrs_scrub_dev).
//
// A scrub reads all n rows and writes almost nothing, so it is bound by HBM
// reads like the encode. The syndromes S_i = sum_l alpha^(i l) d_l need no
// matrix: Horner over the rows from location n - 1 down to 0,
//     acc_i <- alpha^i acc_i + d_l,
// is i relabel-plus-3-XOR steps (xtime) per row in the bit-sliced domain,
// about 3 P (P - 1) / 2 + 8 P VALU ops per row per lane beside the slice.
// A window whose P x 8 syndrome planes are all zero in every lane (one OR
// tree, one ballot) is clean: the wave moves on with no un-slice, no LDS
// access and no store. Only a window with a nonzero syndrome un-slices them
// and runs the shared locator (hrs_locator.hpp) on the lane's bad columns.
//
// Every report word is a count or a minimum, added with atomics, so the
// result does not depend on how the windows were scheduled.
//
// This file holds the window loop, the byte-granular loop and the launchers.
// The Horner step, the walk over a dirty window's columns, the report rule of
// one bad column (count_column -> account_column), the per-wave histogram and
// the field tables are hrs_scrub_device.hpp's, shared with hrs_scrub_crc.hip.
#include <hip/hip_runtime.h>

#include "hrs_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_locator.hpp"
#include "hrs_scrub_device.hpp"

namespace hrs {
namespace {

constexpr int kScrubGroup = 8;  // rows of a window in flight per wave (8 x 2 KiB)

// ------------------------------------------------------ vector kernel

// Heal = false is the scrub as it always was (hrs_last_kernel "scrub_kernel<P>").
// Heal = true adds the write-back of the resolved columns (hrs_heal_dev,
// "heal_kernel<P>"): the clean-window path is the same code, the stores sit
// behind the ballot in count_column.
template <int P, bool Heal = false>
__global__ void __launch_bounds__(kBlockThreads) scrub_kernel(const ScrubArgs a) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  __shared__ uint32_t s_hist[kWavesPerBlock][kScrubHead + kScrubMaxRows];
  load_field_tables(s_exp, s_log, blockDim.x);
  const int nwords = kScrubHead + a.n;
  hist_init(&s_hist[0][0], kScrubHead + kScrubMaxRows, kWavesPerBlock);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const int lane = threadIdx.x & 63;
  uint32_t* hist = s_hist[threadIdx.x >> 6];
  const WaveTasks wt = wave_tasks(a.ntasks, a.order);
  for (uint32_t j = 0; j < 0xFFFFFFFFu; ++j) {
    const uint64_t t = wt.at(j);
    if (t >= wt.end) break;
    const uint64_t stripe = t / a.nwin;
    const uint64_t off = (t - stripe * a.nwin) * kWindowBytes;
    const uint64_t base = stripe * a.stride + off;
    uint32_t acc[P][8];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[i][q] = 0u;
    for (int l0 = a.n; l0 > 0; l0 -= kScrubGroup) {
      uint32_t w[kScrubGroup][8];
#pragma unroll
      for (int g = 0; g < kScrubGroup; ++g)
        if (l0 - 1 - g >= 0) load_row(a.rows[l0 - 1 - g] + base, lane, w[g]);
#pragma unroll
      for (int g = 0; g < kScrubGroup; ++g)
        if (l0 - 1 - g >= 0) {
          bitslice(w[g]);
          horner_sliced<P>(acc, w[g]);
        }
    }
    uint32_t any = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) any |= acc[i][q];
    if (__ballot(any != 0u) == 0ull) continue;  // clean window (wave-uniform)

    // slow path: un-slice the syndromes and run the locator on the lane's bad columns
#pragma unroll
    for (int i = 0; i < P; ++i) bitslice(acc[i]);
    if (any != 0u) {
      auto column = [&](const uint8_t(&s)[P], uint32_t col, int, int) {
        count_column<P, Heal>(f, a.n, s, col, hist, a.rows, stripe * a.stride + col);
      };
      for_each_bad_column<P>(acc, static_cast<uint32_t>(off), lane, column);
    }
    hist_flush(hist, a.reports + stripe * a.report_stride, nwords, lane);
  }
}

// ------------------------------------------- byte-granular kernel (any alignment)

// One column per lane, tables in LDS: rows or strides that are not 16-byte
// aligned, the row tail (len % 2 KiB) and kernel mode 2. Task idx = stripe *
// (len - col0) + (column - col0). Counts go straight into the report.
template <int P, bool Heal = false>
__global__ void __launch_bounds__(kBlockThreads) scrub_bytewise_kernel(const ScrubArgs a) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  load_field_tables(s_exp, s_log, blockDim.x);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const uint64_t nthreads = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < a.ntasks;
       idx += nthreads) {
    const BytewiseTask t = bytewise_task(a, idx);
    uint8_t s[P];
    bytewise_syndromes<P>(f, a, t.at, s);
    uint32_t nz = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i) nz |= s[i];
    if (nz == 0u) continue;
    count_column<P, Heal>(f, a.n, s, static_cast<uint32_t>(t.col), a.reports + t.stripe * a.report_stride, a.rows,
                          t.at);
  }
}

// Empty reports: zeros, and 0xFFFFFFFF in the first-bad-column word.
__global__ void __launch_bounds__(kBlockThreads) scrub_init_kernel(uint32_t* reports, uint64_t report_stride,
                                                                   uint32_t nwords, uint64_t total) {
  const uint64_t nthreads = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total; idx += nthreads) {
    const uint64_t stripe = idx / nwords;
    const uint32_t e = static_cast<uint32_t>(idx - stripe * nwords);
    reports[stripe * report_stride + e] = e == 2 ? kScrubNone : 0u;
  }
}

template <int P, bool Heal>
hipError_t launch_windows(const ScrubArgs& a, hipStream_t s) {
  auto kern = scrub_kernel<P, Heal>;
  note_kernel_t(Heal ? "heal_kernel" : "scrub_kernel", P);
  hipLaunchKernelGGL(kern, dim3(stream_grid(a.ntasks)), dim3(kBlockThreads), 0, s, with_order(a, kOrderScrub));
  return hipGetLastError();
}

template <int P, bool Heal>
hipError_t launch_columns(const ScrubArgs& a, hipStream_t s) {
  auto kern = scrub_bytewise_kernel<P, Heal>;
  note_kernel_t(Heal ? "heal_bytewise_kernel" : "scrub_bytewise_kernel", P);
  const unsigned g = grid_for(kern, kBlockThreads, a.ntasks);
  hipLaunchKernelGGL(kern, dim3(g), dim3(kBlockThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_scrub_init(uint32_t* reports, uint64_t report_stride, int n, uint64_t nstripes, hipStream_t s) {
  const uint32_t nwords = static_cast<uint32_t>(kScrubHead + n);
  const uint64_t total = nstripes * nwords;
  const unsigned g = grid_for(scrub_init_kernel, kBlockThreads, total);
  hipLaunchKernelGGL(scrub_init_kernel, dim3(g), dim3(kBlockThreads), 0, s, reports, report_stride, nwords, total);
  return hipGetLastError();
}

hipError_t launch_scrub(const ScrubArgs& a, hipStream_t s) {
  return dispatch_p<1, 8>(a.p, [&](auto P) { return launch_windows<P, false>(a, s); });
}

hipError_t launch_scrub_bytewise(const ScrubArgs& a, hipStream_t s) {
  return dispatch_p<1, 8>(a.p, [&](auto P) { return launch_columns<P, false>(a, s); });
}

hipError_t launch_heal(const ScrubArgs& a, hipStream_t s) {
  return dispatch_p<1, 8>(a.p, [&](auto P) { return launch_windows<P, true>(a, s); });
}

hipError_t launch_heal_bytewise(const ScrubArgs& a, hipStream_t s) {
  return dispatch_p<1, 8>(a.p, [&](auto P) { return launch_columns<P, true>(a, s); });
}

}  // namespace hrs
