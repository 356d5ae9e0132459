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
#include <hip/hip_runtime.h>

#include "hrs_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_locator.hpp"

namespace hrs {
namespace {

__constant__ gf::Tables d_scrub_tables = gf::make_tables();

constexpr int kScrubGroup = 8;  // rows of a window in flight per wave (8 x 2 KiB)

__device__ __forceinline__ void load_tables(uint8_t* s_exp, uint8_t* s_log) {
  for (int i = threadIdx.x; i < 512; i += blockDim.x) s_exp[i] = d_scrub_tables.exp[i];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_log[i] = d_scrub_tables.log[i];
}

// One bad column (syndromes s, not all zero) into the counters at h: a
// per-wave LDS histogram (vector kernel) or the stripe's report itself.
// Heal: a resolved column is also written back, data[loc[j]] ^= err[j] at
// rows[loc[j]] + at (ReedSolomonCode.java:281-285), one byte load, XOR and
// byte store per nonzero error value, counted in word 3. An unresolved column
// is not touched (the Java returns false after writing it; include/hrs.h).
// The column belongs to this lane alone, so the stores race with nothing.
template <int P, bool Heal>
__device__ __forceinline__ void count_column(const locator::Field& f, int n, const uint8_t (&s)[P], uint32_t col,
                                             uint32_t* h, const uint8_t* const* rows, uint64_t at) {
  int nloc = 0;
  uint8_t loc[locator::kMaxErrors], err[locator::kMaxErrors];
  const bool resolved = locator::locate(f, n, P, s, &nloc, loc, err);
  atomicAdd(&h[0], 1u);
  atomicMin(&h[2], col);
  if (!resolved) {
    atomicAdd(&h[1], 1u);
  } else {
    for (int j = 0; j < nloc; ++j) atomicAdd(&h[kScrubHead + loc[j]], 1u);
    if constexpr (Heal) {
      uint32_t patched = 0u;
      for (int j = 0; j < nloc; ++j)
        if (err[j] != 0) {
          uint8_t* q = const_cast<uint8_t*>(rows[loc[j]]) + at;
          *q = static_cast<uint8_t>(*q ^ err[j]);
          ++patched;
        }
      if (patched != 0u) atomicAdd(&h[kScrubPatched], patched);
    }
  }
}

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
  load_tables(s_exp, s_log);
  const int nwords = kScrubHead + a.n;
  for (int i = threadIdx.x; i < kWavesPerBlock * (kScrubHead + kScrubMaxRows); i += blockDim.x) {
    const int e = i % (kScrubHead + kScrubMaxRows);
    s_hist[i / (kScrubHead + kScrubMaxRows)][e] = e == 2 ? kScrubNone : 0u;
  }
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
#pragma unroll
          for (int i = 0; i < P; ++i) {
#pragma unroll
            for (int r = 0; r < i; ++r) xtime(acc[i]);
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[i][q] ^= w[g][q];
          }
        }
    }
    uint32_t any = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) any |= acc[i][q];
    if (__ballot(any != 0u) == 0ull) continue;  // clean window (wave-uniform)

    // slow path: the lane's 32 columns are bytes 0..3 of words 0..7 of the
    // un-sliced syndromes; word x covers window bytes (x >> 2) * 1024 + lane * 16 + (x & 3) * 4
#pragma unroll
    for (int i = 0; i < P; ++i) bitslice(acc[i]);
    if (any != 0u) {
#pragma unroll 1
      for (int x = 0; x < 8; ++x) {
        uint32_t cur[P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
          uint32_t v = acc[i][0];
#pragma unroll
          for (int q = 1; q < 8; ++q) v = (x == q) ? acc[i][q] : v;  // selects, so acc stays in registers
          cur[i] = v;
        }
        uint32_t anyw = 0u;
#pragma unroll
        for (int i = 0; i < P; ++i) anyw |= cur[i];
        if (anyw == 0u) continue;
#pragma unroll 1
        for (int b = 0; b < 4; ++b) {
          uint8_t s[P];
          uint32_t nz = 0u;
#pragma unroll
          for (int i = 0; i < P; ++i) {
            s[i] = static_cast<uint8_t>(cur[i] >> (8 * b));
            nz |= s[i];
          }
          if (nz == 0u) continue;
          const uint32_t col = static_cast<uint32_t>(off) + (x >> 2) * 1024u + lane * 16u + (x & 3) * 4u + b;
          count_column<P, Heal>(f, a.n, s, col, hist, a.rows, stripe * a.stride + col);
        }
      }
    }
    // flush this window's counts to its stripe (a wave's consecutive windows
    // can belong to different stripes); the exchange re-arms the histogram
    __builtin_amdgcn_wave_barrier();
    uint32_t* rep = a.reports + stripe * a.report_stride;
    for (int e = lane; e < nwords; e += 64) {
      const uint32_t v = atomicExch(&hist[e], e == 2 ? kScrubNone : 0u);
      if (e == 2) {
        if (v != kScrubNone) atomicMin(&rep[2], v);
      } else if (v != 0u) {
        atomicAdd(&rep[e], v);
      }
    }
    __builtin_amdgcn_wave_barrier();
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
  load_tables(s_exp, s_log);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const uint64_t wlen = a.len - a.col0;
  const uint64_t nthreads = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < a.ntasks;
       idx += nthreads) {
    const uint64_t stripe = idx / wlen;
    const uint64_t col = a.col0 + (idx - stripe * wlen);
    const uint64_t at = stripe * a.stride + col;
    uint8_t s[P];
#pragma unroll
    for (int i = 0; i < P; ++i) s[i] = 0;
    for (int l = a.n - 1; l >= 0; --l) locator::horner_step<P>(f, s, a.rows[l][at]);
    uint32_t nz = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i) nz |= s[i];
    if (nz == 0u) continue;
    count_column<P, Heal>(f, a.n, s, static_cast<uint32_t>(col), a.reports + stripe * a.report_stride, a.rows, at);
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

#define HRS_SCRUB_DISPATCH(fn, heal)         \
  switch (a.p) {                             \
    case 1: return fn<1, heal>(a, s);        \
    case 2: return fn<2, heal>(a, s);        \
    case 3: return fn<3, heal>(a, s);        \
    case 4: return fn<4, heal>(a, s);        \
    case 5: return fn<5, heal>(a, s);        \
    case 6: return fn<6, heal>(a, s);        \
    case 7: return fn<7, heal>(a, s);        \
    case 8: return fn<8, heal>(a, s);        \
    default: return hipErrorInvalidValue;    \
  }

hipError_t launch_scrub(const ScrubArgs& a, hipStream_t s) { HRS_SCRUB_DISPATCH(launch_windows, false) }

hipError_t launch_scrub_bytewise(const ScrubArgs& a, hipStream_t s) { HRS_SCRUB_DISPATCH(launch_columns, false) }

hipError_t launch_heal(const ScrubArgs& a, hipStream_t s) { HRS_SCRUB_DISPATCH(launch_windows, true) }

hipError_t launch_heal_bytewise(const ScrubArgs& a, hipStream_t s) { HRS_SCRUB_DISPATCH(launch_columns, true) }

#undef HRS_SCRUB_DISPATCH

}  // namespace hrs
