// Ragged scrub and heal on gfx950 (hrs_scrub_ragged_dev, hrs_heal_ragged_dev
// and their host batches): the scrub of hrs_scrub.hip over cells of which only
// the leading bytes hold data.
//
// The stripes of a file's tail are encoded from short and empty cells
// (hrs_encode_ragged_*); their zero tails are never stored. Here every cell's
// length arrives in a per-call table in hops order (hrs_scrub_ragged.hpp) and
// the zeros are never read: a 2 KiB window of a cell that lies wholly at or
// beyond its length costs no load and no bit-slice, the one window that holds
// the boundary is loaded and masked, and a window at or beyond every cell of
// its stripe costs one scalar read.
//
// scrub_ragged_kernel<P, Heal> is scrub_kernel's window walk: one wave per
// window, wave_tasks, rows in groups of 8 from location n - 1 down, the
// clean-window ballot, the locator on the lane's bad columns. A task's lengths
// are wave-uniform scalar reads, the row cases (full, boundary, dead)
// wave-uniform branches. The Horner recurrence has to advance past a dead row
// (acc_i <- alpha^i acc_i): while every row so far was dead the accumulators
// are zero and the step is skipped behind a wave-uniform flag (the file tail:
// the highest data locations are the empty ones); a dead row below a live one
// runs the step on a zero row, VALU only. The step is one piece of code for
// both row cases: with a Horner step of its own in each branch every
// instantiation took 32 P more VGPRs and P = 2..5 lost a wave per SIMD.
//
// One rule beyond the scrub's, demotion: a virtual zero cannot be patched. A
// column the locator resolves by blaming, with a nonzero error value, a cell
// whose length the column lies at or beyond counts as unresolved, and the heal
// stores nothing in it (include/hrs.h).
#include <hip/hip_runtime.h>

#include "hrs_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_locator.hpp"
#include "hrs_ragged_device.hpp"
#include "hrs_scrub_device.hpp"
#include "hrs_scrub_ragged.hpp"

namespace hrs {
namespace {

constexpr int kScrubRaggedGroup = 8;  // rows of a window in flight per wave, as scrub_kernel

// The locator on the syndromes s (not all zero) of column col, the demotion
// rule over the stripe's lengths lw[0..n), then the report rule. The lengths of
// the blamed locations are ordinary per-lane loads.
template <int P, bool Heal>
__device__ __forceinline__ void count_ragged_column(const locator::Field& f, int n, const uint8_t (&s)[P], uint32_t col,
                                                    const uint32_t* lw, uint32_t* h, const uint8_t* const* rows,
                                                    uint64_t at) {
  int nloc = 0;
  uint8_t loc[locator::kMaxErrors], err[locator::kMaxErrors];
  bool resolved = locator::locate(f, n, P, s, &nloc, loc, err);
  if (resolved)
    for (int j = 0; j < nloc; ++j)
      if (err[j] != 0 && col >= lw[loc[j]]) resolved = false;  // a patch of a virtual zero: demoted
  account_column<P, Heal, false>(h, col, resolved, nloc, loc, err, rows, at);
}

// ------------------------------------------------------ vector kernel

template <int P, bool Heal>
__global__ void __launch_bounds__(kBlockThreads) scrub_ragged_kernel(const ScrubRaggedArgs ra) {
  const ScrubArgs& a = ra.s;
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
    const uint32_t lo = static_cast<uint32_t>(off);  // len <= UINT32_MAX (the entry points)
    const uint32_t* lw = ra.lens + stripe * static_cast<uint64_t>(a.n + 1);
    if (uniform_word(lw + a.n) <= lo) continue;  // at or beyond every cell of the stripe: nothing loaded
    const uint64_t base = stripe * a.stride + off;
    uint32_t acc[P][8];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[i][q] = 0u;
    bool started = false;  // wave-uniform: a live row has been taken, acc may be nonzero
    for (int l0 = a.n; l0 > 0; l0 -= kScrubRaggedGroup) {
      uint32_t live[kScrubRaggedGroup];
      uint32_t w[kScrubRaggedGroup][8];
#pragma unroll
      for (int g = 0; g < kScrubRaggedGroup; ++g)
        live[g] = l0 - 1 - g >= 0 ? window_live(uniform_word(lw + (l0 - 1 - g)), lo) : 0u;
#pragma unroll
      for (int g = 0; g < kScrubRaggedGroup; ++g)
        if (live[g]) load_row(a.rows[l0 - 1 - g] + base, lane, w[g]);
#pragma unroll
      for (int g = 0; g < kScrubRaggedGroup; ++g) {
        if (l0 - 1 - g < 0) continue;
        if (live[g]) {
          if (live[g] < kWindowBytes) mask_row(w[g], lane, live[g]);
          bitslice(w[g]);
          started = true;
        } else {
#pragma unroll
          for (int q = 0; q < 8; ++q) w[g][q] = 0u;  // a dead row: the zero row, sliced or not
        }
        if (started) horner_sliced<P>(acc, w[g]);  // skipped while every row so far was dead: acc is zero
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
        count_ragged_column<P, Heal>(f, a.n, s, col, lw, hist, a.rows, stripe * a.stride + col);
      };
      for_each_bad_column<P>(acc, lo, lane, column);
    }
    hist_flush(hist, a.reports + stripe * a.report_stride, nwords, lane);
  }
}

// ------------------------------------------- byte-granular kernel (any alignment)

// One column per lane, as scrub_bytewise_kernel: rows or strides that are not
// 16-byte aligned, the row tail (len % 2 KiB) and kernel mode 2. A location's
// byte is loaded only where the column lies below its length.
template <int P, bool Heal>
__global__ void __launch_bounds__(kBlockThreads) scrub_ragged_bytewise_kernel(const ScrubRaggedArgs ra) {
  const ScrubArgs& a = ra.s;
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  load_field_tables(s_exp, s_log, blockDim.x);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const uint64_t nthreads = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < a.ntasks;
       idx += nthreads) {
    const BytewiseTask t = bytewise_task(a, idx);
    const uint32_t* lw = ra.lens + t.stripe * static_cast<uint64_t>(a.n + 1);
    const uint32_t col = static_cast<uint32_t>(t.col);
    if (col >= lw[a.n]) continue;  // at or beyond every cell of the stripe
    uint8_t s[P];
#pragma unroll
    for (int i = 0; i < P; ++i) s[i] = 0;
    for (int l = a.n - 1; l >= 0; --l)
      locator::horner_step<P>(f, s, col < lw[l] ? a.rows[l][t.at] : uint8_t{0});
    uint32_t nz = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i) nz |= s[i];
    if (nz == 0u) continue;
    count_ragged_column<P, Heal>(f, a.n, s, col, lw, a.reports + t.stripe * a.report_stride, a.rows, t.at);
  }
}

template <int P, bool Heal>
hipError_t launch_windows(const ScrubRaggedArgs& a, hipStream_t s) {
  auto kern = scrub_ragged_kernel<P, Heal>;
  note_kernel_t(Heal ? "heal_ragged_kernel" : "scrub_ragged_kernel", P);
  ScrubRaggedArgs b = a;
  b.s.order = task_order(kOrderScrub);
  hipLaunchKernelGGL(kern, dim3(stream_grid(a.s.ntasks)), dim3(kBlockThreads), 0, s, b);
  return hipGetLastError();
}

template <int P, bool Heal>
hipError_t launch_columns(const ScrubRaggedArgs& a, hipStream_t s) {
  auto kern = scrub_ragged_bytewise_kernel<P, Heal>;
  note_kernel_t(Heal ? "heal_ragged_bytewise_kernel" : "scrub_ragged_bytewise_kernel", P);
  const unsigned g = grid_for(kern, kBlockThreads, a.s.ntasks);
  hipLaunchKernelGGL(kern, dim3(g), dim3(kBlockThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_scrub_ragged(const ScrubRaggedArgs& a, bool heal, hipStream_t s) {
  return dispatch_p<1, 8>(a.s.p, [&](auto P) {
    return heal ? launch_windows<P, true>(a, s) : launch_windows<P, false>(a, s);
  });
}

hipError_t launch_scrub_ragged_bytewise(const ScrubRaggedArgs& a, bool heal, hipStream_t s) {
  return dispatch_p<1, 8>(a.s.p, [&](auto P) {
    return heal ? launch_columns<P, true>(a, s) : launch_columns<P, false>(a, s);
  });
}

}  // namespace hrs
