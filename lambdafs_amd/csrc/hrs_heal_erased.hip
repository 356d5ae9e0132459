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
#include <hip/hip_runtime.h>

#include "hrs_device.hpp"
#include "hrs_heal_erased.hpp"
#include "hrs_launch.hpp"
#include "hrs_locator.hpp"

namespace hrs {
namespace {

__constant__ gf::Tables d_erased_tables = gf::make_tables();

constexpr int kErasedGroup = 8;  // rows of a window in flight per wave; groups are aligned, one mask byte each

__device__ __forceinline__ void load_tables(uint8_t* s_exp, uint8_t* s_log) {
  for (int i = threadIdx.x; i < 512; i += blockDim.x) s_exp[i] = d_erased_tables.exp[i];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_log[i] = d_erased_tables.log[i];
}

// One column (survivor syndromes s) of a stripe with pattern pt: runs the
// locator, patches the blamed survivors at rows[loc] + at, adds the column to
// the counters at h (a per-wave LDS histogram or the stripe's report) and
// leaves the erased values in v. Returns whether the column was bad.
template <int P>
__device__ __forceinline__ bool heal_column(const locator::Field& f, int n, const uint8_t (&s)[P],
                                            const ErasePattern& pt, uint32_t col, uint32_t* h,
                                            const uint8_t* const* rows, uint64_t at,
                                            uint8_t (&v)[locator::kMaxErased]) {
  int nloc = 0;
  uint8_t loc[locator::kMaxErrors], u[locator::kMaxErrors];
  const int state = locator::locate_errata<P>(f, n, s, pt.e, pt.loc, pt.gamma, &nloc, loc, u, v);
  if (state == locator::kConsistent) return false;
  atomicAdd(&h[0], 1u);
  atomicMin(&h[2], col);
  if (state == locator::kUnresolved) {
    atomicAdd(&h[1], 1u);
    return true;
  }
  uint32_t patched = 0u;
  for (int j = 0; j < nloc; ++j) {
    atomicAdd(&h[kScrubHead + loc[j]], 1u);
    if (u[j] != 0) {
      uint8_t* q = const_cast<uint8_t*>(rows[loc[j]]) + at;
      *q = static_cast<uint8_t>(*q ^ u[j]);
      ++patched;
    }
  }
  if (patched != 0u) atomicAdd(&h[kScrubPatched], patched);
  return true;
}

// ------------------------------------------------------ vector kernel

// The calling wave's copy of its stripe's pattern: lane j % 32 holds dword j
// of the 128-byte table entry (one coalesced load per window); a field comes
// out by v_readlane into an SGPR, so the tests on it run on the scalar unit.
constexpr int kPatE = offsetof(ErasePattern, e) / 4, kPatMask = offsetof(ErasePattern, mask) / 4,
              kPatCw = offsetof(ErasePattern, cw) / 4, kPatLoc = offsetof(ErasePattern, loc) / 4, kPatSpare = offsetof(ErasePattern, spare) / 4;
static_assert(sizeof(ErasePattern) == 128 && offsetof(ErasePattern, cw) % 8 == 0, "one dword per lane of a half wave");

__device__ __forceinline__ uint32_t load_pattern(const HealErasedArgs& ha, int32_t index, int lane) {
  return reinterpret_cast<const uint32_t*>(ha.pats + index)[lane & 31];
}

__device__ __forceinline__ uint32_t pattern_word(uint32_t pv, int word) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(pv), word));
}

template <int P>
__global__ void __launch_bounds__(kBlockThreads) heal_erased_kernel(const HealErasedArgs ha) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  __shared__ uint32_t s_hist[kWavesPerBlock][kScrubHead + kScrubMaxRows];
  const ScrubArgs& a = ha.s;
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
  // Two loads lead to a window's pattern (its stripe's index, then the table
  // entry); both run ahead of the windows so that neither is waited for: while
  // window j runs, the entry of window j + 1 and the index of window j + 2
  // are in flight. One 64-bit division per window, as in the scrub.
  uint64_t stripe_cur = 0, stripe_next = 0;
  uint32_t pv_next = 0u;
  int32_t pi_next = 0;
  if (wt.at(0) < wt.end) {
    stripe_cur = wt.at(0) / a.nwin;
    pv_next = load_pattern(ha, ha.pat[stripe_cur], lane);
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
    if (wt.at(j + 1) < wt.end) pv_next = load_pattern(ha, pi_next, lane);
    if (wt.at(j + 2) < wt.end) {
      stripe_next = wt.at(j + 2) / a.nwin;
      pi_next = ha.pat[stripe_next];
    }
    const int pp = P - static_cast<int>(pattern_word(pv, kPatE));  // wave-uniform, like every field
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
    // tv = M S: T in rows [0, pp), the erased values in rows [pp, P)
    uint32_t tv[P][8];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) tv[i][q] = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      uint32_t x[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = acc[i][q];
      uint32_t cw[2] = {pattern_word(pv, kPatCw + 2 * i), pattern_word(pv, kPatCw + 2 * i + 1)};
      // bit b of every coefficient: tv[o] ^= alpha^b S_i where it is set. Unrolled
      // (xtime is then a relabel of the planes) while the body stays small.
      if constexpr (P <= 4) {
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          if ((cw[0] & (0x01010101u << b)) != 0u) mul_acc_row<P, P>(tv, x, cw, b);
          if (b < 7) xtime(x);
        }
      } else {
#pragma unroll 1
        for (int b = 0; b < 8; ++b) {
          mul_acc_row<P, P>(tv, x, cw, b);
          xtime(x);
        }
      }
    }
    uint32_t any = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i)
      if (i < pp) {
#pragma unroll
        for (int q = 0; q < 8; ++q) any |= tv[i][q];
      }
    const bool dirty = __ballot(any != 0u) != 0ull;  // wave-uniform
    // the lane's 32 columns are bytes 0..3 of words 0..7 of an un-sliced row;
    // word x covers window bytes (x >> 2) * 1024 + lane * 16 + (x & 3) * 4
#pragma unroll
    for (int i = 0; i < P; ++i)
      if (dirty || i >= pp) bitslice(tv[i]);
    if (dirty) {
#pragma unroll
      for (int i = 0; i < P; ++i) bitslice(acc[i]);
      if (any != 0u) {
#pragma unroll 1
        for (int x = 0; x < 8; ++x) {
          uint32_t cur[P], tvx[P];
#pragma unroll
          for (int i = 0; i < P; ++i) {
            uint32_t v = acc[i][0], y = tv[i][0];
#pragma unroll
            for (int q = 1; q < 8; ++q) {  // selects, so acc and tv stay in registers
              v = (x == q) ? acc[i][q] : v;
              y = (x == q) ? tv[i][q] : y;
            }
            cur[i] = v;
            tvx[i] = y;
          }
          uint32_t anyw = 0u;
#pragma unroll
          for (int i = 0; i < P; ++i) anyw |= (i < pp) ? tvx[i] : 0u;
          if (anyw == 0u) continue;
#pragma unroll 1
          for (int b = 0; b < 4; ++b) {
            if (((anyw >> (8 * b)) & 0xFFu) == 0u) continue;
            uint8_t s[P];
#pragma unroll
            for (int i = 0; i < P; ++i) s[i] = static_cast<uint8_t>(cur[i] >> (8 * b));
            const uint32_t col = static_cast<uint32_t>(off) + (x >> 2) * 1024u + lane * 16u + (x & 3) * 4u + b;
            uint8_t v[locator::kMaxErased] = {};
            heal_column<P>(f, a.n, s, ha.pats[ha.pat[stripe]], col, hist, a.rows, stripe * a.stride + col, v);
            // the column's erased bytes, over the corrected syndromes when it resolved
#pragma unroll
            for (int i = 0; i < P; ++i)
              if (i >= pp) {
                uint8_t vb = v[0];
#pragma unroll
                for (int m = 1; m < P; ++m) vb = (i - pp == m) ? v[m] : vb;
                tvx[i] = (tvx[i] & ~(0xFFu << (8 * b))) | (static_cast<uint32_t>(vb) << (8 * b));
              }
          }
#pragma unroll
          for (int i = 0; i < P; ++i)
#pragma unroll
            for (int q = 0; q < 8; ++q) tv[i][q] = (x == q) ? tvx[i] : tv[i][q];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < P; ++i)
      if (i >= pp) {
        const int m = i - pp;
        const int l = (pattern_word(pv, kPatLoc + (m >> 2)) >> (8 * (m & 3))) & 0xFFu;
        store_row(const_cast<uint8_t*>(a.rows[l]) + base, lane, tv[i]);
      }
    if (!dirty) continue;
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
    const uint64_t at = stripe * a.stride + col;
    const ErasePattern& pt = ha.pats[ha.pat[stripe]];
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
// Checked repair (hrs_repair_checked_dev) runs the two kernels above over the
// stripes a device list names (HealListedArgs, hrs_heal_erased.hpp). They are
// copies of the walks, not a template flag on them: with the flag the compiler
// allocated the existing kernels' registers differently (111 -> 96 VGPRs at
// P = 1, another occupancy at P = 1 and 3), and the batch calls keep the code
// they were measured with. What differs: the task range is count * nwin, the
// count read from device memory at kernel entry and clamped to nstripes; a
// task's stripe is the list's entry, which is also its pattern's index; an
// entry that is no stripe of the batch is skipped and never indexed with; a
// block with no task leaves before it loads anything.

// How many stripes the list names, never more than the batch has.
__device__ __forceinline__ uint64_t listed_count(const HealListedArgs& a) {
  const uint32_t count = a.list[0];
  return count < a.nstripes ? count : a.nstripes;
}

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
  __shared__ uint32_t s_hist[kWavesPerBlock][kScrubHead + kScrubMaxRows];
  const HealErasedArgs& ha = la.h;
  const ScrubArgs& a = ha.s;
  // the task range comes from device memory (a.ntasks is only the bound the
  // grid was sized for); a block whose first wave has no window leaves before
  // it loads anything (block-uniform)
  const uint64_t ntasks = listed_count(la) * a.nwin;
  {
    const WaveTasks w0 = wave_tasks(ntasks, a.order);
    if (w0.t0 - (threadIdx.x >> 6) >= w0.end) return;
  }
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
  const WaveTasks wt = wave_tasks(ntasks, a.order);
  // Two loads lead to a window's pattern (its stripe's index, then the table
  // entry); both run ahead of the windows so that neither is waited for: while
  // window j runs, the entry of window j + 1 and the index of window j + 2
  // are in flight; here the first load is the list's entry, which is the index.
  uint64_t pos_cur = 0, pos_next = 0, stripe_cur = 0, stripe_next = 0;
  uint32_t pv_next = 0u;
  int32_t pi_next = 0;
  if (wt.at(0) < wt.end) {
    pos_cur = wt.at(0) / a.nwin;
    stripe_cur = listed_stripe(la, pos_cur);
    pv_next = load_pattern(ha, listed_pattern(la, stripe_cur), lane);
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
    if (wt.at(j + 1) < wt.end) pv_next = load_pattern(ha, pi_next, lane);
    if (wt.at(j + 2) < wt.end) {
      pos_next = wt.at(j + 2) / a.nwin;
      stripe_next = listed_stripe(la, pos_next);
      pi_next = listed_pattern(la, stripe_next);
    }
    if (stripe >= la.nstripes) continue;  // no stripe of this batch: nothing is indexed with it
    const int pp = P - static_cast<int>(pattern_word(pv, kPatE));  // wave-uniform, like every field
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
    // tv = M S: T in rows [0, pp), the erased values in rows [pp, P)
    uint32_t tv[P][8];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) tv[i][q] = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      uint32_t x[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = acc[i][q];
      uint32_t cw[2] = {pattern_word(pv, kPatCw + 2 * i), pattern_word(pv, kPatCw + 2 * i + 1)};
      // bit b of every coefficient: tv[o] ^= alpha^b S_i where it is set. Unrolled
      // (xtime is then a relabel of the planes) while the body stays small.
      if constexpr (P <= 4) {
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          if ((cw[0] & (0x01010101u << b)) != 0u) mul_acc_row<P, P>(tv, x, cw, b);
          if (b < 7) xtime(x);
        }
      } else {
#pragma unroll 1
        for (int b = 0; b < 8; ++b) {
          mul_acc_row<P, P>(tv, x, cw, b);
          xtime(x);
        }
      }
    }
    uint32_t any = 0u;
#pragma unroll
    for (int i = 0; i < P; ++i)
      if (i < pp) {
#pragma unroll
        for (int q = 0; q < 8; ++q) any |= tv[i][q];
      }
    const bool dirty = __ballot(any != 0u) != 0ull;  // wave-uniform
    // the lane's 32 columns are bytes 0..3 of words 0..7 of an un-sliced row;
    // word x covers window bytes (x >> 2) * 1024 + lane * 16 + (x & 3) * 4
#pragma unroll
    for (int i = 0; i < P; ++i)
      if (dirty || i >= pp) bitslice(tv[i]);
    if (dirty) {
#pragma unroll
      for (int i = 0; i < P; ++i) bitslice(acc[i]);
      if (any != 0u) {
#pragma unroll 1
        for (int x = 0; x < 8; ++x) {
          uint32_t cur[P], tvx[P];
#pragma unroll
          for (int i = 0; i < P; ++i) {
            uint32_t v = acc[i][0], y = tv[i][0];
#pragma unroll
            for (int q = 1; q < 8; ++q) {  // selects, so acc and tv stay in registers
              v = (x == q) ? acc[i][q] : v;
              y = (x == q) ? tv[i][q] : y;
            }
            cur[i] = v;
            tvx[i] = y;
          }
          uint32_t anyw = 0u;
#pragma unroll
          for (int i = 0; i < P; ++i) anyw |= (i < pp) ? tvx[i] : 0u;
          if (anyw == 0u) continue;
#pragma unroll 1
          for (int b = 0; b < 4; ++b) {
            if (((anyw >> (8 * b)) & 0xFFu) == 0u) continue;
            uint8_t s[P];
#pragma unroll
            for (int i = 0; i < P; ++i) s[i] = static_cast<uint8_t>(cur[i] >> (8 * b));
            const uint32_t col = static_cast<uint32_t>(off) + (x >> 2) * 1024u + lane * 16u + (x & 3) * 4u + b;
            uint8_t v[locator::kMaxErased] = {};
            heal_column<P>(f, a.n, s, ha.pats[listed_pattern(la, stripe)], col, hist, a.rows, stripe * a.stride + col, v);
            // the column's erased bytes, over the corrected syndromes when it resolved
#pragma unroll
            for (int i = 0; i < P; ++i)
              if (i >= pp) {
                uint8_t vb = v[0];
#pragma unroll
                for (int m = 1; m < P; ++m) vb = (i - pp == m) ? v[m] : vb;
                tvx[i] = (tvx[i] & ~(0xFFu << (8 * b))) | (static_cast<uint32_t>(vb) << (8 * b));
              }
          }
#pragma unroll
          for (int i = 0; i < P; ++i)
#pragma unroll
            for (int q = 0; q < 8; ++q) tv[i][q] = (x == q) ? tvx[i] : tv[i][q];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < P; ++i)
      if (i >= pp) {
        const int m = i - pp;
        const int l = (pattern_word(pv, kPatLoc + (m >> 2)) >> (8 * (m & 3))) & 0xFFu;
        store_row(const_cast<uint8_t*>(a.rows[l]) + base, lane, tv[i]);
      }
    if (!dirty) continue;
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

template <int P>
__global__ void __launch_bounds__(kBlockThreads) heal_listed_bytewise_kernel(const HealListedArgs la) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  const HealErasedArgs& ha = la.h;
  const ScrubArgs& a = ha.s;
  const uint64_t wlen = a.len - a.col0;
  const uint64_t ntasks = listed_count(la) * wlen;
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
    const uint64_t at = stripe * a.stride + col;
    const ErasePattern& pt = ha.pats[listed_pattern(la, stripe)];
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

#define HRS_HEAL_ERASED_DISPATCH(fn)   \
  switch (a.s.p) {                     \
    case 1: return fn<1>(a, s);        \
    case 2: return fn<2>(a, s);        \
    case 3: return fn<3>(a, s);        \
    case 4: return fn<4>(a, s);        \
    case 5: return fn<5>(a, s);        \
    case 6: return fn<6>(a, s);        \
    case 7: return fn<7>(a, s);        \
    case 8: return fn<8>(a, s);        \
    default: return hipErrorInvalidValue; \
  }

hipError_t launch_heal_erased(const HealErasedArgs& a, hipStream_t s) { HRS_HEAL_ERASED_DISPATCH(launch_windows) }

hipError_t launch_heal_erased_bytewise(const HealErasedArgs& a, hipStream_t s) { HRS_HEAL_ERASED_DISPATCH(launch_columns) }

#undef HRS_HEAL_ERASED_DISPATCH

#define HRS_HEAL_LISTED_DISPATCH(fn)   \
  switch (a.h.s.p) {                   \
    case 1: return fn<1>(a, s);        \
    case 2: return fn<2>(a, s);        \
    case 3: return fn<3>(a, s);        \
    case 4: return fn<4>(a, s);        \
    case 5: return fn<5>(a, s);        \
    case 6: return fn<6>(a, s);        \
    case 7: return fn<7>(a, s);        \
    case 8: return fn<8>(a, s);        \
    default: return hipErrorInvalidValue; \
  }

hipError_t launch_heal_listed(const HealListedArgs& a, hipStream_t s) { HRS_HEAL_LISTED_DISPATCH(launch_listed_windows) }

hipError_t launch_heal_listed_bytewise(const HealListedArgs& a, hipStream_t s) { HRS_HEAL_LISTED_DISPATCH(launch_listed_columns) }

#undef HRS_HEAL_LISTED_DISPATCH

}  // namespace hrs
