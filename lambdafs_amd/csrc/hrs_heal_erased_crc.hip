// gfx950 fused heal with known erasures + CRC-32 (hrs_heal_erased_crc_dev,
// hrs_heal_erased_batch_host_crc): every stripe's lost cells rebuilt, the
// silent errors of its survivors fixed AND the java.util.zip.CRC32 of every
// cell as the call leaves it, in one pass over the survivors. Run as two
// passes (hrs_heal_erased_dev, then hrs_crc32_dev over the n rows) every cell
// is read a second time, over pinned host memory a second time across the link.
//
// The walk is heal_erased_kernel's (hrs_heal_erased.hip): one wave per 2 KiB
// window, the stripe's pattern in the lanes (fields by v_readlane), Horner
// over the rows from location n - 1 down in the bit-sliced domain, an erased
// row not loaded and taking the xtime-only step, then the tail both kernels
// run (heal_tail, hrs_heal_erased_device.hpp): tv = M S, the ballot, the bad
// columns. The CRC side is
// scrub_crc_kernel's (hrs_scrub_crc.hip): before a survivor row is sliced its
// eight words feed the lane's two piece chains, the Z_1024 join and the lane
// tree, the chains of a group in lockstep; lane 0 writes the raw window CRC to
// raw[(stripe * n + l) * nwin + w], and crc_fold_kernel finishes them. A slot
// of a group whose row is erased reads one 16-byte piece of a survivor (as in
// heal_erased_kernel) and runs its chain with the others; that word is
// dropped. An erased row's raw word comes from its un-sliced tv registers just
// before store_row: they are the bytes written, in a loaded row's layout.
//
// Dirty rule: every window with a bad column (a nonzero T in some lane) is
// appended to the dirty list, and scrub_crc_redo_kernel, launched after this
// kernel, rewrites its n raw words from memory. In such a window the lane that
// owns a bad column patches survivors after they were loaded; in every other
// window no survivor byte is stored, so the survivors' registers are their
// memory, and an erased row's registers are stored as they are. So the only
// raw words taken from computed registers are a clean window's erased rows.
//
// LDS: the CRC image, the locator's tables and one histogram of 4 + 16 words
// per wave, as scrub_crc_kernel (161,792 B at 1,024 threads; one block per CU).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "hrs_crc.hpp"
#include "hrs_device.hpp"
#include "hrs_heal_erased.hpp"
#include "hrs_heal_erased_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_locator.hpp"
#include "hrs_scrub_device.hpp"

namespace hrs {
namespace {

constexpr int kHistWords = kScrubHead + kScrubCrcMaxRows;  // per wave
constexpr int kFieldWords = (512 + 256) / 4;               // exp + log after the CRC image

constexpr size_t heal_erased_crc_lds_bytes(int threads) {
  return (static_cast<size_t>(kCrcLdsWordsA) + kFieldWords + static_cast<size_t>(threads / 64) * kHistWords) * 4;
}
static_assert(heal_erased_crc_lds_bytes(1024) <= 163840, "the CRC image, the field tables and 16 histograms fit one CU's LDS");

// The raw CRC of the window whose un-sliced words the lane holds in w.
__device__ __forceinline__ uint32_t window_crc(const SliceTab& slices, const uint32_t* zchunk, const uint32_t* tree,
                                               const uint32_t (&w)[8]) {
  const uint32_t c0 = piece_crc(slices, w[0], w[1], w[2], w[3]);
  const uint32_t c1 = piece_crc(slices, w[4], w[5], w[6], w[7]);
  return lane_tree_dpp(tree, zmul_xor(zchunk, c0, c1));
}

// Rows top - 1 .. top - R of the window at `base` (slot g is location
// top - 1 - g; bit R - 1 - g of `gone`: it is erased). Every slot loads in one
// straight run (heal_erased_kernel says why): a slot with no survivor row
// reads one 16-byte piece of row `spare` in every lane. The R pairs of piece
// chains, the joins and the lane trees advance in lockstep as in rows_group of
// hrs_scrub_crc.hip; lane 0 stores the survivors' raw words. Then each row is
// folded into the syndromes (Horner, descending l): a survivor sliced and
// added, an erased row as the xtime-only step.
template <int P, int R>
__device__ __forceinline__ void rows_group(const ScrubCrcArgs& a, int top, uint32_t gone, int spare, uint64_t base,
                                           uint64_t raw_at, int lane, const SliceTab& slices, const uint32_t* zchunk,
                                           const uint32_t* tree, uint32_t (&acc)[P][8]) {
  uint32_t w[R][8];
#pragma unroll
  for (int g = 0; g < R; ++g) {
    const bool take = !((gone >> (R - 1 - g)) & 1u);
    const uint8_t* p = a.rows[take ? top - 1 - g : spare] + base;
    const uint32_t lo = take ? lane * 16u : 0u, hi = take ? 1024u : 0u;
    const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + lo));
    const u32x4 y = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + lo + hi));
    w[g][0] = x[0]; w[g][1] = x[1]; w[g][2] = x[2]; w[g][3] = x[3];
    w[g][4] = y[0]; w[g][5] = y[1]; w[g][6] = y[2]; w[g][7] = y[3];
  }
  uint32_t c0[R], c1[R];
#pragma unroll
  for (int g = 0; g < R; ++g) {
    c0[g] = w[g][0];
    c1[g] = w[g][4];
  }
#pragma unroll
  for (int st = 0; st < 3; ++st)
#pragma unroll
    for (int g = 0; g < R; ++g) {
      c0[g] = slice4_xor(slices, c0[g], w[g][st + 1]);
      c1[g] = slice4_xor(slices, c1[g], w[g][st + 5]);
    }
#pragma unroll
  for (int g = 0; g < R; ++g) {
    c0[g] = slice4(slices, c0[g]);
    c1[g] = slice4(slices, c1[g]);
  }
  uint32_t c[R];
#pragma unroll
  for (int g = 0; g < R; ++g) c[g] = zmul_xor(zchunk, c0[g], c1[g]);
#pragma unroll
  for (int g = 0; g < R; ++g) c[g] = zmul(tree + 0 * 1024, c[g]) ^ dpp_down<1>(c[g]);
#pragma unroll
  for (int g = 0; g < R; ++g) c[g] = zmul(tree + 1 * 1024, c[g]) ^ dpp_down<2>(c[g]);
#pragma unroll
  for (int g = 0; g < R; ++g) c[g] = zmul(tree + 2 * 1024, c[g]) ^ dpp_down<4>(c[g]);
#pragma unroll
  for (int g = 0; g < R; ++g) c[g] = zmul(tree + 3 * 1024, c[g]) ^ dpp_down<8>(c[g]);
#pragma unroll
  for (int g = 0; g < R; ++g) c[g] = zmul(tree + 4 * 1024, c[g]) ^ __shfl_down(c[g], 16, 64);
#pragma unroll
  for (int g = 0; g < R; ++g) c[g] = zmul(tree + 5 * 1024, c[g]) ^ __shfl_down(c[g], 32, 64);
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < R; ++g)
      if (!((gone >> (R - 1 - g)) & 1u)) a.raw[raw_at + static_cast<uint64_t>(top - 1 - g) * a.nwin] = c[g];
  }
#pragma unroll
  for (int g = 0; g < R; ++g) {
    const bool live = !((gone >> (R - 1 - g)) & 1u);
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

// The fused shapes have n <= 16: the whole mask is its first word.
__device__ __forceinline__ uint32_t gone_bits(uint32_t mask0, int top, int r) {
  return (mask0 >> (top - r)) & ((1u << r) - 1u);
}

// G (a power of two): rows of a window in flight per wave; the last, shorter
// group goes as its binary pieces, as in scrub_crc_kernel.
template <int P, int THREADS, int G>
__global__ void __launch_bounds__(THREADS) heal_erased_crc_kernel(const HealErasedCrcArgs ha) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const ScrubCrcArgs& a = ha.c;
  for (int i = threadIdx.x; i < kCrcLdsWordsA; i += THREADS) lds[i] = a.tables[i];
  uint8_t* s_exp = reinterpret_cast<uint8_t*>(lds + kCrcLdsWordsA);
  uint8_t* s_log = s_exp + 512;
  uint32_t* s_hist = lds + kCrcLdsWordsA + kFieldWords;
  load_field_tables(s_exp, s_log, THREADS);
  hist_init(s_hist, kHistWords, THREADS / 64);
  __syncthreads();
  const locator::Field f{s_exp, s_log};
  const int lane = threadIdx.x & 63;
  const SliceTab slices = slice_tab(lane);
  const uint32_t* zchunk = lds + kCrcSliceWords;
  const uint32_t* tree = zchunk + 1024;
  uint32_t* hist = s_hist + (threadIdx.x >> 6) * kHistWords;
  const int nwords = kScrubHead + a.n;
  const WaveTasks wt = wave_tasks(a.ntasks, a.order);
  // the pattern of window j + 1 and the index of window j + 2 are in flight
  // while window j runs, as in heal_erased_kernel
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
    const uint64_t win = t - stripe * a.nwin;
    const uint64_t off = win * kWindowBytes;
    const uint64_t base = stripe * a.stride + off;
    const uint64_t raw_at = stripe * a.n * a.nwin + win;  // + l * nwin: raw[(stripe * n + l) * nwin + win]
    const uint32_t pv = pv_next;
    stripe_cur = stripe_next;
    if (wt.at(j + 1) < wt.end) pv_next = load_pattern(ha.pats, pi_next, lane);
    if (wt.at(j + 2) < wt.end) {
      stripe_next = wt.at(j + 2) / a.nwin;
      pi_next = ha.pat[stripe_next];
    }
    const int spare = static_cast<int>(pattern_word(pv, kPatSpare));
    const uint32_t mask0 = pattern_word(pv, kPatMask);
    uint32_t acc[P][8];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[i][q] = 0u;
    int top = a.n;
#pragma unroll 1
    for (; top >= G; top -= G)
      rows_group<P, G>(a, top, gone_bits(mask0, top, G), spare, base, raw_at, lane, slices, zchunk, tree, acc);
    if constexpr (G > 4)
      if (top & 4) {
        rows_group<P, 4>(a, top, gone_bits(mask0, top, 4), spare, base, raw_at, lane, slices, zchunk, tree, acc);
        top -= 4;
      }
    if constexpr (G > 2)
      if (top & 2) {
        rows_group<P, 2>(a, top, gone_bits(mask0, top, 2), spare, base, raw_at, lane, slices, zchunk, tree, acc);
        top -= 2;
      }
    if constexpr (G > 1)
      if (top & 1) rows_group<P, 1>(a, top, gone_bits(mask0, top, 1), spare, base, raw_at, lane, slices, zchunk, tree, acc);
    // a clean window's erased rows give their raw words before they are
    // stored; a dirty window's words come from the redo kernel
    const bool dirty = heal_tail<P>(
        f, a.n, a.rows, ha.pats, pv, stripe * a.stride, static_cast<uint32_t>(off), lane, hist, acc,
        [&] { return ha.pat[stripe]; },
        [&](int l, const uint32_t(&row)[8], bool dirty_window) {
          if (!dirty_window) {
            const uint32_t c = window_crc(slices, zchunk, tree, row);
            if (lane == 0) a.raw[raw_at + static_cast<uint64_t>(l) * a.nwin] = c;
          }
          store_row(const_cast<uint8_t*>(a.rows[l]) + base, lane, row);
        });
    if (!dirty) continue;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      const unsigned long long at = atomicAdd(reinterpret_cast<unsigned long long*>(a.dirty), 1ull);
      a.dirty[1 + at] = t;
    }
    hist_flush(hist, a.reports + stripe * a.report_stride, nwords, lane);
  }
}

// Block width and rows in flight, from the compiler's resource report (DESIGN
// 10.4): HRS_HEAL_ERASED_CRC_THREADS=512 selects the 512-thread form where
// both are built (A/B runs; read per launch).
int heal_erased_crc_threads() {
  const char* e = getenv("HRS_HEAL_ERASED_CRC_THREADS");
  return (e && atoi(e) == 512) ? 512 : 1024;
}

template <int P>
hipError_t launch_hec(const HealErasedCrcArgs& a, int cus, hipStream_t s) {
  // P = 4 has the 512-thread form only: under the 128-VGPR budget of 1,024
  // threads the compiler leaves 16 bytes per lane in scratch, at 2 rows in
  // flight as at 4 (resource report; no built instantiation carries any)
  const int threads = P == 4 ? 512 : heal_erased_crc_threads();
  void (*kern)(const HealErasedCrcArgs) = heal_erased_crc_kernel<P, 512, 8>;
  if constexpr (P != 4)
    if (threads == 1024) kern = heal_erased_crc_kernel<P, 1024, 4>;
  const size_t shm = heal_erased_crc_lds_bytes(threads);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(shm));
  if (e != hipSuccess) return e;
  note_kernel_t("heal_erased_crc_kernel", P);
  const uint64_t per_block = threads / 64;
  uint64_t g = (a.c.ntasks + per_block - 1) / per_block;
  if (g > static_cast<uint64_t>(cus)) g = cus;
  g = capped_grid(g);  // zero-copy calls cap it (hrs::GridCap)
  HealErasedCrcArgs b = a;
  b.c.order = task_order(kOrderScrub);
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(g)), dim3(threads), shm, s, b);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_heal_erased_crc(const HealErasedCrcArgs& a, int cus, hipStream_t s) {
  if (a.c.n < 1 || a.c.n > kScrubCrcMaxRows || a.c.nwin == 0) return hipErrorInvalidValue;
  return dispatch_p<2, kScrubCrcMaxP>(a.c.p, [&](auto P) { return launch_hec<P>(a, cus, s); });
}

}  // namespace hrs
