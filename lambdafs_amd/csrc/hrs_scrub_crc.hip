// gfx950 fused scrub + CRC-32 (hrs_scrub_crc_dev, hrs_heal_crc_dev): the
// syndromes of every byte column of every stripe AND the java.util.zip.CRC32
// of every cell in ONE pass over the cells. In the reference system a bad
// block is first known by its checksum (Decoder.java:373-387 turns a
// ChecksumException into an erased location) and a repaired block is accepted
// by it (Decoder.java:222-229); a scrubber wants both verdicts from one read.
// Run as two passes (scrub, then hrs_crc32_dev over the n rows) every cell is
// read twice, over pinned host memory twice across the link.
//
// The walk is scrub_kernel's (hrs_scrub.hip): one wave per (stripe, 2 KiB
// window), rows from location n - 1 down to 0 in groups, Horner in the
// bit-sliced domain, one ballot for the clean window; the Horner step, the
// dirty window's column walk, count_column and the per-wave histogram are the
// same code, hrs_scrub_device.hpp. Before a row is sliced
// its eight words feed the lane's two piece CRCs (slicing-by-4, the chains of
// a group in lockstep), which are joined with Z_1024 and the Z_{16*2^t} lane
// tree exactly as decode_crc_kernel joins an output's: lane 0 writes the raw
// window CRC to raw[(stripe * n + l) * nwin + w], and crc_fold_kernel finishes
// them with 2 KiB windows. A clean window stores those n words and nothing
// else.
//
// LDS (one block per CU, 163,840 B): the window kernels' CRC image at LDS
// address 0 (kCrcLdsWordsA * 4 = 159,744 B) leaves 4,096 B. The locator's
// exp/log tables take 768 B, so 3,328 B remain for the per-wave histograms of
// 4 + n words: 16 waves x 52 words. The fused limit kScrubCrcMaxRows = 16
// locations (20 words per wave, 1,280 B for 16 waves) is set by the default
// codec table, not by LDS; 161,792 B are used.
//
// Heal: the CRC is computed from the registers, i.e. from the bytes as loaded,
// so a window in which the wave patched a column holds stale raw words. The
// wave appends such a task to a list in the call's scratch (one atomic per
// dirty window; a window is one wave's, so no task is listed twice), and
// scrub_crc_redo_kernel, launched after it, reads the listed windows again
// and rewrites their n raw words. The kernel boundary orders the byte stores
// before those loads, over pinned host memory too. The list's order depends
// on scheduling; the words written do not.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "hrs_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_locator.hpp"
#include "hrs_scrub_device.hpp"

namespace hrs {
namespace {

constexpr int kHistWords = kScrubHead + kScrubCrcMaxRows;  // per wave
constexpr int kFieldWords = (512 + 256) / 4;               // exp + log after the CRC image

constexpr size_t scrub_crc_lds_bytes(int threads) {
  return (static_cast<size_t>(kCrcLdsWordsA) + kFieldWords + static_cast<size_t>(threads / 64) * kHistWords) * 4;
}
static_assert(scrub_crc_lds_bytes(1024) <= 163840, "the CRC image, the field tables and 16 histograms fit one CU's LDS");

// Rows top - 1 .. top - R of the window at `base`: loaded together, their 2R
// piece chains, R Z_1024 joins and R lane trees advanced in lockstep (8R
// independent LDS lookups per step), the raw window CRCs stored by lane 0,
// then each row sliced and folded into the syndromes (Horner, descending l).
template <int P, int R>
__device__ __forceinline__ void rows_group(const ScrubCrcArgs& a, int top, uint64_t base, uint64_t raw_at, int lane,
                                           const SliceTab& slices, const uint32_t* zchunk, const uint32_t* tree,
                                           uint32_t (&acc)[P][8]) {
  uint32_t w[R][8];
#pragma unroll
  for (int g = 0; g < R; ++g) load_row(a.rows[top - 1 - g] + base, lane, w[g]);
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
  // lane_tree_dpp, level by level across the group
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
    for (int g = 0; g < R; ++g) a.raw[raw_at + static_cast<uint64_t>(top - 1 - g) * a.nwin] = c[g];
  }
#pragma unroll
  for (int g = 0; g < R; ++g) {
    bitslice(w[g]);
    horner_sliced<P>(acc, w[g]);
  }
}

// G (a power of two): rows of a window in flight per wave. The last, shorter
// group goes as its binary pieces, so no lane computes a CRC of a row that is
// not there.
template <int P, bool Heal, int THREADS, int G>
__global__ void __launch_bounds__(THREADS) scrub_crc_kernel(const ScrubCrcArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
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
  for (uint32_t j = 0; j < 0xFFFFFFFFu; ++j) {
    const uint64_t t = wt.at(j);
    if (t >= wt.end) break;
    const uint64_t stripe = t / a.nwin;
    const uint64_t win = t - stripe * a.nwin;
    const uint64_t off = win * kWindowBytes;
    const uint64_t base = stripe * a.stride + off;
    const uint64_t raw_at = stripe * a.n * a.nwin + win;  // + l * nwin: raw[(stripe * n + l) * nwin + win]
    uint32_t acc[P][8];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[i][q] = 0u;
    int top = a.n;
#pragma unroll 1
    for (; top >= G; top -= G) rows_group<P, G>(a, top, base, raw_at, lane, slices, zchunk, tree, acc);
    if constexpr (G > 4)
      if (top & 4) {
        rows_group<P, 4>(a, top, base, raw_at, lane, slices, zchunk, tree, acc);
        top -= 4;
      }
    if constexpr (G > 2)
      if (top & 2) {
        rows_group<P, 2>(a, top, base, raw_at, lane, slices, zchunk, tree, acc);
        top -= 2;
      }
    if constexpr (G > 1)
      if (top & 1) rows_group<P, 1>(a, top, base, raw_at, lane, slices, zchunk, tree, acc);
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
      // count_column with constant indices: loc / err stay in registers (no scratch)
      auto column = [&](const uint8_t(&s)[P], uint32_t col, int, int) {
        count_column<P, Heal, true>(f, a.n, s, col, hist, a.rows, stripe * a.stride + col);
      };
      for_each_bad_column<P>(acc, static_cast<uint32_t>(off), lane, column);
    }
    if constexpr (Heal) {
      // the wave stored into this window: its raw words are stale (redo kernel)
      __builtin_amdgcn_wave_barrier();
      if (lane == 0 && hist[kScrubPatched] != 0u) {
        const unsigned long long at = atomicAdd(reinterpret_cast<unsigned long long*>(a.dirty), 1ull);
        a.dirty[1 + at] = t;
      }
    }
    hist_flush(hist, a.reports + stripe * a.report_stride, nwords, lane);
  }
}

// The raw window CRCs of the tasks the heal listed, from the bytes as they
// are now: one wave per listed task, a row at a time. A block whose first
// wave has nothing to do leaves before it loads the table image, so a clean
// batch costs one launch of blocks that read one word.
constexpr int kRedoThreads = 512;

__global__ void __launch_bounds__(kRedoThreads) scrub_crc_redo_kernel(const ScrubCrcArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr uint32_t wpb = kRedoThreads / 64;
  const uint64_t count = a.dirty[0];
  if (static_cast<uint64_t>(blockIdx.x) * wpb >= count) return;  // block-uniform
  for (int i = threadIdx.x; i < kCrcLdsWordsA; i += kRedoThreads) lds[i] = a.tables[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const SliceTab slices = slice_tab(lane);
  const uint32_t* zchunk = lds + kCrcSliceWords;
  const uint32_t* tree = zchunk + 1024;
  const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * wpb;
  for (uint64_t i = wave_id_in_grid(); i < count; i += nwaves) {
    const uint64_t t = a.dirty[1 + i];
    const uint64_t stripe = t / a.nwin;
    const uint64_t win = t - stripe * a.nwin;
    const uint64_t base = stripe * a.stride + win * kWindowBytes;
#pragma unroll 1
    for (int l = 0; l < a.n; ++l) {
      uint32_t w[8];
      load_row(a.rows[l] + base, lane, w);
      const uint32_t c0 = piece_crc(slices, w[0], w[1], w[2], w[3]);
      const uint32_t c1 = piece_crc(slices, w[4], w[5], w[6], w[7]);
      const uint32_t c = lane_tree_dpp(tree, zmul_xor(zchunk, c0, c1));
      if (lane == 0) a.raw[(stripe * a.n + l) * a.nwin + win] = c;
    }
  }
}

// Block width and rows in flight, from the compiler's resource report
// (DESIGN §10.2): 1,024 threads (4 waves per SIMD, 128 VGPRs) hold 4 rows of
// a window in flight; HRS_SCRUB_CRC_THREADS=512 selects 2 waves per SIMD with
// 8 rows in flight (A/B runs; read per launch).
int scrub_crc_threads() {
  const char* e = getenv("HRS_SCRUB_CRC_THREADS");
  return (e && atoi(e) == 512) ? 512 : 1024;
}

template <int P, bool Heal>
hipError_t launch_sc(const ScrubCrcArgs& a, int cus, hipStream_t s) {
  // P = 2 has the 512-thread form only: under the 128-VGPR budget of 1,024
  // threads the compiler leaves 8 bytes of the locator's arrays in scratch
  // at every G (resource report; the fused kernels carry none)
  const int threads = P == 2 ? 512 : scrub_crc_threads();
  void (*kern)(const ScrubCrcArgs) = scrub_crc_kernel<P, Heal, 512, 8>;
  if constexpr (P != 2)
    if (threads == 1024) kern = scrub_crc_kernel<P, Heal, 1024, 4>;
  const size_t shm = scrub_crc_lds_bytes(threads);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(shm));
  if (e != hipSuccess) return e;
  note_kernel_t(Heal ? "heal_crc_kernel" : "scrub_crc_kernel", P);
  const uint64_t per_block = threads / 64;
  uint64_t g = (a.ntasks + per_block - 1) / per_block;
  if (g > static_cast<uint64_t>(cus)) g = cus;
  g = capped_grid(g);  // zero-copy calls cap it (hrs::GridCap)
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(g)), dim3(threads), shm, s, with_order(a, kOrderScrub));
  return hipGetLastError();
}

}  // namespace

hipError_t launch_scrub_crc(const ScrubCrcArgs& a, bool heal, int cus, hipStream_t s) {
  if (a.n < 1 || a.n > kScrubCrcMaxRows || a.nwin == 0) return hipErrorInvalidValue;
  return dispatch_p<2, kScrubCrcMaxP>(a.p, [&](auto P) {
    return heal ? launch_sc<P, true>(a, cus, s) : launch_sc<P, false>(a, cus, s);
  });
}

hipError_t launch_scrub_crc_redo(const ScrubCrcArgs& a, int cus, hipStream_t s) {
  const size_t shm = static_cast<size_t>(kCrcLdsWordsA) * 4;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(scrub_crc_redo_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(shm));
  if (e != hipSuccess) return e;
  constexpr uint64_t per_block = kRedoThreads / 64;
  uint64_t g = (a.ntasks + per_block - 1) / per_block;
  if (g > static_cast<uint64_t>(cus)) g = cus;
  g = capped_grid(g);
  hipLaunchKernelGGL(scrub_crc_redo_kernel, dim3(static_cast<unsigned>(g)), dim3(kRedoThreads), shm, s, a);
  return hipGetLastError();
}

}  // namespace hrs
