// gfx950 ragged encode + CRC-32 (hrs_encode_ragged_crc_dev,
// hrs_encode_ragged_batch_host_crc): Encoder.encodeStripe with
// computeBlockChecksum over a file's last stripe. The reference zero-fills
// what a source has no bytes for (RaidUtils.readTillEnd) and checksums every
// buffer over its full length, zero fill included (updateChecksums,
// Encoder.java:408-460). Here data cell j of stripe s holds valid[s * k + j]
// leading bytes and the zeros behind them are never stored or read: the raw
// CRC of a window of zeros is 0 and a raw CRC followed by n zero bytes is
// Z_n of it (crc32.hpp), so a dead window costs no load and no table lookup.
//
// encode_ragged_crc_kernel<K, P, MATRIX, THREADS, G> is
// encode_crc_grouped_kernel's walk (hrs_fused.hip): one wave per (stripe,
// window of `subs` 2 KiB sub-windows), the same lane layout, the Z_1024 Horner
// chain per row across sub-windows, the lane tree, the factored XOR network,
// the raw layout [stripe][row][window], task order and block shape. Each data
// row of each sub-window is classified as encode_ragged_body does it
// (hrs_ragged.hip), from the stripe's K valid words in SGPRs:
//   full      loaded and processed as in the plain fused kernel;
//   boundary  loaded, then masked BEFORE the CRC and the bit-slice see it;
//   dead      no load, no slicing lookups, no bit-slice, zero planes into the
//             network; its CRC chain still advances over the 2 KiB of zeros
//             (two Z_1024 steps) unless the row has been dead since the
//             window's first sub-window, when the chain is still 0.
// A group's live rows are all loaded before the group's math. A group whose
// rows are all live runs the parent's lockstep CRC chains; a mixed group runs
// its live rows' chains one row at a time.
//
// crc_ragged_window_kernel<ALIGNED> is crc_window_kernel (hrs_crc.hip) with an
// upper limit per data row: bytes at or beyond `valid` read as zero and are
// not loaded, a window wholly at or beyond it writes raw 0 without a load.
// Same 32 KiB windows, right-aligned tail window and raw layout, so
// crc_fold_kernel finishes both kernels' words unchanged.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "hrs_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_ragged.hpp"
#include "hrs_ragged_device.hpp"

namespace hrs {
namespace {

// see hrs_fused.hip
#define HRS_PHASE_FENCE() __builtin_amdgcn_sched_barrier(0)

template <int K, int P, class MATRIX, int THREADS, int G>
__global__ void __launch_bounds__(THREADS) encode_ragged_crc_kernel(const EncodeRaggedCrcArgs ra) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const EncodeCrcArgs& a = ra.e;
  for (int i = threadIdx.x; i < kCrcLdsWordsA; i += THREADS) lds[i] = a.tables[i];
  __syncthreads();
  constexpr int N = K + P;
  constexpr int kGroups = (K + G - 1) / G;
  const int lane = threadIdx.x & 63;
  const uint32_t loff = static_cast<uint32_t>(lane) * 16u;
  const SliceTab slices = slice_tab(lane, a.rep_mask);
  const uint32_t* zchunk = lds + kCrcSliceWords;
  const uint32_t* tree = zchunk + 1024;
  const uint64_t ntasks = a.nstripes * a.nwin;
  const WaveTasks wt = wave_tasks(ntasks, a.order);
  for (uint32_t j = 0; j < 0xFFFFFFFFu; ++j) {
    const uint64_t t = wt.at(j);
    if (t >= wt.end) break;
    const uint64_t stripe = t / a.nwin;
    const uint64_t w = t - stripe * a.nwin;
    const uint64_t in_base = stripe * a.in_stride + w * a.subs * kWindowBytes;
    const uint64_t out_base = stripe * a.out_stride + w * a.subs * kWindowBytes;
    const uint32_t win_lo = static_cast<uint32_t>(w * a.subs * kWindowBytes);  // len <= UINT32_MAX (the entry points)
    uint32_t vr[K];  // wave-uniform: SGPRs
#pragma unroll
    for (int r = 0; r < K; ++r) vr[r] = uniform_word(ra.valid + stripe * K + r);
    uint32_t crc[N];
#pragma unroll
    for (int r = 0; r < N; ++r) crc[r] = 0u;
#pragma unroll 1
    for (uint32_t sub = 0; sub < a.subs; ++sub) {
      const uint64_t off = static_cast<uint64_t>(sub) * kWindowBytes;
      const uint32_t lo = win_lo + sub * kWindowBytes;
      uint32_t acc[P][8];
      static_for<0, kGroups>([&](auto gi) __attribute__((always_inline)) {
        constexpr int GI = decltype(gi)::value;
        constexpr int r0 = GI * G;
        HRS_PHASE_FENCE();
        // data bytes of each row inside this sub-window: 0 dead, 2048 full, else the boundary
        uint32_t live[G];
        bool full = true;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          live[g] = kWindowBytes;
          if (r0 + g < K) {
            const uint32_t d = vr[r0 + g] > lo ? vr[r0 + g] - lo : 0u;
            live[g] = d < kWindowBytes ? d : kWindowBytes;
            full = full && live[g] == kWindowBytes;
          }
        }
        uint32_t x[G][8];
        if (full) {  // the plain kernel's group, no branch inside
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (r0 + g < K) load_row_u(a.in[r0 + g] + in_base + off, loff, x[g]);
          uint32_t c0[G], c1[G];
#pragma unroll
          for (int g = 0; g < G; ++g) {
            c0[g] = x[g][0];
            c1[g] = x[g][4];
          }
#pragma unroll
          for (int st = 0; st < 3; ++st)
#pragma unroll
            for (int g = 0; g < G; ++g)
              if (r0 + g < K) {
                c0[g] = slice4_xor(slices, c0[g], x[g][st + 1]);
                c1[g] = slice4_xor(slices, c1[g], x[g][st + 5]);
              }
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (r0 + g < K) {
              c0[g] = slice4(slices, c0[g]);
              c1[g] = slice4(slices, c1[g]);
            }
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (r0 + g < K) {
              crc[r0 + g] = zmul_xor(zchunk, zmul_xor(zchunk, crc[r0 + g], c0[g]), c1[g]);
              __asm__ volatile("" : "+v"(crc[r0 + g]));
            }
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (r0 + g < K) bitslice(x[g]);
        } else {  // a boundary or a dead row in the group: row by row, the live rows' loads first
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (r0 + g < K && live[g]) load_row_u(a.in[r0 + g] + in_base + off, loff, x[g]);
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (r0 + g < K) {
              if (live[g]) {
                if (live[g] < kWindowBytes) mask_row(x[g], lane, live[g]);  // before the CRC and the bit-slice
                const uint32_t c0 = piece_crc(slices, x[g][0], x[g][1], x[g][2], x[g][3]);
                const uint32_t c1 = piece_crc(slices, x[g][4], x[g][5], x[g][6], x[g][7]);
                crc[r0 + g] = zmul_xor(zchunk, zmul_xor(zchunk, crc[r0 + g], c0), c1);
                bitslice(x[g]);
              } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) x[g][q] = 0u;  // zero planes: no load, no lookups, no bit-slice
                // dead after a live sub-window of this window: the chain moves on over the zeros
                if (vr[r0 + g] > win_lo) crc[r0 + g] = zmul(zchunk, zmul(zchunk, crc[r0 + g]));
              }
              __asm__ volatile("" : "+v"(crc[r0 + g]));
            }
        }
        xor_sched_apply<xsched::Sched<MatrixFamily<MATRIX>::value, K, P, G>, GI, G, P>(x, acc);
        // The group's branches end its basic block, and across blocks the
        // compiler sinks every group's network to the planes' first use after
        // the last group, keeping all K rows' sliced planes live (spills): pin
        // the running planes where the group leaves them.
#pragma unroll
        for (int o = 0; o < P; ++o)
#pragma unroll
          for (int q = 0; q < 8; ++q) __asm__ volatile("" : "+v"(acc[o][q]));
      });
      HRS_PHASE_FENCE();
#pragma unroll
      for (int o = 0; o < P; ++o) {
        bitslice(acc[o]);
        store_row_u(a.out[o] + out_base + off, loff, acc[o]);
      }
      uint32_t p0[P], p1[P];
      rows_piece_crcs<P>(slices, acc, p0, p1);
#pragma unroll
      for (int o = 0; o < P; ++o) crc[K + o] = zmul_xor(zchunk, zmul_xor(zchunk, crc[K + o], p0[o]), p1[o]);
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
      const uint32_t c = lane_tree(tree, crc[r]);
      if (lane == 0) a.raw[(stripe * N + r) * a.nwin + w] = c;
    }
  }
}

// crc_window_raw (hrs_device.hpp) of a row that reads as zero from `limit` on
// (wave-uniform): nothing at or beyond it is loaded.
template <bool ALIGNED>
__device__ __forceinline__ uint32_t crc_window_raw_to(const uint8_t* base, uint64_t w, uint64_t nwin, uint64_t len,
                                                      uint64_t limit, int lane, const SliceTab& slices,
                                                      const uint32_t* zchunk, const uint32_t* tree) {
  const bool full = w < nwin;
  const int64_t end = full ? static_cast<int64_t>((w + 1) * kCrcWindow) : static_cast<int64_t>(len);
  const int64_t lo = full ? static_cast<int64_t>(w * kCrcWindow) : static_cast<int64_t>(nwin * kCrcWindow);
  const int64_t hi = static_cast<int64_t>(limit);
  if (hi <= lo) return 0u;  // a window of zeros: raw 0, no load
  if (hi >= end) return crc_window_raw<ALIGNED>(base, w, nwin, len, lane, slices, zchunk, tree);
  // the window that holds the boundary: bytes of [lo, hi) only
  const int64_t start = end - kCrcWindow + lane * crc::kPieceBytes;
  uint32_t c = 0;
#pragma unroll 1
  for (int g = 0; g < crc::kPieces; g += kCrcGroup) {
    uint32_t words[kCrcGroup][4];
#pragma unroll
    for (int q = 0; q < kCrcGroup; ++q) {
      const int64_t pos0 = start + static_cast<int64_t>(g + q) * crc::kChunkBytes;
      if (ALIGNED && full && pos0 + crc::kPieceBytes <= hi) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(base + pos0));
        words[q][0] = v[0];
        words[q][1] = v[1];
        words[q][2] = v[2];
        words[q][3] = v[3];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint32_t x = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int64_t pos = pos0 + 4 * j + b;
            if (pos >= lo && pos < hi) x |= static_cast<uint32_t>(base[pos]) << (8 * b);
          }
          words[q][j] = x;
        }
      }
    }
    uint32_t ch[kCrcGroup];
#pragma unroll
    for (int q = 0; q < kCrcGroup; ++q) ch[q] = 0u;
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int q = 0; q < kCrcGroup; ++q) ch[q] = slice4(slices, ch[q] ^ words[q][st]);
#pragma unroll
    for (int q = 0; q < kCrcGroup; ++q) c = (g + q == 0) ? ch[q] : (zmul(zchunk, c) ^ ch[q]);
  }
  return lane_tree(tree, c);
}

template <bool ALIGNED>
__global__ void __launch_bounds__(kCrcBlockThreads) crc_ragged_window_kernel(const RaggedCrcWinArgs ra) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const CrcWinArgs& a = ra.w;
  for (int i = threadIdx.x; i < kCrcLdsWordsA; i += blockDim.x) lds[i] = a.tables[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const SliceTab slices = slice_tab(lane);
  const uint32_t* zchunk = lds + kCrcSliceWords;
  const uint32_t* tree = zchunk + 1024;
  const uint64_t wpr = a.nwin + (a.tail ? 1 : 0);
  const uint64_t ntasks = a.nstripes * a.nrows * wpr;
  const WaveTasks wt = wave_tasks(ntasks, a.order);
  for (uint32_t j = 0; j < 0xFFFFFFFFu; ++j) {
    const uint64_t t = wt.at(j);
    if (t >= wt.end) break;
    const uint64_t sr = t / wpr;
    const uint64_t w = t - sr * wpr;
    const uint64_t stripe = sr / a.nrows;
    const int row = static_cast<int>(sr - stripe * a.nrows);
    const uint8_t* base = a.rows[row] + stripe * a.stride[row];
    const int r = a.row0 + row;  // parity rows (r >= k) are full
    const uint64_t limit = r < ra.k ? uniform_word(ra.valid + stripe * ra.k + r) : a.len;
    const uint32_t c = crc_window_raw_to<ALIGNED>(base, w, a.nwin, a.len, limit, lane, slices, zchunk, tree);
    if (lane == 0) a.raw[(stripe * a.nrows_total + r) * wpr + w] = c;
  }
}

// One 1024-thread block per CU (16 waves share the 156 KiB table image), on
// capped zero-copy grids too: the plain fused launcher's 256-thread variant
// for small capped jobs (hrs_fused.hip) is not carried over.
constexpr int kThreads = 1024;

// Rows per lockstep group: 2 for every shape. The plain fused kernel takes 4
// from K = 12 (hrs_fused.hip kFusedGroup) and carries 60 bytes of scratch per
// lane there; this kernel at 4 would carry 40 under the 128-VGPR budget of a
// 1,024-thread block, at 2 it has none.
template <int K>
constexpr int kGroup = 2;

template <class MATRIX> constexpr const char* kMatrixName = "";
template <int K, int P> constexpr const char* kMatrixName<gf::EncodeMatrix<K, P>> = "hrs::gf::EncodeMatrix";
template <int K, int P> constexpr const char* kMatrixName<gf::CauchyMatrix<K, P>> = "hrs::gf::CauchyMatrix";

template <int K, int P, class MATRIX>
hipError_t launch_one(const EncodeRaggedCrcArgs& a, int cus, hipStream_t s) {
  constexpr int G = kGroup<K>;
  const size_t shm = static_cast<size_t>(kCrcLdsWordsA) * 4;
  const uint64_t ntasks = a.e.nstripes * a.e.nwin;
  void (*k)(const EncodeRaggedCrcArgs) = encode_ragged_crc_kernel<K, P, MATRIX, kThreads, G>;
  const std::string mat = std::string(kMatrixName<MATRIX>) + "<" + std::to_string(K) + ", " + std::to_string(P) + ">";
  note_kernel_t("encode_ragged_crc_kernel", K, P, mat.c_str(), kThreads, G);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(shm));
  if (e != hipSuccess) return e;
  const uint64_t per_block = kThreads / 64;
  uint64_t g = (ntasks + per_block - 1) / per_block;
  if (g > static_cast<uint64_t>(cus)) g = cus;
  g = capped_grid(g);  // zero-copy calls cap it (hrs::GridCap)
  EncodeRaggedCrcArgs b = a;
  b.e.order = task_order(kOrderFusedEncode);
  hipLaunchKernelGGL(k, dim3(static_cast<unsigned>(g)), dim3(kThreads), shm, s, b);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_encode_ragged_crc(int family, int k, int p, const EncodeRaggedCrcArgs& a, int cus, hipStream_t s,
                                    bool* handled) {
  *handled = true;
  if (family == kStaticCauchy) {
    if (k == 10 && p == 4) return launch_one<10, 4, gf::CauchyMatrix<10, 4>>(a, cus, s);
    if (k == 6 && p == 3) return launch_one<6, 3, gf::CauchyMatrix<6, 3>>(a, cus, s);
  } else {
    if (k == 10 && p == 4) return launch_one<10, 4, gf::EncodeMatrix<10, 4>>(a, cus, s);
    if (k == 6 && p == 3) return launch_one<6, 3, gf::EncodeMatrix<6, 3>>(a, cus, s);
    if (k == 3 && p == 2) return launch_one<3, 2, gf::EncodeMatrix<3, 2>>(a, cus, s);
    if (k == 12 && p == 4) return launch_one<12, 4, gf::EncodeMatrix<12, 4>>(a, cus, s);
  }
  *handled = false;
  return hipSuccess;
}

hipError_t launch_crc_ragged_windows(const RaggedCrcWinArgs& a, bool aligned, int cus, hipStream_t s) {
  // one 1024-thread block per CU (the 156 KiB table image fills its LDS)
  const uint64_t waves = a.w.nstripes * a.w.nrows * (a.w.nwin + (a.w.tail ? 1 : 0));
  const uint64_t per_block = kCrcBlockThreads / 64;
  uint64_t g = (waves + per_block - 1) / per_block;
  if (g > static_cast<uint64_t>(cus)) g = cus;
  g = capped_grid(g);  // zero-copy calls cap it (hrs::GridCap)
  const size_t shm = static_cast<size_t>(kCrcLdsWordsA) * 4;
  auto k = aligned ? crc_ragged_window_kernel<true> : crc_ragged_window_kernel<false>;
  note_kernel(aligned ? "crc_ragged_window_kernel<true>" : "crc_ragged_window_kernel<false>");
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(shm));
  if (e != hipSuccess) return e;
  RaggedCrcWinArgs b = a;
  b.w.order = task_order(kOrderCrc);
  hipLaunchKernelGGL(k, dim3(static_cast<unsigned>(g)), dim3(kCrcBlockThreads), shm, s, b);
  return hipGetLastError();
}

}  // namespace hrs
