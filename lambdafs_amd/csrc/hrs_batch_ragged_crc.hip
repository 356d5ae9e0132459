// gfx950 ragged repair batches + CRC-32 (hrs_decode_batch_ragged_crc_dev,
// hrs_decode_batch_ragged_host_crc): the ragged repair of
// hrs_batch_ragged.hip with the java.util.zip.CRC32 of every rebuilt cell over
// EXACTLY its real length, as the Decoder takes it: fixErasedBlockImpl updates
// the block's CRC32 with crc.update(writeBufs[i], 0, toWrite),
// toWrite = min(bufSize, limit - written) (Decoder.java:360-369), so no zero
// fill is checksummed behind a short cell (the ragged ENCODE's CRCs, which
// follow Encoder.updateChecksums, do cover it: hrs_ragged_crc.hip).
//
// batch_ragged_crc_kernel<NOUT, NINB, THREADS> is batch_ragged_kernel's walk
// (one wave per (stripe, 2 KiB window), wave_tasks, the pattern indices of the
// next 64 tasks in one vector load, the plan through the constant address
// space, lengths as wave-uniform scalar reads of the plan-order table, the
// skip of a task whose outputs are all dead, full / boundary / dead inputs
// with all live rows loaded before the math, store_row / store_row_below) with
// batch_decode_crc_kernel's CRC half (the 156 KiB LDS image, one block per CU,
// the lane's two piece CRCs joined with Z_1024, lane_tree_dpp, lane 0 writes
// raw[(stripe * max_erased + o) * nwin + w]). Per output of a live task:
//   full      stored and checksummed as in the plain fused kernel;
//   boundary  the un-sliced words are stored below the boundary, then masked
//             from the boundary on before the CRC sees them: the raw word is
//             that of the live bytes followed by zeros up to 2 KiB;
//   dead      no store, no table lookup, no raw word.
// The CRC is taken from the registers; the kernel never reads `out`, so what a
// staged slot image holds behind a cell's length stays out of the checksum.
//
// batch_ragged_crc_fold_kernel folds each cell over its own length: it joins
// the raw words that exist as batch_crc_fold_kernel does (right-aligned over
// the lanes, G windows per lane, the lane tree) and takes the zero padding of
// the last word (fused) or of the row (the window pass of the two-pass route)
// off again with crc::unpad (crc32.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hrs_batch_ragged.hpp"
#include "hrs_crc.hpp"
#include "hrs_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_ragged_device.hpp"

namespace hrs {
namespace {

typedef const __attribute__((address_space(4))) BatchPlan* ConstPlanPtr;

template <int NOUT, int NINB, int THREADS>
__global__ void __launch_bounds__(THREADS) batch_ragged_crc_kernel(const BatchRaggedCrcArgs d) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  for (int i = threadIdx.x; i < kCrcLdsWordsA; i += THREADS) lds[i] = d.tables[i];
  __syncthreads();
  const BatchRaggedArgs& a = d.r;
  const int lane = threadIdx.x & 63;
  const SliceTab slices = slice_tab(lane);
  const uint32_t* zchunk = lds + kCrcSliceWords;
  const uint32_t* tree = zchunk + 1024;
  const ConstPlanPtr plans = (ConstPlanPtr)a.b.plans;
  int patv = 0;
  const WaveTasks wt = wave_tasks(a.b.ntasks, a.b.order);
  for (uint32_t k = 0; k < 0xFFFFFFFFu; ++k) {
    const uint64_t t = wt.at(k);
    if (t >= wt.end) break;
    const uint64_t stripe = t / a.b.nwin;
    const uint64_t w = t - stripe * a.b.nwin;
    const uint64_t off = w * kWindowBytes;
    const uint32_t lo = static_cast<uint32_t>(off);  // len <= UINT32_MAX (the entry points)
    if ((k & 63u) == 0) {  // pattern indices of the next 64 tasks, one vector load
      const uint64_t tl = wt.at(k + static_cast<uint32_t>(lane));
      patv = tl < wt.end ? a.b.pat[tl / a.b.nwin] : 0;
    }
    const ConstPlanPtr pl = plans + __builtin_amdgcn_readlane(patv, static_cast<int>(k & 63u));
    const uint32_t* lw = a.lens + stripe * static_cast<uint64_t>(a.words);
    // output bytes inside this window (0 past the plan's nout: the table says so)
    uint32_t olive[NOUT];
    uint32_t any = 0u;
    bool all_full = true;
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      olive[o] = window_live(uniform_word(lw + a.nin_words + o), lo);
      any |= olive[o];
      all_full = all_full && olive[o] == kWindowBytes;
    }
    if (any == 0u) continue;  // every output dead: nothing loaded, nothing stored, no raw word
    const uint8_t* sb = a.b.base + stripe * a.b.stripe_stride + off;
    uint32_t acc[NOUT][8];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[o][q] = 0u;
    {
      uint32_t live[NINB];  // 0 past the batch's max_nin and past the plan's nin
      uint32_t rows[NINB][8];
#pragma unroll
      for (int i = 0; i < NINB; ++i) live[i] = i < a.nin_words ? window_live(uniform_word(lw + i), lo) : 0u;
#pragma unroll
      for (int i = 0; i < NINB; ++i)
        if (live[i]) load_row(sb + static_cast<uint64_t>(pl->loc[i]) * a.b.row_stride, lane, rows[i]);
#pragma unroll
      for (int i = 0; i < NINB; ++i) {
        if (!live[i]) continue;  // zero planes: no load, no bit-slice, nothing to add
        if (live[i] < kWindowBytes) mask_row(rows[i], lane, live[i]);
        accumulate_row<NOUT, NINB>(acc, rows[i], pl->cw[i]);
      }
    }
    uint8_t* ob = a.b.out + stripe * a.b.out_stripe_stride + off;
    uint32_t* rw = d.raw + stripe * static_cast<uint64_t>(d.rows_per_stripe) * a.b.nwin + w;
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      if (!olive[o]) continue;
      bitslice(acc[o]);
      uint8_t* p = ob + static_cast<uint64_t>(o) * a.b.out_row_stride;
      if (olive[o] == kWindowBytes) {
        store_row(p, lane, acc[o]);
      } else {
        store_row_below(p, lane, acc[o], olive[o]);
        mask_row(acc[o], lane, olive[o]);  // the CRC sees zeros from the boundary on
      }
    }
    if (all_full) {  // wave-uniform: every output's chains in lockstep, as the plain fused kernel
      uint32_t c0[NOUT], c1[NOUT];
      rows_piece_crcs<NOUT>(slices, acc, c0, c1);
#pragma unroll
      for (int o = 0; o < NOUT; ++o) {
        const uint32_t c = lane_tree_dpp(tree, zmul_xor(zchunk, c0[o], c1[o]));
        if (lane == 0) rw[static_cast<uint64_t>(o) * a.b.nwin] = c;
      }
    } else {  // a boundary or a dead output among them: the live outputs one at a time
#pragma unroll
      for (int o = 0; o < NOUT; ++o) {
        if (!olive[o]) continue;
        const uint32_t c0 = piece_crc(slices, acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
        const uint32_t c1 = piece_crc(slices, acc[o][4], acc[o][5], acc[o][6], acc[o][7]);
        const uint32_t c = lane_tree_dpp(tree, zmul_xor(zchunk, c0, c1));
        if (lane == 0) rw[static_cast<uint64_t>(o) * a.b.nwin] = c;
      }
    }
  }
}

__global__ void __launch_bounds__(256) batch_ragged_crc_fold_kernel(const BatchRaggedCrcFoldArgs b) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const CrcFoldArgs& a = b.f;
  for (int i = threadIdx.x; i < kCrcLdsWordsB; i += blockDim.x) lds[i] = a.tables[i];
  __syncthreads();
  const uint32_t* zw = lds;                // Z_window
  const uint32_t* ztree = lds + 1024;      // Z_{window*G*2^t}, t = 0..5
  const uint32_t* ztail = lds + 7 * 1024;  // Z_tail
  const int lane = threadIdx.x & 63;
  const uint64_t wpr = a.nwin + (a.tail ? 1 : 0);
  const uint32_t nwaves = gridDim.x * (blockDim.x / 64);
  for (uint64_t sr = wave_id_in_grid(); sr < a.nsr; sr += nwaves) {
    const uint64_t stripe = sr / b.rows_per_stripe;
    const int t = static_cast<int>(sr - stripe * b.rows_per_stripe);
    const uint32_t start = a.crc_in ? a.crc_in[sr] : 0u;
    // 0 past the stripe's losses (the table says so) and past the batch's max_nout
    const uint32_t v = t < b.max_nout ? b.lens[stripe * static_cast<uint64_t>(b.words) + b.nin_words + t] : 0u;
    if (v == 0u) {  // wave-uniform: continues over no bytes, raw is not read
      if (lane == 0) a.crc_out[sr] = start;
      continue;
    }
    // the full windows whose words exist, and what the last of them (fused) or the row is padded to
    const uint64_t nw = b.fused ? (static_cast<uint64_t>(v) + kWindowBytes - 1) / kWindowBytes : a.nwin;
    const uint64_t tail = b.fused ? 0 : a.tail;
    const uint32_t total = b.fused ? static_cast<uint32_t>(nw * kWindowBytes) : b.len;
    const uint32_t c =
        fold_row(a.raw + sr * wpr, nw, a.G, static_cast<uint64_t>(a.G) * 64 - nw, tail, zw, ztree, ztail, lane);
    if (lane == 0) a.crc_out[sr] = crc::unpad(start, c, total, total - v);
  }
}

// 768 threads (3 waves/SIMD), as batch_decode_crc_kernel: no instantiation
// carries scratch at that width (`make ragged_repair_crc_resources`, DESIGN
// section 13.1).
constexpr int kThreads = 768;

template <int NOUT, int NINB>
hipError_t launch_brc(const BatchRaggedCrcArgs& d, int cus, hipStream_t s) {
  BatchRaggedCrcArgs dc = d;
  dc.r.b.order = task_order(kOrderDecodeCrc);
  auto kern = batch_ragged_crc_kernel<NOUT, NINB, kThreads>;
  const size_t shm = static_cast<size_t>(kCrcLdsWordsA) * 4;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(shm));
  if (e != hipSuccess) return e;
  note_kernel_t("batch_ragged_crc_kernel", NOUT, NINB, kThreads);
  const uint64_t per_block = kThreads / 64;
  uint64_t g = (d.r.b.ntasks + per_block - 1) / per_block;
  if (g > static_cast<uint64_t>(cus)) g = cus;
  g = capped_grid(g);  // zero-copy calls cap it (hrs::GridCap)
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(g)), dim3(kThreads), shm, s, dc);
  return hipGetLastError();
}

template <int NOUT>
hipError_t launch_brc_n(const BatchRaggedCrcArgs& d, int max_nin, int cus, hipStream_t s) {
  if (max_nin <= 4) return launch_brc<NOUT, 4>(d, cus, s);
  if (max_nin <= 8) return launch_brc<NOUT, 8>(d, cus, s);
  if constexpr (NOUT <= 3) {
    if (max_nin <= 12) return launch_brc<NOUT, 12>(d, cus, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_batch_ragged_crc(const BatchRaggedCrcArgs& d, int max_nout, int max_nin, int cus, hipStream_t s) {
  if (!batch_ragged_crc_shape(max_nout, max_nin)) return hipErrorInvalidValue;
  switch (max_nout) {
    case 1: return launch_brc_n<1>(d, max_nin, cus, s);
    case 2: return launch_brc_n<2>(d, max_nin, cus, s);
    case 3: return launch_brc_n<3>(d, max_nin, cus, s);
    default: return launch_brc_n<4>(d, max_nin, cus, s);
  }
}

hipError_t launch_batch_ragged_crc_fold(const BatchRaggedCrcFoldArgs& b, int cus, hipStream_t s) {
  uint64_t blocks = (b.f.nsr + 3) / 4;
  const uint64_t cap = static_cast<uint64_t>(cus) * kCrcFoldBlocksPerCU;
  if (blocks > cap) blocks = cap;
  const size_t shm = static_cast<size_t>(kCrcLdsWordsB) * 4;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(batch_ragged_crc_fold_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(shm));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_ragged_crc_fold_kernel, dim3(static_cast<unsigned>(blocks ? blocks : 1)), dim3(256), shm, s,
                     b);
  return hipGetLastError();
}

}  // namespace hrs
