// gfx950 heterogeneous repair batches + CRC-32 (hrs_decode_batch_crc_dev): one
// erasure pattern per stripe, and the java.util.zip.CRC32 of every repaired
// cell in the same pass — what the Decoder does per lost block (decodeBulk,
// then the repaired block's CRC32 against the NameNode's; Decoder.java:222-229,
// :645-655), for a repair job whose stripes lost different locations.
//
// The task decomposition is batch_bitsliced_kernel's (hrs_batch.hip): one wave
// per (stripe, 2 KiB window), the stripe's plan read through the constant
// address space, its pattern index by one vector load per 64 tasks. The CRC
// half is decode_crc_kernel's (hrs_decode_crc.hip): after a window's outputs
// are un-sliced and stored, lane l holds the pieces at 16 l and 1024 + 16 l of
// each; their raw CRCs, joined with Z_1024 and the lane tree, are the window's
// raw CRC, which lane 0 writes to raw[stripe][output][window] with the CALLER's
// max_erased as the row count, so the fold's (stripe, row) index is the crc_out
// index. Outputs past a stripe's losses are not stored, not checksummed and
// have no raw word; batch_crc_fold_kernel yields crc_in for them without
// reading raw (so crc_out may alias crc_in).
//
// LDS: the window kernels' 156 KiB image, one block per CU; 768 threads
// (3 waves/SIMD), as decode_crc_kernel.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "hrs_crc.hpp"
#include "hrs_device.hpp"
#include "hrs_launch.hpp"

namespace hrs {
namespace {

typedef const __attribute__((address_space(4))) BatchPlan* ConstPlanPtr;

// The raw CRCs of the window's first M outputs, their 2M chains in lockstep
// (dc_crc_task); M is the stripe's loss count, wave-uniform.
template <int M, int NOUT>
__device__ __forceinline__ void bc_crc_outputs(const BatchCrcArgs& d, uint64_t stripe, uint64_t w, int lane,
                                               const SliceTab& slices, const uint32_t* zchunk, const uint32_t* tree,
                                               const uint32_t (&acc)[NOUT][8]) {
  uint32_t x[M][8];
#pragma unroll
  for (int o = 0; o < M; ++o)
#pragma unroll
    for (int q = 0; q < 8; ++q) x[o][q] = acc[o][q];
  uint32_t c0[M], c1[M];
  rows_piece_crcs<M>(slices, x, c0, c1);
#pragma unroll
  for (int o = 0; o < M; ++o) {
    const uint32_t c = lane_tree_dpp(tree, zmul_xor(zchunk, c0[o], c1[o]));
    if (lane == 0) d.raw[(stripe * d.rows_per_stripe + o) * d.b.nwin + w] = c;
  }
}

template <int NOUT, int NINB, int THREADS>
__global__ void __launch_bounds__(THREADS) batch_decode_crc_kernel(const BatchCrcArgs d) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  for (int i = threadIdx.x; i < kCrcLdsWordsA; i += THREADS) lds[i] = d.tables[i];
  __syncthreads();
  const BatchArgs& a = d.b;
  const int lane = threadIdx.x & 63;
  const SliceTab slices = slice_tab(lane);
  const uint32_t* zchunk = lds + kCrcSliceWords;
  const uint32_t* tree = zchunk + 1024;
  const ConstPlanPtr plans = (ConstPlanPtr)a.plans;
  int patv = 0;
  const WaveTasks wt = wave_tasks(a.ntasks, a.order);
  for (uint32_t k = 0; k < 0xFFFFFFFFu; ++k) {
    const uint64_t t = wt.at(k);
    if (t >= wt.end) break;
    const uint64_t stripe = t / a.nwin;
    const uint64_t w = t - stripe * a.nwin;
    const uint64_t off = w * kWindowBytes;
    if ((k & 63u) == 0) {  // pattern indices of the next 64 tasks, one vector load
      const uint64_t tl = wt.at(k + static_cast<uint32_t>(lane));
      patv = tl < wt.end ? a.pat[tl / a.nwin] : 0;
    }
    const ConstPlanPtr pl = plans + __builtin_amdgcn_readlane(patv, static_cast<int>(k & 63u));
    const int nin = pl->nin;
    const int nout = pl->nout;
    // written out, not through helpers, like decode_crc_kernel (its register notes)
    const uint8_t* sb = a.base + stripe * a.stripe_stride + off;
    uint32_t rows[NINB][8];
#pragma unroll
    for (int r = 0; r < NINB; ++r)
      if (r < nin) load_row(sb + static_cast<uint64_t>(pl->loc[r]) * a.row_stride, lane, rows[r]);
    uint32_t acc[NOUT][8];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[o][q] = 0u;
#pragma unroll
    for (int r = 0; r < NINB; ++r)
      if (r < nin) accumulate_row<NOUT, NINB>(acc, rows[r], pl->cw[r]);
    uint8_t* ob = a.out + stripe * a.out_stripe_stride + off;
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      if (o < nout) {
        bitslice(acc[o]);
        store_row(ob + static_cast<uint64_t>(o) * a.out_row_stride, lane, acc[o]);
      }
    }
    // nout is wave-uniform (a scalar load): one branch, then the present
    // outputs' chains in lockstep; a lossless stripe does nothing
    if (nout == 1) bc_crc_outputs<1, NOUT>(d, stripe, w, lane, slices, zchunk, tree, acc);
    if constexpr (NOUT >= 2)
      if (nout == 2) bc_crc_outputs<2, NOUT>(d, stripe, w, lane, slices, zchunk, tree, acc);
    if constexpr (NOUT >= 3)
      if (nout == 3) bc_crc_outputs<3, NOUT>(d, stripe, w, lane, slices, zchunk, tree, acc);
    if constexpr (NOUT >= 4)
      if (nout == 4) bc_crc_outputs<4, NOUT>(d, stripe, w, lane, slices, zchunk, tree, acc);
  }
}

// crc_fold_kernel (hrs_crc.hip) for a batch: pair (stripe, t) with
// t >= the stripe's loss count has no raw words; its CRC continues over no
// bytes, crc_out = crc_in (0 without one), and raw is not read.
__global__ void __launch_bounds__(256) batch_crc_fold_kernel(const BatchCrcFoldArgs b) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const CrcFoldArgs& a = b.f;
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
  for (uint64_t sr = wave_id_in_grid(); sr < a.nsr; sr += nwaves) {
    const uint64_t stripe = sr / b.rows_per_stripe;
    const int t = static_cast<int>(sr - stripe * b.rows_per_stripe);
    const uint32_t start = a.crc_in ? a.crc_in[sr] : 0u;
    if (t >= b.plans[b.pat[stripe]].nout) {  // wave-uniform
      if (lane == 0) a.crc_out[sr] = start;
      continue;
    }
    const uint32_t* raw = a.raw + sr * wpr;
    uint32_t c = 0;
    for (int g = 0; g < a.G; ++g) {
      const int64_t w = static_cast<int64_t>(lane) * a.G + g - static_cast<int64_t>(pad);
      if (w >= 0) c = zmul(zw, c) ^ raw[w];
    }
    c = lane_tree(ztree, c);
    if (lane == 0) {
      if (a.tail) c = zmul(ztail, c) ^ raw[a.nwin];
      a.crc_out[sr] = zmul(zlen, start ^ 0xFFFFFFFFu) ^ c ^ 0xFFFFFFFFu;
    }
  }
}

// 768 threads (3 waves/SIMD): every instantiation fits that budget's 168
// VGPRs without scratch (at most 146). HRS_BCRC_THREADS=512
// for A/B runs.
int bcrc_threads() {
  static const int v = [] {
    const char* e = getenv("HRS_BCRC_THREADS");
    return (e && atoi(e) == 512) ? 512 : 768;
  }();
  return v;
}

template <int NOUT, int NINB>
hipError_t launch_bc(const BatchCrcArgs& d, int cus, hipStream_t s) {
  BatchCrcArgs dc = d;
  dc.b.order = task_order(kOrderDecodeCrc);
  const int threads = bcrc_threads();
  auto kern = threads == 768 ? batch_decode_crc_kernel<NOUT, NINB, 768> : batch_decode_crc_kernel<NOUT, NINB, 512>;
  const size_t shm = static_cast<size_t>(kCrcLdsWordsA) * 4;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(shm));
  if (e != hipSuccess) return e;
  note_kernel_t("batch_decode_crc_kernel", NOUT, NINB, threads);
  const uint64_t per_block = threads / 64;
  uint64_t g = (d.b.ntasks + per_block - 1) / per_block;
  if (g > static_cast<uint64_t>(cus)) g = cus;
  g = capped_grid(g);  // zero-copy calls cap it (hrs::GridCap)
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(g)), dim3(threads), shm, s, dc);
  return hipGetLastError();
}

template <int NOUT>
hipError_t launch_bc_n(const BatchCrcArgs& d, int max_nin, int cus, hipStream_t s) {
  if (max_nin <= 4) return launch_bc<NOUT, 4>(d, cus, s);
  if (max_nin <= 8) return launch_bc<NOUT, 8>(d, cus, s);
  if constexpr (NOUT <= 3) {
    if (max_nin <= 12) return launch_bc<NOUT, 12>(d, cus, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_batch_decode_crc(const BatchCrcArgs& d, int max_nout, int max_nin, int cus, hipStream_t s) {
  switch (max_nout) {
    case 1: return launch_bc_n<1>(d, max_nin, cus, s);
    case 2: return launch_bc_n<2>(d, max_nin, cus, s);
    case 3: return launch_bc_n<3>(d, max_nin, cus, s);
    case 4: return launch_bc_n<4>(d, max_nin, cus, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_batch_crc_fold(const BatchCrcFoldArgs& b, int cus, hipStream_t s) {
  uint64_t blocks = (b.f.nsr + 3) / 4;
  const uint64_t cap = static_cast<uint64_t>(cus) * kCrcFoldBlocksPerCU;
  if (blocks > cap) blocks = cap;
  const size_t shm = static_cast<size_t>(kCrcLdsWordsB) * 4;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(batch_crc_fold_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(shm));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(batch_crc_fold_kernel, dim3(static_cast<unsigned>(blocks ? blocks : 1)), dim3(256), shm, s, b);
  return hipGetLastError();
}

}  // namespace hrs
