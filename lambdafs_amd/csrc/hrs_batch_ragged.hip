// Ragged repair batches (hrs_decode_batch_ragged_dev / _host): the repair
// batch of hrs_batch.hip over cells of which only the leading bytes hold data.
//
// The reference hands decodeBulk full buffers: a survivor past the end of the
// file is a ZeroInputStream (StripeReader.java:111-120), a short read is
// zero-filled by RaidUtils.readTillEnd, and the repaired block is written only
// up to the lost block's real length (Decoder.java:345-369). Here every cell's
// length arrives in a per-call table in PLAN order (hrs_batch_ragged.hpp) and
// the zeros are never read or written: a 2 KiB window of a survivor that lies
// wholly at or beyond its length costs no load and no bit-slice, the one
// window that holds the boundary is loaded and masked, an output is stored
// only below its length, and a task whose outputs are all dead loads nothing.
//
// batch_ragged_kernel<NOUT, NINB> is batch_bitsliced_kernel's walk: one wave
// per window, wave_tasks, the pattern indices of the next 64 tasks in one
// vector load, the plan through the constant address space, load_row /
// store_row, accumulate_row. A task's lengths are wave-uniform scalar reads at
// stripe * words + r; the row cases (full, boundary, dead) are wave-uniform
// branches. batch_ragged_bytewise_kernel is batch_bytewise_kernel's shape:
// correct for every plan, layout and alignment and fast for none.
#include <hip/hip_runtime.h>

#include "hrs_batch_ragged.hpp"
#include "hrs_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_ragged_device.hpp"

namespace hrs {
namespace {

__constant__ gf::Tables d_batch_ragged_tables = gf::make_tables();

typedef const __attribute__((address_space(4))) BatchPlan* ConstPlanPtr;

// Rows whose loads are in flight together: all NINB of the plan, as in
// batch_bitsliced_kernel (no instantiation needs scratch for it: `make
// ragged_repair_resources`; groups of NINB / 2 rows ran the full batch 26 %
// behind the plain kernel, profiles/ragged_repair/bench_ragged_repair_first_run.json).
// A group's live rows are all loaded before its math, so the branches around
// the loads do not serialise their waits.
template <int NINB>
struct BatchRaggedGroup {
  static constexpr int value = NINB;
};

template <int NOUT, int NINB>
__global__ void __launch_bounds__(kBlockThreads) batch_ragged_kernel(const BatchRaggedArgs a) {
  const int lane = threadIdx.x & 63;
  const ConstPlanPtr plans = (ConstPlanPtr)a.b.plans;
  int patv = 0;
  const WaveTasks wt = wave_tasks(a.b.ntasks, a.b.order);
  for (uint32_t k = 0;; ++k) {
    const uint64_t t = wt.at(k);
    if (t >= wt.end) break;
    const uint64_t stripe = t / a.b.nwin;
    const uint64_t off = (t - stripe * a.b.nwin) * kWindowBytes;
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
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      olive[o] = window_live(uniform_word(lw + a.nin_words + o), lo);
      any |= olive[o];
    }
    if (any == 0u) continue;  // every output dead: nothing loaded, nothing stored
    const uint8_t* sb = a.b.base + stripe * a.b.stripe_stride + off;
    uint32_t acc[NOUT][8];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[o][q] = 0u;
    constexpr int G = BatchRaggedGroup<NINB>::value;
#pragma unroll
    for (int g0 = 0; g0 < NINB; g0 += G) {
      uint32_t live[G];  // 0 past the batch's max_nin and past the plan's nin
      uint32_t w[G][8];
#pragma unroll
      for (int i = 0; i < G; ++i)
        live[i] = g0 + i < a.nin_words ? window_live(uniform_word(lw + g0 + i), lo) : 0u;
#pragma unroll
      for (int i = 0; i < G; ++i)
        if (live[i]) load_row(sb + static_cast<uint64_t>(pl->loc[g0 + i]) * a.b.row_stride, lane, w[i]);
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (!live[i]) continue;  // zero planes: no load, no bit-slice, nothing to add
        if (live[i] < kWindowBytes) mask_row(w[i], lane, live[i]);
        accumulate_row<NOUT, NINB>(acc, w[i], pl->cw[g0 + i]);
      }
    }
    uint8_t* ob = a.b.out + stripe * a.b.out_stripe_stride + off;
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      if (!olive[o]) continue;
      bitslice(acc[o]);
      uint8_t* p = ob + static_cast<uint64_t>(o) * a.b.out_row_stride;
      if (olive[o] == kWindowBytes)
        store_row(p, lane, acc[o]);
      else
        store_row_below(p, lane, acc[o], olive[o]);
    }
  }
}

// Byte columns [col0, len) of every stripe. A column at or beyond a survivor's
// length reads nothing of that row; a column at or beyond an output's length
// stores nothing to it, and one beyond every output's reads nothing at all.
__global__ void __launch_bounds__(kBlockThreads) batch_ragged_bytewise_kernel(const BatchRaggedArgs a) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  for (int i = threadIdx.x; i < 512; i += blockDim.x) s_exp[i] = d_batch_ragged_tables.exp[i];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_log[i] = d_batch_ragged_tables.log[i];
  __syncthreads();
  const uint64_t ncol = a.b.len - a.b.col0;
  const uint64_t nthreads = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < a.b.ntasks;
       idx += nthreads) {
    const uint64_t stripe = idx / ncol;
    const uint64_t col = a.b.col0 + (idx - stripe * ncol);
    const BatchPlan& pl = a.b.plans[a.b.pat[stripe]];
    const uint32_t* lw = a.lens + stripe * static_cast<uint64_t>(a.words);
    const uint32_t* ow = lw + a.nin_words;
    bool wanted = false;
    for (int o = 0; o < pl.nout; ++o) wanted |= col < ow[o];
    if (!wanted) continue;
    const uint8_t* sb = a.b.base + stripe * a.b.stripe_stride + col;
    uint8_t acc[kMaxOut] = {};
    for (int r = 0; r < pl.nin; ++r) {
      if (col >= lw[r]) continue;
      const uint8_t x = sb[static_cast<uint64_t>(pl.loc[r]) * a.b.row_stride];
      if (x == 0) continue;
      const int lx = s_log[x];
      const uint64_t w = pl.cw[r];
#pragma unroll
      for (int o = 0; o < kMaxOut; ++o) {
        const uint8_t c = static_cast<uint8_t>(w >> (8 * o));
        if (c != 0) acc[o] ^= s_exp[lx + s_log[c]];
      }
    }
    uint8_t* ob = a.b.out + stripe * a.b.out_stripe_stride + col;
    for (int o = 0; o < pl.nout; ++o)
      if (col < ow[o]) ob[static_cast<uint64_t>(o) * a.b.out_row_stride] = acc[o];
  }
}

// launch_batch_n's geometry (hrs_batch.hip): 3 blocks per CU for the rolled bit loop, else 2.
template <int NOUT, int NINB>
hipError_t launch_batch_ragged_n(const BatchRaggedArgs& a, hipStream_t s) {
  note_kernel_t("batch_ragged_kernel", NOUT, NINB);
  const int per_cu = BitLoop<NOUT, NINB>::kRolled ? 3 : 2;
  BatchRaggedArgs b = a;
  b.b.order = task_order(kOrderBatch);
  hipLaunchKernelGGL((batch_ragged_kernel<NOUT, NINB>), dim3(stream_grid(a.b.ntasks, per_cu)), dim3(kBlockThreads), 0,
                     s, b);
  return hipGetLastError();
}

template <int NOUT>
hipError_t launch_batch_ragged_nout(const BatchRaggedArgs& a, int max_nin, hipStream_t s) {
  if (max_nin <= 4) return launch_batch_ragged_n<NOUT, 4>(a, s);
  if (max_nin <= 8) return launch_batch_ragged_n<NOUT, 8>(a, s);
  if (max_nin <= 12) return launch_batch_ragged_n<NOUT, 12>(a, s);
  return launch_batch_ragged_n<NOUT, 16>(a, s);
}

}  // namespace

hipError_t launch_batch_ragged(const BatchRaggedArgs& a, int max_nout, int max_nin, hipStream_t s) {
  if (!batch_ragged_vector_shape(max_nout, max_nin)) return hipErrorInvalidValue;
  switch (max_nout) {
    case 1: return launch_batch_ragged_nout<1>(a, max_nin, s);
    case 2: return launch_batch_ragged_nout<2>(a, max_nin, s);
    case 3: return launch_batch_ragged_nout<3>(a, max_nin, s);
    default: return launch_batch_ragged_nout<4>(a, max_nin, s);
  }
}

hipError_t launch_batch_ragged_bytewise(const BatchRaggedArgs& a, hipStream_t s) {
  const unsigned g = grid_for(batch_ragged_bytewise_kernel, kBlockThreads, a.b.ntasks);
  note_kernel("batch_ragged_bytewise_kernel");
  hipLaunchKernelGGL(batch_ragged_bytewise_kernel, dim3(g), dim3(kBlockThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace hrs
