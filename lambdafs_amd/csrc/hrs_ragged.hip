// Ragged encode kernels (hrs_encode_ragged_dev, hrs_encode_ragged_batch_host).
//
// The reference zero-fills what a stripe's source has no bytes for
// (RaidUtils.readTillEnd, the ZeroInputStream of FileStripeReader) and hands
// encodeBulk full buffers; ParallelStreamReader.ReadResult.numRead says how
// many bytes of each were real. Here that count arrives as valid[s * k + j]
// and the zeros are never stored or read: a 2 KiB window of a data cell that
// lies wholly at or beyond `valid` contributes zero planes to the XOR network
// without a load, the one window that holds the boundary is loaded and
// masked, and bytes at or beyond `valid` never reach an output.
//
// encode_ragged_kernel<K, P> is encode_static_body's walk (hrs_kernels.hip):
// one wave per window, wave_tasks, nontemporal row accesses, the compile-time
// XOR network, the same grid and task order. The K valid words of a task are
// wave-uniform and come through the scalar path; the three row cases (full,
// boundary, dead) are wave-uniform branches around the loads and around the
// bit-slice, the network itself (has / pend) does not depend on them. The rs
// and nrs families are the same template over their compile-time matrix; the
// two sets of kernels carry one name in the namespaces rs and nrs.
//
// encode_ragged_bytewise_kernel is bytewise_kernel's shape: one byte column
// per lane, tables in LDS, a run-time matrix. It is correct for every code,
// shape and alignment and fast for none: it serves the row tail below 2 KiB,
// unaligned layouts, kernel mode 2 and every code without a static network.
#include <hip/hip_runtime.h>

#include "hrs_device.hpp"
#include "hrs_launch.hpp"
#include "hrs_ragged.hpp"

namespace hrs {
namespace {

__constant__ gf::Tables d_ragged_tables = gf::make_tables();

// A word every lane of the wave reads from one address: constant address
// space (the table does not change under the kernel) and a uniform address, so
// the load is scalar and the value lives in an SGPR.
typedef __attribute__((address_space(4))) const uint32_t c_u32;

__device__ __forceinline__ uint32_t uniform_word(const uint32_t* p) {
  return __builtin_amdgcn_readfirstlane(*reinterpret_cast<c_u32*>(uniform_addr(p)));
}

// Clears the bytes at or beyond `nbytes` (0 < nbytes < 2 KiB) of the lane's
// words of a window (load_row's layout: words 0-3 at 16 lane, 4-7 1 KiB later).
__device__ __forceinline__ void mask_row(uint32_t (&w)[8], int lane, uint32_t nbytes) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int at = (i < 4 ? 0 : 1024) + lane * 16 + (i & 3) * 4;
    const int d = static_cast<int>(nbytes) - at;  // data bytes of this word
    w[i] &= d >= 4 ? 0xFFFFFFFFu : d <= 0 ? 0u : (1u << (8 * d)) - 1u;
  }
}

// Rows whose loads are in flight together: all of a narrow code, half of a
// wide one (12 rows at once would not fit the register file without scratch).
template <int K>
struct RaggedGroup {
  static constexpr int value = K <= 6 ? K : (K + 1) / 2;
};

template <int K, int P, class MATRIX>
__device__ __forceinline__ void encode_ragged_body(const RaggedArgs& a) {
  const int lane = threadIdx.x & 63;
  const WaveTasks wt = wave_tasks(a.r.ntasks, a.r.order);
  for (uint32_t j = 0; j < 0xFFFFFFFFu; ++j) {
    const uint64_t t = wt.at(j);
    if (t >= wt.end) break;
    const uint64_t stripe = t / a.r.nwin;
    const uint64_t off = (t - stripe * a.r.nwin) * kWindowBytes;
    const uint32_t lo = static_cast<uint32_t>(off);  // len <= UINT32_MAX (the entry points)
    const uint32_t* v = a.valid + stripe * K;
    // data bytes of row r inside this window: 0 dead, 2048 full, else the boundary
    uint32_t live[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const uint32_t vr = uniform_word(v + r);
      const uint32_t d = vr > lo ? vr - lo : 0u;
      live[r] = d < kWindowBytes ? d : kWindowBytes;
    }
    uint32_t acc[P][8];
    uint32_t pend[P][8];
    bool has[P][8];  // compile-time after unrolling
#pragma unroll
    for (int o = 0; o < P; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        acc[o][q] = 0u;
        pend[o][q] = 0u;
        has[o][q] = false;
      }
    // rows in groups of G: a group's live rows are all loaded before its math,
    // so the branches around the loads do not serialise them
    constexpr int G = RaggedGroup<K>::value;
#pragma unroll
    for (int g0 = 0; g0 < K; g0 += G) {
      uint32_t w[G][8];
#pragma unroll
      for (int i = 0; i < G; ++i)
        if (g0 + i < K && live[g0 + i])
          load_row(a.r.in[g0 + i] + stripe * a.r.in_stride + off, lane, w[i]);
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (g0 + i >= K) continue;
        const int r = g0 + i;
        if (live[r]) {
          if (live[r] < kWindowBytes) mask_row(w[i], lane, live[r]);
          bitslice(w[i]);
        } else {
#pragma unroll
          for (int q = 0; q < 8; ++q) w[i][q] = 0u;  // zero planes: no load, no bit-slice
        }
        encode_row_acc<K, P, MATRIX>(r, w[i], acc, pend, has);
      }
    }
#pragma unroll
    for (int o = 0; o < P; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (has[o][q]) acc[o][q] ^= pend[o][q];
#pragma unroll
    for (int o = 0; o < P; ++o) {
      bitslice(acc[o]);
      store_row(a.r.out[o] + stripe * a.r.out_stride + off, lane, acc[o]);
    }
  }
}

namespace rs {  // the hops generator rows (ReedSolomonCode)
template <int K, int P>
__global__ void __launch_bounds__(kBlockThreads) encode_ragged_kernel(const RaggedArgs a) {
  encode_ragged_body<K, P, gf::EncodeMatrix<K, P>>(a);
}
}  // namespace rs

namespace nrs {  // the Cauchy rows of ISA-L gf_gen_cauchy1_matrix (NativeReedSolomonCode)
template <int K, int P>
__global__ void __launch_bounds__(kBlockThreads) encode_ragged_kernel(const RaggedArgs a) {
  encode_ragged_body<K, P, gf::CauchyMatrix<K, P>>(a);
}
}  // namespace nrs

// One byte column per lane over columns [col0, len) of every stripe. A column
// at or beyond a row's valid count reads nothing of that row.
__global__ void __launch_bounds__(kBlockThreads) encode_ragged_bytewise_kernel(const RaggedArgs a) {
  __shared__ uint8_t s_exp[512];
  __shared__ uint8_t s_log[256];
  for (int i = threadIdx.x; i < 512; i += blockDim.x) s_exp[i] = d_ragged_tables.exp[i];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_log[i] = d_ragged_tables.log[i];
  __syncthreads();
  const uint64_t span = a.r.len - a.col0;
  const uint64_t nthreads = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < a.r.ntasks;
       idx += nthreads) {
    const uint64_t stripe = idx / span;
    const uint64_t col = a.col0 + (idx - stripe * span);
    const uint32_t* v = a.valid + stripe * a.k + a.row0;
    uint8_t acc[kMaxOut];
#pragma unroll
    for (int o = 0; o < kMaxOut; ++o)
      acc[o] = (a.r.accumulate && o < a.r.nout) ? a.r.out[o][stripe * a.r.out_stride + col] : 0;
    for (int r = 0; r < a.r.nin; ++r) {
      if (a.r.cw[r] == 0 || col >= v[r]) continue;
      const uint8_t x = a.r.in[r][stripe * a.r.in_stride + col];
      if (x == 0) continue;
      const int lx = s_log[x];
#pragma unroll
      for (int o = 0; o < kMaxOut; ++o) {
        const uint8_t c = static_cast<uint8_t>(a.r.cw[r] >> (8 * o));
        if (o < a.r.nout && c != 0) acc[o] ^= s_exp[lx + s_log[c]];
      }
    }
#pragma unroll
    for (int o = 0; o < kMaxOut; ++o)
      if (o < a.r.nout) a.r.out[o][stripe * a.r.out_stride + col] = acc[o];
  }
}

template <int K, int P, class Kernel>
hipError_t launch_ragged(Kernel kern, const RaggedArgs& a, hipStream_t s) {
  note_kernel_t("encode_ragged_kernel", K, P);
  RaggedArgs b = a;
  b.r.order = task_order(kOrderStaticEncode);
  hipLaunchKernelGGL(kern, dim3(stream_grid(a.r.ntasks)), dim3(kBlockThreads), 0, s, b);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_ragged_encode(int family, int k, int p, const RaggedArgs& a, hipStream_t s, bool* handled) {
  *handled = true;
  if (family == kStaticCauchy) {
    if (k == 10 && p == 4) return launch_ragged<10, 4>(nrs::encode_ragged_kernel<10, 4>, a, s);
    if (k == 6 && p == 3) return launch_ragged<6, 3>(nrs::encode_ragged_kernel<6, 3>, a, s);
    *handled = false;
    return hipSuccess;
  }
  if (k == 10 && p == 4) return launch_ragged<10, 4>(rs::encode_ragged_kernel<10, 4>, a, s);
  if (k == 6 && p == 3) return launch_ragged<6, 3>(rs::encode_ragged_kernel<6, 3>, a, s);
  if (k == 3 && p == 2) return launch_ragged<3, 2>(rs::encode_ragged_kernel<3, 2>, a, s);
  if (k == 12 && p == 4) return launch_ragged<12, 4>(rs::encode_ragged_kernel<12, 4>, a, s);
  *handled = false;
  return hipSuccess;
}

hipError_t launch_ragged_bytewise(const RaggedArgs& a, hipStream_t s) {
  const unsigned g = grid_for(encode_ragged_bytewise_kernel, kBlockThreads, a.r.ntasks);
  note_kernel("encode_ragged_bytewise_kernel");
  hipLaunchKernelGGL(encode_ragged_bytewise_kernel, dim3(g), dim3(kBlockThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace hrs
