// Device code shared by the scrub and heal kernels and their fused CRC forms
// (hrs_scrub.hip, hrs_scrub_crc.hip): the locator's field tables, the
// per-wave report histograms, the Horner step over a bit-sliced row, the walk
// over a dirty window's bad columns, the report rule of one bad column and the
// byte-granular kernels' task arithmetic. Every piece is forced inline: no
// kernel of the family makes a call.
#pragma once
#include <hip/hip_runtime.h>

#include "hrs_device.hpp"
#include "hrs_locator.hpp"

namespace hrs {

// The units are separate code objects: one copy of the tables in each.
static __constant__ gf::Tables d_field_tables = gf::make_tables();

// exp / log into LDS (768 bytes), by the block's `nthreads` threads.
__device__ __forceinline__ void load_field_tables(uint8_t* s_exp, uint8_t* s_log, int nthreads) {
  for (int i = threadIdx.x; i < 512; i += nthreads) s_exp[i] = d_field_tables.exp[i];
  for (int i = threadIdx.x; i < 256; i += nthreads) s_log[i] = d_field_tables.log[i];
}

// ---- per-wave report histograms: `words_per_wave` words each, laid out as a
// report (word 2 is a minimum and rests at kScrubNone, the others are counts).

__device__ __forceinline__ void hist_init(uint32_t* hist_base, int words_per_wave, int nwaves) {
  for (int i = threadIdx.x; i < nwaves * words_per_wave; i += nwaves * 64)
    hist_base[i] = i % words_per_wave == 2 ? kScrubNone : 0u;
}

// A window's counts to its stripe's report (a wave's consecutive windows can
// belong to different stripes); the exchange re-arms the histogram.
__device__ __forceinline__ void hist_flush(uint32_t* hist, uint32_t* rep, int nwords, int lane) {
  __builtin_amdgcn_wave_barrier();
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

// ---- syndromes of a window

// One Horner step of the P syndromes over the sliced row w (rows are taken
// from location n - 1 down to 0): acc_i <- alpha^i acc_i + w.
template <int P>
__device__ __forceinline__ void horner_sliced(uint32_t (&acc)[P][8], const uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < P; ++i) {
#pragma unroll
    for (int r = 0; r < i; ++r) xtime(acc[i]);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[i][q] ^= w[q];
  }
}

// The lane's 32 columns of a dirty window are bytes 0..3 of words 0..7 of the
// un-sliced syndrome planes; word x covers window bytes (x >> 2) * 1024 +
// lane * 16 + (x & 3) * 4. Calls fn(s, col, x, b) on every column whose P
// syndrome bytes s are not all zero, col = off + its window byte. The planes
// are picked by select chains, so they stay in registers.
template <int P, class Fn>
__device__ __forceinline__ void for_each_bad_column(const uint32_t (&acc)[P][8], uint32_t off, int lane, Fn&& fn) {
  // The select chains run over a local copy: over a reference parameter they
  // are folded into one indexed load before this function is inlined, and the
  // caller's planes then live in scratch.
  uint32_t sy[P][8];
#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int q = 0; q < 8; ++q) sy[i][q] = acc[i][q];
#pragma unroll 1
  for (int x = 0; x < 8; ++x) {
    uint32_t cur[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
      uint32_t v = sy[i][0];
#pragma unroll
      for (int q = 1; q < 8; ++q) v = (x == q) ? sy[i][q] : v;
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
      const uint32_t col = off + (x >> 2) * 1024u + lane * 16u + (x & 3) * 4u + b;
      fn(s, col, x, b);
    }
  }
}

// ---- the report rule

// One bad column into the counters at h: a per-wave LDS histogram or the
// stripe's report itself. `resolved`: the locator blamed loc[0..nloc) with
// error values err[]. Heal: a resolved column is also written back,
// data[loc[j]] ^= err[j] at rows[loc[j]] + at (ReedSolomonCode.java:281-285),
// one byte load, XOR and byte store per nonzero error value, counted in word
// 3. An unresolved column is not touched (the Java returns false after writing
// it; include/hrs.h). The column belongs to this lane alone, so the stores
// race with nothing.
//
// ConstIndex picks the form of the loops over the blamed locations. A locator
// of degree P / 2 has at most P / 2 roots, so nloc <= P / 2 <= kMaxErrors. true: the
// loops run to that bound with constant indices and test j < nloc, which keeps
// loc / err in registers; the fused kernels need it to stay without scratch.
// false: the loops run to nloc, the form the scrub and heal kernels have
// always had (DESIGN 10.1 says why they keep it).
template <int P, bool Heal, bool ConstIndex>
__device__ __forceinline__ void account_column(uint32_t* h, uint32_t col, bool resolved, int nloc,
                                               const uint8_t (&loc)[locator::kMaxErrors],
                                               const uint8_t (&err)[locator::kMaxErrors], const uint8_t* const* rows,
                                               uint64_t at) {
  static_assert(P / 2 <= locator::kMaxErrors, "loc / err hold a locator's roots");
  const int bound = ConstIndex ? P / 2 : nloc;
  constexpr int kUnroll = ConstIndex && P >= 2 ? P / 2 : 1;  // 1: the loop stays a loop
  atomicAdd(&h[0], 1u);
  atomicMin(&h[2], col);
  if (!resolved) {
    atomicAdd(&h[1], 1u);
  } else {
#pragma unroll kUnroll
    for (int j = 0; j < bound; ++j)
      if (j < nloc) atomicAdd(&h[kScrubHead + loc[j]], 1u);
    if constexpr (Heal) {
      uint32_t patched = 0u;
#pragma unroll kUnroll
      for (int j = 0; j < bound; ++j)
        if (j < nloc && err[j] != 0) {
          uint8_t* q = const_cast<uint8_t*>(rows[loc[j]]) + at;
          *q = static_cast<uint8_t>(*q ^ err[j]);
          ++patched;
        }
      if (patched != 0u) atomicAdd(&h[kScrubPatched], patched);
    }
  }
}

// count_column of the scrub and heal kernels: the locator on the syndromes s
// (not all zero) of column col, then the report rule.
template <int P, bool Heal, bool ConstIndex = false>
__device__ __forceinline__ void count_column(const locator::Field& f, int n, const uint8_t (&s)[P], uint32_t col,
                                             uint32_t* h, const uint8_t* const* rows, uint64_t at) {
  int nloc = 0;
  uint8_t loc[locator::kMaxErrors], err[locator::kMaxErrors];
  const bool resolved = locator::locate(f, n, P, s, &nloc, loc, err);
  account_column<P, Heal, ConstIndex>(h, col, resolved, nloc, loc, err, rows, at);
}

// ---- byte-granular kernels: one column per lane (rows or strides that are
// not 16-byte aligned, the row tail len % 2 KiB, kernel mode 2)

struct BytewiseTask {
  uint64_t stripe, col, at;  // rows[l][at] is the column's byte of location l
};

// Task idx = stripe * (len - col0) + (column - col0).
__device__ __forceinline__ BytewiseTask bytewise_task(const ScrubArgs& a, uint64_t idx) {
  const uint64_t wlen = a.len - a.col0;
  const uint64_t stripe = idx / wlen;
  const uint64_t col = a.col0 + (idx - stripe * wlen);
  return {stripe, col, stripe * a.stride + col};
}

// The column's syndromes, Horner from location n - 1 down.
template <int P>
__device__ __forceinline__ void bytewise_syndromes(const locator::Field& f, const ScrubArgs& a, uint64_t at,
                                                   uint8_t (&s)[P]) {
#pragma unroll
  for (int i = 0; i < P; ++i) s[i] = 0;
  for (int l = a.n - 1; l >= 0; --l) locator::horner_step<P>(f, s, a.rows[l][at]);
}

}  // namespace hrs
