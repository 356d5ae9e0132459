// Device code shared by the kernels that heal with known erasures
// (hrs_heal_erased.hip, its listed form there, hrs_heal_erased_crc.hip): the
// wave's copy of its stripe's pattern, the locator on one bad column, the tail
// of a window's walk from tv = M S to the erased rows' values, and the count
// of a device list. Every piece is forced inline: no kernel makes a call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "hrs_device.hpp"
#include "hrs_heal_erased.hpp"
#include "hrs_locator.hpp"

namespace hrs {

// ---- the pattern in the lanes

// The calling wave's copy of its stripe's pattern: lane j % 32 holds dword j
// of the 128-byte table entry (one coalesced load per window); a field comes
// out by v_readlane into an SGPR, so the tests on it run on the scalar unit.
constexpr int kPatE = offsetof(ErasePattern, e) / 4, kPatMask = offsetof(ErasePattern, mask) / 4,
              kPatCw = offsetof(ErasePattern, cw) / 4, kPatLoc = offsetof(ErasePattern, loc) / 4, kPatSpare = offsetof(ErasePattern, spare) / 4;
static_assert(sizeof(ErasePattern) == 128 && offsetof(ErasePattern, cw) % 8 == 0, "one dword per lane of a half wave");

__device__ __forceinline__ uint32_t load_pattern(const ErasePattern* pats, int32_t index, int lane) {
  return reinterpret_cast<const uint32_t*>(pats + index)[lane & 31];
}

__device__ __forceinline__ uint32_t pattern_word(uint32_t pv, int word) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(pv), word));
}

// ---- one bad column

// One column (survivor syndromes s) of a stripe with pattern pt: runs the
// locator, patches the blamed survivors at rows[loc] + at, adds the column to
// the counters at h (a per-wave LDS histogram or the stripe's report) and
// leaves the erased values in v.
template <int P>
__device__ __forceinline__ void heal_column(const locator::Field& f, int n, const uint8_t (&s)[P],
                                            const ErasePattern& pt, uint32_t col, uint32_t* h,
                                            const uint8_t* const* rows, uint64_t at,
                                            uint8_t (&v)[locator::kMaxErased]) {
  int nloc = 0;
  uint8_t loc[locator::kMaxErrors], u[locator::kMaxErrors];
  const int state = locator::locate_errata<P>(f, n, s, pt.e, pt.loc, pt.gamma, &nloc, loc, u, v);
  if (state == locator::kConsistent) return;
  atomicAdd(&h[0], 1u);
  atomicMin(&h[2], col);
  if (state == locator::kUnresolved) {
    atomicAdd(&h[1], 1u);
    return;
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
}

// ---- the tail of a window's walk

// From the sliced survivor syndromes S of the window at column `off` of a
// stripe (its byte 0 of row l at rows[l] + stripe_at) with pattern pv:
// tv = M S, T in rows [0, pp) and the erased values in rows [pp, P). A window
// whose T planes are zero in every lane (one ballot) is clean: its erased
// values are un-sliced and handed out. In any other window the lane that owns
// a bad column runs heal_column on it, with the table entry pats[pat_index()]
// (a callable, so that the index is loaded on this path alone), and replaces
// the column's erased bytes in its registers. Then store_erased(l, w, dirty)
// gets the un-sliced words w of every erased row, l its location, in ascending
// order. Returns whether the window was dirty (wave-uniform).
//
// S is copied and tv lives here: the select chains below run over locals of
// this function (for_each_bad_column of hrs_scrub_device.hpp says what happens
// over a reference parameter).
template <int P, class PatIndex, class StoreErased>
__device__ __forceinline__ bool heal_tail(const locator::Field& f, int n, const uint8_t* const* rows,
                                          const ErasePattern* pats, uint32_t pv, uint64_t stripe_at, uint32_t off,
                                          int lane, uint32_t* hist, const uint32_t (&syn)[P][8], PatIndex&& pat_index,
                                          StoreErased&& store_erased) {
  const int pp = P - static_cast<int>(pattern_word(pv, kPatE));  // wave-uniform, like every field
  uint32_t acc[P][8], tv[P][8];
#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      acc[i][q] = syn[i][q];
      tv[i][q] = 0u;
    }
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
          const uint32_t col = off + (x >> 2) * 1024u + lane * 16u + (x & 3) * 4u + b;
          uint8_t v[locator::kMaxErased] = {};
          heal_column<P>(f, n, s, pats[pat_index()], col, hist, rows, stripe_at + col, v);
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
      store_erased(l, tv[i], dirty);
    }
  return dirty;
}

// ---- device lists (HealListedArgs, hrs_heal_erased.hpp; the kernels of
// hrs_repair.hip walk the same list)

// How many stripes the list names, never more than the batch has.
__device__ __forceinline__ uint32_t listed_count(const uint32_t* list, uint32_t nstripes) {
  const uint32_t count = list[0];
  return count < nstripes ? count : nstripes;
}

}  // namespace hrs
