// Checked repair (hrs_repair_checked_dev / hrs_repair_checked_host,
// include/hrs.h): the one statement of its rule, compiled by the host call
// (hrs_scrub_api.cpp) and by the kernels (hrs_repair.hip), the way
// hrs_locator.hpp is shared: which cells a stripe doubts, what becomes of the
// stripe before the repair (plan_verdict), what the repair's outcome is called
// (final_verdict), and the table entry of an erased set (fill_pattern), which
// the plan kernel builds on the device and make_pattern on the host.
#pragma once
#include <cstdint>

#include "gf256.hpp"
#include "hrs_heal_erased.hpp"
#include "hrs_locator.hpp"

namespace hrs {
namespace repair {

// HRS_REPAIR_* of include/hrs.h; kListed never leaves the library.
enum Verdict : uint32_t {
  kClean = 0,
  kRepaired = 1,
  kRestamp = 2,
  kFailed = 3,
  kTooMany = 4,
  kAmbiguous = 5,
  kListed = 0xFFFFFFFFu,  // goes to the second pass with the erased set B
};

constexpr int kJoinSyndromes = 1;  // HRS_REPAIR_JOIN_SYNDROMES

// Step 1: cell l is in D when its CRC as read differs from the stored one.
HRS_HD inline bool doubted(uint32_t crc, uint32_t stored) { return crc != stored; }

// Step 2: cell l is in B when it is in D or, with the join flag, pass 1's
// report blamed it in some resolved column (word 4 + l).
HRS_HD inline bool suspected(uint32_t crc, uint32_t stored, uint32_t blamed, int flags) {
  return doubted(crc, stored) || ((flags & kJoinSyndromes) != 0 && blamed != 0u);
}

// Step 3, in its order: nd = |D|, nb = |B|, bad / unresolved = words 0 / 1 of
// pass 1's report.
HRS_HD inline uint32_t plan_verdict(int nd, int nb, int p, uint32_t bad, uint32_t unresolved) {
  if (nd == 0 && unresolved > 0u) return kAmbiguous;
  if (nd == 0 && bad == 0u) return kClean;
  if (nb > p) return kTooMany;
  return kListed;
}

// Step 6 over a listed stripe: any_f: some cell's CRC after the repair differs
// from the stored one (F is not empty); any_fd: one of those cells was in D;
// unresolved = word 1 of the repair's report.
HRS_HD inline uint32_t final_verdict(bool any_f, bool any_fd, uint32_t unresolved) {
  if (!any_f) return kRepaired;
  if (!any_fd && unresolved == 0u) return kRestamp;
  return kFailed;
}

// Working room of fill_pattern, kept out of the builder's frame so that the
// kernel can hand in LDS (indexed local arrays would become scratch memory).
struct PatternWork {
  uint8_t a[locator::kMaxErased][2 * locator::kMaxErased];  // [V | I] -> [I | V^-1]
  uint8_t mat[locator::kMaxSyndromes][locator::kMaxSyndromes];
};

// Completes the table entry of an erased set (hrs_heal_erased.hpp): pt.e and
// pt.loc[0..e) (ascending, distinct, e <= p) are given and every other byte of
// pt is zero; fills mask, spare, gamma and the packed matrix cw. The inverse of
// the e x e Vandermonde matrix alpha^(loc[m] i) is a Gauss-Jordan elimination
// (distinct locations: a pivot always exists).
HRS_HD inline void fill_pattern(const locator::Field& f, int p, ErasePattern& pt, PatternWork& w) {
  const int e = pt.e, pp = p - e;
  for (int m = 0; m < e; ++m) pt.mask[pt.loc[m] >> 5] |= 1u << (pt.loc[m] & 31);
  uint32_t spare = 0;
  while ((pt.mask[spare >> 5] >> (spare & 31)) & 1u) ++spare;
  pt.spare = spare;
  locator::erasure_locator(f, e, pt.loc, pt.gamma);
  for (int o = 0; o < p; ++o)
    for (int i = 0; i < p; ++i) w.mat[o][i] = 0;
  for (int o = 0; o < pp; ++o)
    for (int j = 0; j <= e; ++j) w.mat[o][o + e - j] = pt.gamma[j];
  for (int i = 0; i < e; ++i)
    for (int m = 0; m < e; ++m) {
      w.a[i][m] = locator::fpow(f, static_cast<int>(pt.loc[m]) * i);
      w.a[i][e + m] = i == m ? 1 : 0;
    }
  for (int col = 0; col < e; ++col) {
    int piv = col;
    while (piv < e && w.a[piv][col] == 0) ++piv;
    if (piv == e) return;  // singular: cannot happen for distinct locations
    for (int c = 0; c < 2 * e; ++c) {
      const uint8_t x = w.a[col][c];
      w.a[col][c] = w.a[piv][c];
      w.a[piv][c] = x;
    }
    const uint8_t d = w.a[col][col];
    for (int c = 0; c < 2 * e; ++c) w.a[col][c] = locator::fdiv(f, w.a[col][c], d);
    for (int r = 0; r < e; ++r) {
      const uint8_t lead = w.a[r][col];
      if (r == col || lead == 0) continue;
      for (int c = 0; c < 2 * e; ++c) w.a[r][c] ^= locator::fmul(f, lead, w.a[col][c]);
    }
  }
  for (int m = 0; m < e; ++m)
    for (int i = 0; i < e; ++i) w.mat[pp + m][i] = w.a[m][e + i];
  for (int i = 0; i < p; ++i) {
    uint64_t cw = 0;
    for (int o = 0; o < p; ++o) cw |= static_cast<uint64_t>(w.mat[o][i]) << (8 * o);
    pt.cw[i] = cw;
  }
}

}  // namespace repair
}  // namespace hrs
