// Error location of one symbol column, as ReedSolomonCode.computeErrorLocations
// does it (ReedSolomonCode.java:243-287): p syndromes -> p/2 x (p/2 + 1)
// syndrome matrix -> the reference's Gaussian elimination -> locator
// polynomial -> root scan over the n locations -> error values -> re-check.
//
// Host and device share this code: hrs_compute_error_locations runs it over
// gf::make_tables() on the host, the scrub kernels (hrs_scrub.hip) run it on
// the columns whose syndrome is nonzero, over the same tables in LDS.
//
// The reference's behaviour is reproduced, not repaired:
//   - the elimination looks for a pivot along ROW i (matrix[i][j], j >= i) and
//     then swaps rows i and j (GaloisField.java:412-451), so the pivot it
//     divides by may be zero;
//   - a division by zero yields 0 (GaloisField's divTable[x][0]);
//   - p = 1 has no locator root, so any nonzero syndrome is unresolved.
//
// After the root scan the Java zeroes the located symbols, solves a
// Vandermonde system for their values and recomputes every syndrome of the
// patched column. Both steps are linear in the column and the located
// positions are distinct, so the solve is exact and they can be done on the
// syndromes alone: with X_j = alpha^loc_j, solving sum_j e_j X_j^i = S_i for
// i < nloc gives the error values e_j (the Java's value at loc_j is the symbol
// there XOR e_j), and the patched column's syndromes are
// S_i XOR sum_j e_j X_j^i for i < p. The column is never read again.
#pragma once
#include <cstdint>

#include "gf256.hpp"

namespace hrs {
namespace locator {

constexpr int kMaxSyndromes = 8;               // parity_size the scrub supports (kMaxOut)
constexpr int kMaxErrors = kMaxSyndromes / 2;  // locator degree

// log / antilog tables the caller hands in (gf::Tables layout: exp[512], log[256]).
struct Field {
  const uint8_t* exp;
  const uint8_t* log;
};

HRS_HD inline uint8_t fmul(const Field& f, uint8_t a, uint8_t b) {
  return (a == 0 || b == 0) ? 0 : f.exp[f.log[a] + f.log[b]];
}

// a / b with the reference's a / 0 = 0.
HRS_HD inline uint8_t fdiv(const Field& f, uint8_t a, uint8_t b) {
  return (a == 0 || b == 0) ? 0 : f.exp[f.log[a] + 255 - f.log[b]];
}

// alpha^e, e >= 0.
HRS_HD inline uint8_t fpow(const Field& f, int e) { return f.exp[e % 255]; }

// One Horner step of S_i = sum_l alpha^(i l) d_l, taken from location n - 1
// down to 0: S_i <- alpha^i S_i + d.
template <int P>
HRS_HD inline void horner_step(const Field& f, uint8_t (&s)[P], uint8_t d) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < P; ++i) s[i] = static_cast<uint8_t>((s[i] ? f.exp[f.log[s[i]] + i] : 0) ^ d);
}

// The column behind the p syndromes s (not all zero; p <= kMaxSyndromes):
// fills loc[0..*nloc) ascending and the error value err[j] at loc[j], and
// returns what computeErrorLocations returns. n <= 255 locations (the
// nonzero field elements alpha^0 .. alpha^254 are distinct).
HRS_HD inline bool locate(const Field& f, int n, int p, const uint8_t* s, int* nloc, uint8_t* loc, uint8_t* err) {
  const int t = p / 2, w = t + 1;
  uint8_t m[kMaxErrors][kMaxErrors + 1];
  for (int i = 0; i < t; ++i)
    for (int j = 0; j < w; ++j) m[i][j] = s[i + j];
  // GaloisField.gaussianElimination, the row-wise pivot search included
  for (int i = 0; i < t; ++i) {
    int piv = -1;
    for (int j = i; j < t && piv < 0; ++j)
      if (m[i][j] != 0) piv = j;
    if (piv < 0) continue;
    for (int c = 0; c < w; ++c) {
      const uint8_t x = m[i][c];
      m[i][c] = m[piv][c];
      m[piv][c] = x;
    }
    const uint8_t pivot = m[i][i];
    for (int c = i; c < w; ++c) m[i][c] = fdiv(f, m[i][c], pivot);
    for (int r = i + 1; r < t; ++r) {
      const uint8_t lead = m[r][i];
      for (int c = i; c < w; ++c) m[r][c] ^= fmul(f, lead, m[i][c]);
    }
  }
  for (int i = t - 1; i >= 0; --i)
    for (int r = 0; r < i; ++r) {
      const uint8_t lead = m[r][i];
      for (int c = i; c < w; ++c) m[r][c] ^= fmul(f, lead, m[i][c]);
    }
  uint8_t poly[kMaxErrors + 1];
  poly[0] = 1;
  for (int i = 0; i < t; ++i) poly[i + 1] = m[t - 1 - i][t];
  // roots alpha^-l of the locator among the n locations (a polynomial with
  // constant term 1 and degree <= t has at most t of them)
  int found = 0;
  for (int l = 0; l < n; ++l) {
    const uint8_t root = f.exp[255 - l];
    uint8_t v = 0, y = 1;
    for (int j = 0; j < w; ++j) {
      v ^= fmul(f, poly[j], y);
      y = fmul(f, root, y);
    }
    if (v == 0 && found < kMaxErrors) loc[found++] = static_cast<uint8_t>(l);
  }
  *nloc = found;
  if (found == 0) return false;  // nothing patched: the nonzero syndrome stands
  // GaloisField.solveVandermondeSystem on the first `found` syndromes
  uint8_t x[kMaxErrors];
  for (int j = 0; j < found; ++j) {
    x[j] = f.exp[loc[j]];
    err[j] = s[j];
  }
  for (int i = 0; i < found - 1; ++i)
    for (int j = found - 1; j > i; --j) err[j] ^= fmul(f, x[i], err[j - 1]);
  for (int i = found - 1; i >= 0; --i) {
    for (int j = i + 1; j < found; ++j) err[j] = fdiv(f, err[j], static_cast<uint8_t>(x[j] ^ x[j - i - 1]));
    for (int j = i; j < found - 1; ++j) err[j] ^= err[j + 1];
  }
  // the second computeSyndrome, on the patched column
  for (int i = 0; i < p; ++i) {
    uint8_t v = s[i];
    for (int j = 0; j < found; ++j) v ^= fmul(f, err[j], fpow(f, static_cast<int>(loc[j]) * i));
    if (v != 0) return false;
  }
  return true;
}

// ---- errors and erasures together (hrs_heal_erased_*, include/hrs.h)
//
// A column of which the e locations eloc[0..e) (ascending, distinct) are lost
// and the other n - e bytes may carry silent errors. s[0..p) are the syndromes
// of the survivors alone (erased cells counted as zero). With the erasure
// locator Gamma(x) = prod_m (1 + alpha^eloc[m] x) = sum_j gamma[j] x^j the
// modified syndromes T_i = sum_{j <= e} gamma[j] s[i + e - j], i < p - e, hold
// no term of an erased cell: an error u at survivor y adds
// u prod_m (alpha^y + alpha^eloc[m]) alpha^(y i), an error-only syndrome
// sequence of length p - e that locate() takes as it is.

constexpr int kMaxErased = kMaxSyndromes;

enum Errata : int {
  kConsistent = 0,  // every T_i is 0 (or p - e = 0): nobody is blamed
  kResolved = 1,    // locate() returned true and blamed survivors only
  kUnresolved = 2,  // the survivors disagree and cannot be told apart
};

// gamma[0..e] of the erased set.
HRS_HD inline void erasure_locator(const Field& f, int e, const uint8_t* eloc, uint8_t* gamma) {
  gamma[0] = 1;
  for (int m = 0; m < e; ++m) {
    const uint8_t x = f.exp[eloc[m]];
    gamma[m + 1] = 0;
    for (int j = m + 1; j > 0; --j) gamma[j] ^= fmul(f, gamma[j - 1], x);
  }
}

// locate() over the pp modified syndromes t, pp in [2, P]: one call per
// value, so that each sees a compile-time syndrome count as the scrub's call
// does (its loops unroll and its matrix stays in registers on the device).
template <int PP>
HRS_HD inline bool locate_modified(const Field& f, int n, int pp, const uint8_t* t, int* nloc, uint8_t* loc,
                                   uint8_t* err) {
  if constexpr (PP < 2) {
    return false;
  } else {
    if (pp == PP) return locate(f, n, PP, t, nloc, loc, err);
    return locate_modified<PP - 1>(f, n, pp, t, nloc, loc, err);
  }
}

// What locate() is to an error-only column: fills the survivors blamed
// (loc[0..*nloc) ascending, their error values u[j], the byte at loc[j] is
// wrong by u[j]; kResolved only) and the e erased values v[m] at eloc[m]:
// the solution of sum_m v[m] alpha^(eloc[m] i) = s'_i, i < e, over the
// syndromes s' corrected by the blamed errors (kResolved) or s as it stands
// (kConsistent, kUnresolved). e <= p <= kMaxSyndromes; gamma from
// erasure_locator. e = 0 is locate() itself. P = p, the code's parity size.
template <int P>
HRS_HD inline int locate_errata(const Field& f, int n, const uint8_t* s, int e, const uint8_t* eloc,
                                const uint8_t* gamma, int* nloc, uint8_t* loc, uint8_t* u, uint8_t* v) {
  const int pp = P - e;
  uint8_t c[kMaxSyndromes];  // the syndromes the erased values are solved from
  for (int i = 0; i < P; ++i) c[i] = s[i];
  uint8_t t[kMaxSyndromes];
  uint32_t nz = 0;
  for (int i = 0; i < pp; ++i) {
    uint8_t x = 0;
    for (int j = 0; j <= e; ++j) x ^= fmul(f, gamma[j], s[i + e - j]);
    t[i] = x;
    nz |= x;
  }
  int state = kConsistent;
  *nloc = 0;
  if (nz != 0) {
    state = kUnresolved;
    if (pp >= 2) {
      int found = 0;
      bool ok = locate_modified<P>(f, n, pp, t, &found, loc, u);
      for (int j = 0; j < found; ++j)
        for (int m = 0; m < e; ++m) ok &= loc[j] != eloc[m];
      if (ok) {
        state = kResolved;
        *nloc = found;
        for (int j = 0; j < found; ++j) {
          const uint8_t y = f.exp[loc[j]];
          uint8_t scale = 1;
          for (int m = 0; m < e; ++m) scale = fmul(f, scale, static_cast<uint8_t>(y ^ f.exp[eloc[m]]));
          u[j] = fdiv(f, u[j], scale);
          for (int i = 0; i < e; ++i) c[i] ^= fmul(f, u[j], fpow(f, static_cast<int>(loc[j]) * i));
        }
      }
    }
  }
  // the Vandermonde solve of locate(), over the erased locations
  uint8_t x[kMaxErased];
  for (int m = 0; m < e; ++m) {
    x[m] = f.exp[eloc[m]];
    v[m] = c[m];
  }
  for (int i = 0; i < e - 1; ++i)
    for (int j = e - 1; j > i; --j) v[j] ^= fmul(f, x[i], v[j - 1]);
  for (int i = e - 1; i >= 0; --i) {
    for (int j = i + 1; j < e; ++j) v[j] = fdiv(f, v[j], static_cast<uint8_t>(x[j] ^ x[j - i - 1]));
    for (int j = i; j < e - 1; ++j) v[j] ^= v[j + 1];
  }
  return state;
}

}  // namespace locator
}  // namespace hrs
