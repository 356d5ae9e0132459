// Checked repair on the CPU, two parts.
//
// 1. The erasure-pattern builder the plan kernel and make_pattern share
//    (repair::fill_pattern, hrs_repair_rule.hpp) against a construction of its
//    own written here from the definitions of hrs_heal_erased.hpp: Gamma as a
//    polynomial product, the Vandermonde inverse by the Lagrange basis (no
//    elimination), both over gf::mul / gf::div, not over the locator's log
//    tables. Over every erased set of RS(3,2) and RS(6,3) and 200 random sets
//    of RS(12,8) the 128-byte ErasePattern must be equal byte for byte. Each
//    set is also driven through hrs_heal_erased_host (whose make_pattern is
//    that builder): the erased cells of a codeword, filled with noise, come
//    back exactly.
// 2. hrs_repair_checked_host on a host-only handle: the verdicts CLEAN,
//    REPAIRED, TOOMANY and RESTAMP on few-column damage, with the bytes, the
//    erased_out row and the CRCs (zlib) each verdict promises, and the empty
//    call.
// Exits 0 when every assertion holds.
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../lambdafs_amd/csrc/hrs_repair_rule.hpp"
#include "hrs.h"

namespace {

namespace gf = hrs::gf;

int g_fail = 0;

void fail(const char* what, int k, int p, const std::vector<int>& set) {
  if (g_fail++ >= 20) return;
  std::fprintf(stderr, "RS(%d,%d) {", k, p);
  for (int l : set) std::fprintf(stderr, " %d", l);
  std::fprintf(stderr, " }: %s\n", what);
}

// The table entry of an erased set, from the definitions.
hrs::ErasePattern reference_pattern(int p, const std::vector<int>& key) {
  hrs::ErasePattern pt;
  std::memset(&pt, 0, sizeof pt);
  const int e = static_cast<int>(key.size()), pp = p - e;
  pt.e = e;
  for (int m = 0; m < e; ++m) {
    pt.loc[m] = static_cast<uint8_t>(key[m]);
    pt.mask[key[m] / 32] |= 1u << (key[m] % 32);
  }
  uint32_t spare = 0;
  while (std::find(key.begin(), key.end(), static_cast<int>(spare)) != key.end()) ++spare;
  pt.spare = spare;
  // Gamma(x) = prod_m (1 + X_m x)
  std::vector<uint8_t> gamma(e + 1, 0);
  gamma[0] = 1;
  for (int m = 0; m < e; ++m) {
    const uint8_t x = gf::alpha_pow(key[m]);
    for (int j = m + 1; j > 0; --j) gamma[j] = static_cast<uint8_t>(gamma[j] ^ gf::mul(gamma[j - 1], x));
  }
  for (int j = 0; j <= e; ++j) pt.gamma[j] = gamma[j];
  uint8_t mat[8][8] = {};
  for (int o = 0; o < pp; ++o)
    for (int j = 0; j <= e; ++j) mat[o][o + e - j] = gamma[j];
  // sum_m v_m X_m^i = S_i, i < e: v_m = sum_i c_{m,i} S_i with c_{m,.} the
  // coefficients of the Lagrange basis polynomial prod_{j != m} (x + X_j) / (X_m + X_j)
  for (int m = 0; m < e; ++m) {
    std::vector<uint8_t> poly(e, 0);
    poly[0] = 1;
    int deg = 0;
    uint8_t denom = 1;
    for (int j = 0; j < e; ++j) {
      if (j == m) continue;
      const uint8_t xj = gf::alpha_pow(key[j]);
      for (int d = deg + 1; d > 0; --d) poly[d] = static_cast<uint8_t>(poly[d - 1] ^ gf::mul(poly[d], xj));
      poly[0] = gf::mul(poly[0], xj);
      ++deg;
      denom = gf::mul(denom, static_cast<uint8_t>(gf::alpha_pow(key[m]) ^ xj));
    }
    for (int i = 0; i < e; ++i) mat[pp + m][i] = gf::div(poly[i], denom);
  }
  for (int i = 0; i < p; ++i)
    for (int o = 0; o < p; ++o) pt.cw[i] |= static_cast<uint64_t>(mat[o][i]) << (8 * o);
  return pt;
}

struct Stripe {
  int n;
  size_t len;
  std::vector<std::vector<uint8_t>> rows;
  std::vector<uint8_t*> ptrs() {
    std::vector<uint8_t*> p(n);
    for (int l = 0; l < n; ++l) p[l] = rows[l].data();
    return p;
  }
};

// A codeword stripe: random data cells, the p parity cells (locations 0..p-1)
// rebuilt as erasures.
Stripe codeword(hrs_codec* c, int k, int p, size_t len, std::mt19937& rng) {
  Stripe s{k + p, len, {}};
  s.rows.assign(k + p, std::vector<uint8_t>(len));
  for (auto& r : s.rows)
    for (auto& b : r) b = static_cast<uint8_t>(rng());
  std::vector<int> par(p);
  for (int l = 0; l < p; ++l) par[l] = l;
  std::vector<uint32_t> rep(HRS_SCRUB_HEAD + k + p);
  auto ptrs = s.ptrs();
  if (hrs_heal_erased_host(c, ptrs.data(), len, par.data(), p, rep.data()) != HRS_OK || rep[HRS_SCRUB_BAD] != 0) {
    std::fprintf(stderr, "codeword: %s\n", hrs_last_error(c));
    ++g_fail;
  }
  return s;
}

void check_set(hrs_codec* c, int k, int p, const std::vector<int>& key, std::mt19937& rng) {
  static constexpr gf::Tables kT = gf::make_tables();
  const hrs::locator::Field f{kT.exp, kT.log};
  hrs::ErasePattern pt;
  std::memset(&pt, 0, sizeof pt);
  pt.e = static_cast<int>(key.size());
  for (size_t m = 0; m < key.size(); ++m) pt.loc[m] = static_cast<uint8_t>(key[m]);
  hrs::repair::PatternWork work;
  std::memset(&work, 0xA5, sizeof work);  // the builder relies on nothing in it
  hrs::repair::fill_pattern(f, p, pt, work);
  const hrs::ErasePattern want = reference_pattern(p, key);
  if (std::memcmp(&pt, &want, sizeof pt) != 0) fail("fill_pattern differs from the definitions", k, p, key);
  Stripe s = codeword(c, k, p, 64, rng);
  const auto good = s.rows;
  for (int l : key)
    for (auto& b : s.rows[l]) b = static_cast<uint8_t>(rng());
  std::vector<uint32_t> rep(HRS_SCRUB_HEAD + k + p);
  auto ptrs = s.ptrs();
  if (hrs_heal_erased_host(c, ptrs.data(), s.len, key.data(), static_cast<int>(key.size()), rep.data()) != HRS_OK)
    fail(hrs_last_error(c), k, p, key);
  if (s.rows != good || rep[HRS_SCRUB_BAD] != 0) fail("erased cells not rebuilt", k, p, key);
}

hrs_codec* host_codec(int k, int p) {
  hrs_opts o{};
  o.device = HRS_DEVICE_NONE;
  hrs_codec* c = nullptr;
  if (hrs_create(k, p, &o, &c) != HRS_OK) {
    std::fprintf(stderr, "hrs_create(%d,%d): %s\n", k, p, hrs_last_error(nullptr));
    ++g_fail;
    return nullptr;
  }
  return c;
}

void patterns(int k, int p, int random_sets, unsigned seed) {
  hrs_codec* c = host_codec(k, p);
  if (!c) return;
  const int n = k + p;
  std::mt19937 rng(seed);
  long sets = 0;
  if (random_sets == 0) {
    for (uint32_t bits = 0; bits < (1u << n); ++bits) {
      if (__builtin_popcount(bits) > p) continue;
      std::vector<int> key;
      for (int l = 0; l < n; ++l)
        if ((bits >> l) & 1u) key.push_back(l);
      check_set(c, k, p, key, rng);
      ++sets;
    }
  } else {
    for (int i = 0; i < random_sets; ++i) {
      std::vector<int> all(n);
      for (int l = 0; l < n; ++l) all[l] = l;
      std::shuffle(all.begin(), all.end(), rng);
      std::vector<int> key(all.begin(), all.begin() + 1 + static_cast<int>(rng() % p));
      std::sort(key.begin(), key.end());
      check_set(c, k, p, key, rng);
      ++sets;
    }
  }
  std::printf("RS(%d,%d): %ld erased sets, patterns equal\n", k, p, sets);
  hrs_destroy(c);
}

uint32_t zcrc(const std::vector<uint8_t>& r) { return static_cast<uint32_t>(crc32(0L, r.data(), static_cast<uInt>(r.size()))); }

struct Outcome {
  uint32_t verdict = 99;
  std::vector<int32_t> erased;
  std::vector<uint32_t> report, crcs;
};

Outcome run(hrs_codec* c, Stripe& s, int p, const std::vector<uint32_t>& stored, int flags) {
  Outcome o;
  o.erased.assign(p, 77);
  o.report.assign(HRS_SCRUB_HEAD + s.n, 0xA5A5A5A5u);
  o.crcs.assign(s.n, 0xA5A5A5A5u);
  auto ptrs = s.ptrs();
  const hrs_status st = hrs_repair_checked_host(c, ptrs.data(), s.len, stored.data(), flags, &o.verdict, o.erased.data(),
                                                o.report.data(), o.crcs.data());
  if (st != HRS_OK) {
    std::fprintf(stderr, "hrs_repair_checked_host: %d %s\n", st, hrs_last_error(c));
    ++g_fail;
  }
  return o;
}

void expect(bool ok, const char* what) {
  if (!ok && g_fail++ < 20) std::fprintf(stderr, "repair_checked_host: %s\n", what);
}

void verdicts(int k, int p, size_t len, unsigned seed) {
  hrs_codec* c = host_codec(k, p);
  if (!c) return;
  const int n = k + p;
  std::mt19937 rng(seed);
  const Stripe good = codeword(c, k, p, len, rng);
  std::vector<uint32_t> stored(n);
  for (int l = 0; l < n; ++l) stored[l] = zcrc(good.rows[l]);
  const size_t cols[] = {0, 15, len / 2, len - 1};
  // every cell in columns of its own: one error per column, which the locator
  // resolves at p >= 2, so the join flag blames exactly the damaged cells
  auto damage = [&](Stripe& s, int l) {
    for (size_t col : cols) s.rows[l][(col + 3 * l + 1) % len] ^= static_cast<uint8_t>(1 + rng() % 255);
  };
  for (int flags = 0; flags <= 1; ++flags) {
    {  // untouched
      Stripe s = good;
      const Outcome o = run(c, s, p, stored, flags);
      expect(o.verdict == HRS_REPAIR_CLEAN && s.rows == good.rows && o.crcs == stored, "clean stripe");
      expect(std::all_of(o.erased.begin(), o.erased.end(), [](int32_t v) { return v == -1; }), "clean erased_out");
      expect(o.report[HRS_SCRUB_BAD] == 0 && o.report[HRS_SCRUB_FIRST_BAD] == HRS_SCRUB_NONE, "clean report");
    }
    {  // p damaged cells, true checksums
      Stripe s = good;
      for (int l = 0; l < p; ++l) damage(s, l + 1);
      const Outcome o = run(c, s, p, stored, flags);
      expect(o.verdict == HRS_REPAIR_REPAIRED, "p damaged cells: verdict");
      expect(s.rows == good.rows && o.crcs == stored, "p damaged cells: bytes and CRCs");
      expect(std::is_sorted(o.erased.begin(), o.erased.end()) && o.erased[0] >= 0, "p damaged cells: erased_out");
    }
    {  // p + 1 damaged cells: never written
      Stripe s = good;
      for (int l = 0; l <= p; ++l) damage(s, l);
      const Stripe before = s;
      const Outcome o = run(c, s, p, stored, flags);
      expect(o.verdict == HRS_REPAIR_TOOMANY && s.rows == before.rows, "p + 1 damaged cells");
      for (int l = 0; l < n; ++l) expect(o.crcs[l] == zcrc(before.rows[l]), "too many: CRCs as read");
      expect(std::all_of(o.erased.begin(), o.erased.end(), [](int32_t v) { return v == -1; }), "too many erased_out");
    }
    if (p >= 2) {  // a stale parity cell whose checksum was rewritten with it
      Stripe s = good;
      damage(s, 0);
      std::vector<uint32_t> st2 = stored;
      st2[0] = zcrc(s.rows[0]);
      const Outcome o = run(c, s, p, st2, flags);
      expect(o.verdict == HRS_REPAIR_RESTAMP && s.rows == good.rows, "restamped parity cell");
      expect(o.crcs == stored, "restamp: crc_out holds the new values");
    }
  }
  {  // the empty call touches nothing
    Stripe s = good;
    Outcome o;
    o.report.assign(HRS_SCRUB_HEAD + n, 0xA5A5A5A5u);
    auto ptrs = s.ptrs();
    expect(hrs_repair_checked_host(c, ptrs.data(), 0, nullptr, 0, nullptr, nullptr, o.report.data(), nullptr) == HRS_OK &&
               o.report[0] == 0xA5A5A5A5u,
           "empty call");
    expect(hrs_repair_checked_host(c, ptrs.data(), 0, nullptr, 2, nullptr, nullptr, o.report.data(), nullptr) == HRS_EINVAL,
           "bad flag bit on an empty call");
  }
  std::printf("RS(%d,%d) len %zu: verdicts as promised\n", k, p, len);
  hrs_destroy(c);
}

}  // namespace

int main() {
  patterns(3, 2, 0, 1);
  patterns(6, 3, 0, 2);
  patterns(12, 8, 200, 3);
  verdicts(6, 3, 300, 4);
  verdicts(10, 4, 2048 + 80, 5);
  verdicts(3, 2, 100, 6);
  if (g_fail) {
    std::fprintf(stderr, "%d failures\n", g_fail);
    return 1;
  }
  std::printf("repair_checked_logic ok\n");
  return 0;
}
