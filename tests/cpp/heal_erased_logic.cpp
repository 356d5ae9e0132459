// Heal with known erasures on the CPU (hrs_heal_erased_host on host-only
// handles: the column loop over locator::locate_errata that the kernels run)
// over seeded columns: codewords from the oracle's encoder, e cells erased
// (their stored bytes replaced by noise) and t survivors damaged, for every
// e <= p and t = 0 .. (p - e) / 2 + 1. Asserts (include/hrs.h):
//   - uniqueness: within capacity (t <= (p - e) / 2) every column that is not
//     counted unresolved equals the codeword in all n bytes;
//   - at parity_size <= 4 every column within capacity resolves;
//   - with nothing erased the call equals hrs_heal_host, bytes and report.
// Prints, per shape and (e, t), the columns restored, unresolved and wrong
// without being counted unresolved (miscorrected or undetected): the counts
// DESIGN.md section 10.3 quotes. Exits 0 when every assertion holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "hrs.h"
#include "rs_oracle.h"

namespace {

int g_fail = 0;

void fail(const char* what, int k, int p, int e, int t) {
  if (g_fail++ < 20) std::fprintf(stderr, "RS(%d,%d) e=%d t=%d: %s\n", k, p, e, t, what);
}

std::vector<int> sample(std::mt19937& rng, int n, int count, const std::vector<int>& avoid) {
  std::vector<int> out;
  while (static_cast<int>(out.size()) < count) {
    const int l = static_cast<int>(rng() % n);
    if (std::find(out.begin(), out.end(), l) == out.end() && std::find(avoid.begin(), avoid.end(), l) == avoid.end())
      out.push_back(l);
  }
  return out;
}

// ncols columns in stripes of `per` columns, each stripe with its own erased set.
void run_shape(int k, int p, int ncols, int per, unsigned seed) {
  const int n = k + p;
  hrs_opts o{};
  o.device = HRS_DEVICE_NONE;
  hrs_codec* c = nullptr;
  if (hrs_create(k, p, &o, &c) != HRS_OK) {
    std::fprintf(stderr, "hrs_create(%d,%d): %s\n", k, p, hrs_last_error(nullptr));
    ++g_fail;
    return;
  }
  std::mt19937 rng(seed);
  for (int e = 0; e <= p; ++e) {
    const int cap = (p - e) / 2;
    for (int t = 0; t <= cap + 1 && e + t <= n; ++t) {
      long restored = 0, unresolved = 0, other = 0;
      for (int c0 = 0; c0 < ncols; c0 += per) {
        std::vector<int> erased = sample(rng, n, e, {});
        std::vector<std::vector<uint8_t>> rows(n, std::vector<uint8_t>(per)), want(n, std::vector<uint8_t>(per));
        for (int col = 0; col < per; ++col) {
          std::vector<int> msg(k), par(p);
          for (int& v : msg) v = static_cast<int>(rng() & 0xFF);
          orc_rs_encode(k, p, msg.data(), par.data());
          for (int l = 0; l < n; ++l) want[l][col] = rows[l][col] = static_cast<uint8_t>(l < p ? par[l] : msg[l - p]);
          for (int l : erased) rows[l][col] = static_cast<uint8_t>(rng());  // never read
          for (int l : sample(rng, n, t, erased)) rows[l][col] ^= static_cast<uint8_t>(1 + rng() % 255);
        }
        std::vector<std::vector<uint8_t>> before(rows);
        std::vector<uint8_t*> ptrs(n);
        for (int l = 0; l < n; ++l) ptrs[l] = rows[l].data();
        std::vector<uint32_t> rep(HRS_SCRUB_HEAD + n + 1, 0xA5A5A5A5u);
        std::shuffle(erased.begin(), erased.end(), rng);  // any order is accepted
        erased.push_back(-1);
        const hrs_status st = hrs_heal_erased_host(c, ptrs.data(), static_cast<size_t>(per), erased.data(),
                                                   static_cast<int>(erased.size()), rep.data());
        if (st != HRS_OK || rep.back() != 0xA5A5A5A5u) {
          fail("bad status or a report word past 4 + n written", k, p, e, t);
          continue;
        }
        long wrong = 0;
        for (int col = 0; col < per; ++col) {
          bool same = true;
          for (int l = 0; l < n; ++l) same &= rows[l][col] == want[l][col];
          wrong += !same;
        }
        restored += per - wrong;
        unresolved += rep[HRS_SCRUB_UNRESOLVED];
        other += wrong - static_cast<long>(rep[HRS_SCRUB_UNRESOLVED]);
        for (int l : erased)
          if (l >= 0 && rep[HRS_SCRUB_HEAD + l] != 0) fail("an erased location was blamed", k, p, e, t);
        if (t <= cap && wrong != static_cast<long>(rep[HRS_SCRUB_UNRESOLVED]))
          fail("a column within capacity came back resolved and wrong (uniqueness)", k, p, e, t);
        if (t == 0 && (rep[HRS_SCRUB_BAD] != 0 || rep[HRS_SCRUB_FIRST_BAD] != HRS_SCRUB_NONE || rep[HRS_SCRUB_PATCHED] != 0))
          fail("clean survivors were reported bad", k, p, e, t);
        if (e == 0) {  // nothing erased: hrs_heal_host
          std::vector<uint8_t*> hp(n);
          for (int l = 0; l < n; ++l) hp[l] = before[l].data();
          std::vector<uint32_t> hrep(HRS_SCRUB_HEAD + n, 0);
          if (hrs_heal_host(c, hp.data(), static_cast<size_t>(per), hrep.data()) != HRS_OK || before != rows ||
              !std::equal(hrep.begin(), hrep.end(), rep.begin()))
            fail("differs from hrs_heal_host", k, p, e, t);
        }
      }
      if (t <= cap && p <= 4 && unresolved != 0) fail("a column within capacity did not resolve", k, p, e, t);
      std::printf("RS(%d,%d) e=%d t=%d%s: %ld restored, %ld unresolved, %ld wrong and not unresolved, of %d\n", k, p, e, t,
                  t > cap ? " (past capacity)" : "", restored, unresolved, other, ncols);
    }
  }
  hrs_destroy(c);
}

}  // namespace

int main() {
  const int shapes[][4] = {{10, 4, 600, 60}, {12, 4, 600, 60}, {6, 3, 600, 60}, {3, 2, 600, 60},
                           {4, 1, 600, 60},  {20, 8, 600, 60}, {247, 8, 60, 10}, {6, 5, 600, 60},
                           {7, 6, 600, 60},  {10, 7, 600, 60}};
  unsigned seed = 211;
  for (const auto& s : shapes) run_shape(s[0], s[1], s[2], s[3], seed++);
  // argument errors on a host-only handle
  hrs_opts o{};
  o.device = HRS_DEVICE_NONE;
  hrs_codec* c = nullptr;
  uint8_t cell[5][4] = {};
  uint8_t* ptrs[5];
  for (int l = 0; l < 5; ++l) ptrs[l] = cell[l];
  uint32_t rep[9] = {};
  if (hrs_create(3, 2, &o, &c) != HRS_OK) return 1;
  const int three[] = {0, 1, 2}, twice[] = {1, 1}, outside[] = {5}, one[] = {4};
  if (hrs_heal_erased_host(c, ptrs, 4, three, 3, rep) != HRS_ETOOMANY) fail("three erasures accepted", 3, 2, 3, 0);
  if (hrs_heal_erased_host(c, ptrs, 4, twice, 2, rep) != HRS_EINVAL) fail("a repeated location accepted", 3, 2, 2, 0);
  if (hrs_heal_erased_host(c, ptrs, 4, outside, 1, rep) != HRS_EINVAL) fail("location n accepted", 3, 2, 1, 0);
  if (hrs_heal_erased_host(c, ptrs, 4, one, -1, rep) != HRS_EINVAL) fail("num_erased -1 accepted", 3, 2, 1, 0);
  if (hrs_heal_erased_host(c, ptrs, 4, one, 1, rep) != HRS_OK || rep[0] != 0) fail("a zero stripe is not clean", 3, 2, 1, 0);
  hrs_destroy(c);
  std::printf("heal_erased_logic: %d mismatches\n", g_fail);
  return g_fail ? 1 : 0;
}
