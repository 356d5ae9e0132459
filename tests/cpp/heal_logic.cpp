// Stripe healing on the CPU (hrs_heal_host on host-only handles: the column
// loop over lambdafs_amd/csrc/hrs_locator.hpp that the heal kernels run)
// against the oracle's restatement of ReedSolomonCode.computeErrorLocations,
// over seeded words laid out as the byte columns of one stripe. The rule
// (include/hrs.h): a column the method resolves with a non-empty location set
// becomes the oracle's post-call data, any other column stays as it was, also
// where the oracle wrote into it before returning false. The report is
// rebuilt from the oracle's answers, word 3 as the bytes that changed.
// Exits 0 when every stripe and report agree.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "hrs.h"
#include "rs_oracle.h"

namespace {

int g_fail = 0;

struct Tally {
  long words = 0, clean = 0, restored = 0, spurious = 0, other_codeword = 0, unresolved = 0, unresolved_mutated = 0;
};

void run_shape(int k, int p, int ncols, unsigned seed, Tally& t) {
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
  std::vector<std::vector<uint8_t>> rows(n, std::vector<uint8_t>(ncols)), want(n, std::vector<uint8_t>(ncols));
  std::vector<uint32_t> rep(HRS_SCRUB_HEAD + n, 0), got(HRS_SCRUB_HEAD + n + 1, 0xA5A5A5A5u);
  rep[HRS_SCRUB_FIRST_BAD] = HRS_SCRUB_NONE;
  for (int col = 0; col < ncols; ++col) {
    std::vector<int> msg(k), par(p);
    for (int& v : msg) v = static_cast<int>(rng() & 0xFF);
    orc_rs_encode(k, p, msg.data(), par.data());
    std::vector<int> clean(par);
    clean.insert(clean.end(), msg.begin(), msg.end());
    std::vector<int> word(clean);
    const int errors = std::min(col % (p + 2), n);  // 0 .. p + 1 wrong symbols
    std::vector<int> locs;
    while (static_cast<int>(locs.size()) < errors) {
      const int l = static_cast<int>(rng() % n);
      if (std::find(locs.begin(), locs.end(), l) == locs.end()) locs.push_back(l);
    }
    for (int l : locs) word[l] ^= 1 + static_cast<int>(rng() % 255);
    std::vector<int> after(word), found(n, -1);
    int nfound = 0;
    const int ok = orc_rs_compute_error_locations(k, p, after.data(), found.data(), &nfound);
    const bool heal = ok && nfound > 0;
    const std::vector<int>& expect = heal ? after : word;
    for (int l = 0; l < n; ++l) {
      rows[l][col] = static_cast<uint8_t>(word[l]);
      want[l][col] = static_cast<uint8_t>(expect[l]);
    }
    ++t.words;
    if (ok && nfound == 0) {
      ++t.clean;
      continue;
    }
    ++rep[HRS_SCRUB_BAD];
    if (rep[HRS_SCRUB_FIRST_BAD] == HRS_SCRUB_NONE) rep[HRS_SCRUB_FIRST_BAD] = static_cast<uint32_t>(col);
    if (!ok) {
      ++rep[HRS_SCRUB_UNRESOLVED];
      ++t.unresolved;
      if (after != word) ++t.unresolved_mutated;
      continue;
    }
    int changed = 0;
    for (int l = 0; l < n; ++l) changed += after[l] != word[l];
    rep[HRS_SCRUB_PATCHED] += static_cast<uint32_t>(changed);
    for (int j = 0; j < nfound; ++j) ++rep[HRS_SCRUB_HEAD + found[j]];
    if (after == clean) ++t.restored;
    else ++t.other_codeword;
    if (nfound > changed) ++t.spurious;
    if (errors <= p / 2 && after != clean) {
      std::fprintf(stderr, "RS(%d,%d) column %d: %d errors resolved away from the codeword\n", k, p, col, errors);
      ++g_fail;
    }
  }
  std::vector<uint8_t*> ptrs(n);
  for (int l = 0; l < n; ++l) ptrs[l] = rows[l].data();
  const hrs_status st = hrs_heal_host(c, ptrs.data(), static_cast<size_t>(ncols), got.data());
  bool same = st == HRS_OK && got.back() == 0xA5A5A5A5u;
  for (int e = 0; same && e < HRS_SCRUB_HEAD + n; ++e) same = got[e] == rep[e];
  if (!same) {
    std::fprintf(stderr, "RS(%d,%d): status %d, report head %u %u %u %u, want %u %u %u %u\n", k, p, st, got[0], got[1],
                 got[2], got[3], rep[0], rep[1], rep[2], rep[3]);
    ++g_fail;
  }
  for (int l = 0; l < n; ++l)
    if (rows[l] != want[l]) {
      if (g_fail++ < 10) std::fprintf(stderr, "RS(%d,%d): row %d differs from the oracle's\n", k, p, l);
    }
  // a second pass stores nothing and finds only the unresolved columns
  std::vector<uint32_t> again(HRS_SCRUB_HEAD + n, 0);
  if (hrs_heal_host(c, ptrs.data(), static_cast<size_t>(ncols), again.data()) != HRS_OK ||
      again[HRS_SCRUB_PATCHED] != 0 || again[HRS_SCRUB_BAD] != rep[HRS_SCRUB_UNRESOLVED] ||
      again[HRS_SCRUB_UNRESOLVED] != rep[HRS_SCRUB_UNRESOLVED]) {
    std::fprintf(stderr, "RS(%d,%d): the second heal reports %u %u %u %u\n", k, p, again[0], again[1], again[2],
                 again[3]);
    ++g_fail;
  }
  for (int l = 0; l < n; ++l)
    if (rows[l] != want[l]) {
      if (g_fail++ < 10) std::fprintf(stderr, "RS(%d,%d): the second heal changed row %d\n", k, p, l);
    }
  hrs_destroy(c);
}

}  // namespace

int main() {
  const int shapes[][3] = {{10, 4, 3000}, {12, 4, 3000}, {6, 3, 3000}, {3, 2, 3000}, {4, 1, 600},  {20, 8, 3000},
                           {40, 7, 1000}, {5, 5, 1000},  {6, 6, 1000}, {245, 8, 300}, {247, 8, 300}};  // up to n = 255
  Tally t;
  unsigned seed = 101;
  for (const auto& s : shapes) run_shape(s[0], s[1], s[2], seed++, t);
  // argument errors on a host-only handle
  hrs_opts o{};
  o.device = HRS_DEVICE_NONE;
  hrs_codec* c = nullptr;
  uint8_t cell[12][4] = {};
  uint8_t* ptrs[12];
  for (int l = 0; l < 12; ++l) ptrs[l] = cell[l];
  uint32_t rep[16] = {};
  if (hrs_create(3, 9, &o, &c) != HRS_OK || hrs_heal_host(c, ptrs, 4, rep) != HRS_EINVAL) {
    std::fprintf(stderr, "parity_size 9 was not rejected\n");
    ++g_fail;
  }
  hrs_destroy(c);
  c = nullptr;
  if (hrs_create(3, 2, &o, &c) != HRS_OK) ++g_fail;
  ptrs[3] = ptrs[1];
  if (c && hrs_heal_host(c, ptrs, 4, rep) != HRS_EINVAL) {
    std::fprintf(stderr, "two equal row pointers were not rejected\n");
    ++g_fail;
  }
  ptrs[3] = nullptr;
  if (c && hrs_heal_host(c, ptrs, 4, rep) != HRS_EINVAL) {
    std::fprintf(stderr, "a NULL row was not rejected\n");
    ++g_fail;
  }
  hrs_destroy(c);
  std::printf(
      "heal_logic: %ld words (%ld clean, %ld restored, %ld with a spurious location, %ld resolved to another codeword, "
      "%ld unresolved of which %ld the oracle mutated), %d mismatches\n",
      t.words, t.clean, t.restored, t.spurious, t.other_codeword, t.unresolved, t.unresolved_mutated, g_fail);
  if (t.clean == 0 || t.restored == 0 || t.spurious == 0 || t.unresolved == 0 || t.unresolved_mutated == 0) {
    std::fprintf(stderr, "an outcome class never occurred: the comparison would be vacuous\n");
    return 1;
  }
  return g_fail ? 1 : 0;
}
