// The error locator (lambdafs_amd/csrc/hrs_locator.hpp, reached through
// hrs_compute_error_locations on host-only handles) against the oracle's
// restatement of ReedSolomonCode.computeErrorLocations, over seeded words:
// the boolean, the location list and the mutated data must all agree. This
// also checks the locator's shortcut (error values and the second syndrome
// from the first syndromes alone) on every word. Exits 0 when all agree.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "hrs.h"
#include "rs_oracle.h"

namespace {

int g_fail = 0;

struct Tally {
  long words = 0, clean = 0, exact = 0, wrong_set = 0, unresolved = 0;
};

void compare(hrs_codec* c, int k, int p, const std::vector<int>& word, const std::vector<int>& truth, Tally& t) {
  const int n = k + p;
  std::vector<int> a(word), b(word), la(n, -1), lb(n, -1);
  int na = 0, nb = 0, ra = -1;
  const int rb = orc_rs_compute_error_locations(k, p, b.data(), lb.data(), &nb);
  const hrs_status st = hrs_compute_error_locations(c, a.data(), la.data(), &na, &ra);
  bool ok = st == HRS_OK && ra == rb && na == nb && a == b;
  for (int i = 0; ok && i < nb; ++i) ok = la[i] == lb[i];
  if (!ok && g_fail++ < 10) {
    std::fprintf(stderr, "RS(%d,%d) mismatch: status %d resolved %d/%d nloc %d/%d, word:", k, p, st, ra, rb, na, nb);
    for (int v : word) std::fprintf(stderr, " %d", v);
    std::fprintf(stderr, "\n");
  }
  ++t.words;
  if (rb && nb == 0) ++t.clean;
  else if (!rb) ++t.unresolved;
  else if (std::vector<int>(lb.begin(), lb.begin() + nb) == truth) ++t.exact;
  else ++t.wrong_set;
}

void run_shape(int k, int p, unsigned seed, Tally& t) {
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
  for (int rep = 0; rep < 400; ++rep) {
    std::vector<int> msg(k), par(p);
    for (int& v : msg) v = static_cast<int>(rng() & 0xFF);
    orc_rs_encode(k, p, msg.data(), par.data());
    std::vector<int> clean(par);
    clean.insert(clean.end(), msg.begin(), msg.end());
    for (int errors = 0; errors <= 3 && errors <= n; ++errors) {
      std::vector<int> word(clean), locs;
      while (static_cast<int>(locs.size()) < errors) {
        const int l = static_cast<int>(rng() % n);
        bool dup = false;
        for (int x : locs) dup |= x == l;
        if (!dup) locs.push_back(l);
      }
      const int same = 1 + static_cast<int>(rng() % 255);
      const bool equal_values = errors == 2 && (rep & 1);  // S_0 = 0
      for (int l : locs) word[l] ^= equal_values ? same : 1 + static_cast<int>(rng() % 255);
      std::vector<int> truth(locs);
      for (size_t i = 0; i < truth.size(); ++i)
        for (size_t j = i + 1; j < truth.size(); ++j)
          if (truth[j] < truth[i]) std::swap(truth[i], truth[j]);
      compare(c, k, p, word, truth, t);
    }
    std::vector<int> noise(n);  // a word far from every codeword
    for (int& v : noise) v = static_cast<int>(rng() & 0xFF);
    compare(c, k, p, noise, {}, t);
  }
  hrs_destroy(c);
}

}  // namespace

int main() {
  const int shapes[][2] = {{10, 4}, {12, 4}, {6, 3}, {3, 2}, {4, 1}, {20, 8}, {40, 7}, {5, 5}, {6, 6}, {245, 8},
                           {247, 8}};  // n = 255, the most hrs_create admits
  Tally t;
  unsigned seed = 1;
  for (const auto& kp : shapes) run_shape(kp[0], kp[1], seed++, t);
  // argument errors on a host-only handle
  hrs_opts o{};
  o.device = HRS_DEVICE_NONE;
  hrs_codec* c = nullptr;
  int data[16] = {}, locs[16], nloc = 0, res = 0;
  if (hrs_create(3, 9, &o, &c) != HRS_OK || hrs_compute_error_locations(c, data, locs, &nloc, &res) != HRS_EINVAL) {
    std::fprintf(stderr, "parity_size 9 was not rejected\n");
    ++g_fail;
  }
  hrs_destroy(c);
  c = nullptr;
  data[2] = 256;
  if (hrs_create(3, 2, &o, &c) != HRS_OK || hrs_compute_error_locations(c, data, locs, &nloc, &res) != HRS_EINVAL) {
    std::fprintf(stderr, "a symbol of 256 was not rejected\n");
    ++g_fail;
  }
  hrs_destroy(c);
  std::printf("scrub_logic: %ld words (%ld clean, %ld exact, %ld resolved with another set, %ld unresolved), %d mismatches\n",
              t.words, t.clean, t.exact, t.wrong_set, t.unresolved, g_fail);
  if (t.clean == 0 || t.exact == 0 || t.wrong_set == 0 || t.unresolved == 0) {
    std::fprintf(stderr, "an outcome class never occurred: the comparison would be vacuous\n");
    return 1;
  }
  return g_fail ? 1 : 0;
}
