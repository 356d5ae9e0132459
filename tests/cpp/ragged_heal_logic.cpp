// hrs_heal_ragged_host (one stripe on the CPU, host-only handle) against a model
// built from the scalar hrs_compute_error_locations alone: every column
// zero-filled beyond its cells' lengths, the method's post-call data, then the
// demotion rule of include/hrs.h ("ragged scrub and heal"). Every cell is
// allocated with exactly its valid bytes, so under `make asan` a read or a
// write at or beyond a cell's length is a heap overflow.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "hrs.h"

namespace {

int fails = 0;

void check(bool ok, const char* what, int k, int p, int trial) {
  if (ok) return;
  std::printf("FAIL RS(%d,%d) trial %d: %s\n", k, p, trial, what);
  ++fails;
}

void run(int k, int p, size_t len, int trials, uint32_t seed) {
  const int n = k + p;
  hrs_codec* c = nullptr;
  hrs_opts o{};
  o.device = HRS_DEVICE_NONE;
  if (hrs_create(k, p, &o, &c) != HRS_OK) {
    std::printf("FAIL hrs_create(%d,%d)\n", k, p);
    ++fails;
    return;
  }
  std::mt19937 rng(seed);
  long demoted = 0, patched = 0, unresolved = 0;
  for (int trial = 0; trial < trials; ++trial) {
    // a codeword of full cells, made column by column with the heal itself: the
    // parity cells are "erased" by solving through hrs_encode_matrix
    std::vector<uint8_t> g(static_cast<size_t>(p) * k);
    hrs_encode_matrix(c, g.data());
    std::vector<std::vector<uint8_t>> full(n, std::vector<uint8_t>(len));
    for (int j = 0; j < k; ++j)
      for (size_t col = 0; col < len; ++col) full[p + j][col] = static_cast<uint8_t>(rng());
    // GF(2^8) multiply, polynomial 0x11D
    auto mul = [](uint8_t a, uint8_t b) {
      uint8_t r = 0;
      for (int i = 0; i < 8; ++i) {
        if (b & 1) r ^= a;
        const bool hi = a & 0x80;
        a = static_cast<uint8_t>(a << 1);
        if (hi) a ^= 0x1D;
        b >>= 1;
      }
      return r;
    };
    // lengths: data cells of every kind, parity cells full or (one trial in three) one of them short
    std::vector<uint32_t> valid(n, static_cast<uint32_t>(len));
    for (int j = 0; j < k; ++j) {
      const uint32_t pick = rng() % 4;
      valid[p + j] = pick == 0 ? 0u : pick == 1 ? static_cast<uint32_t>(len) : static_cast<uint32_t>(rng() % (len + 1));
    }
    const bool consistent = trial % 3 != 0;  // else: parity made from data longer than the lengths say
    for (int r = 0; r < p; ++r)
      for (size_t col = 0; col < len; ++col) {
        uint8_t x = 0;
        for (int j = 0; j < k; ++j)
          if (!consistent || col < valid[p + j]) x ^= mul(g[static_cast<size_t>(r) * k + j], full[p + j][col]);
        full[r][col] = x;
      }
    if (trial % 3 == 2) valid[rng() % p] = static_cast<uint32_t>(rng() % (len + 1));
    // the cells as stored: exactly valid bytes each, with a few wrong bytes
    std::vector<uint8_t*> rows(n);
    for (int l = 0; l < n; ++l) {
      rows[l] = static_cast<uint8_t*>(std::malloc(valid[l] ? valid[l] : 1));
      std::memcpy(rows[l], full[l].data(), valid[l]);
    }
    for (int e = 0; e < 6; ++e) {
      const int l = static_cast<int>(rng() % n);
      if (valid[l]) rows[l][rng() % valid[l]] ^= static_cast<uint8_t>(1 + rng() % 255);
    }
    // the model
    std::vector<std::vector<uint8_t>> want(n);
    for (int l = 0; l < n; ++l) want[l].assign(rows[l], rows[l] + valid[l]);
    std::vector<uint32_t> rep(HRS_SCRUB_HEAD + n, 0u);
    rep[HRS_SCRUB_FIRST_BAD] = HRS_SCRUB_NONE;
    std::vector<int> data(n), before(n), locs(n);
    for (size_t col = 0; col < len; ++col) {
      for (int l = 0; l < n; ++l) before[l] = data[l] = col < valid[l] ? rows[l][col] : 0;
      int nloc = 0, resolved = 0;
      if (hrs_compute_error_locations(c, data.data(), locs.data(), &nloc, &resolved) != HRS_OK) {
        check(false, "hrs_compute_error_locations", k, p, trial);
        break;
      }
      if (resolved && nloc == 0) continue;  // a codeword
      ++rep[HRS_SCRUB_BAD];
      if (rep[HRS_SCRUB_FIRST_BAD] == HRS_SCRUB_NONE) rep[HRS_SCRUB_FIRST_BAD] = static_cast<uint32_t>(col);
      bool virt = false;
      for (int j = 0; j < nloc; ++j) virt |= data[locs[j]] != before[locs[j]] && col >= valid[locs[j]];
      if (!resolved || virt) {
        ++rep[HRS_SCRUB_UNRESOLVED];
        demoted += resolved && virt;
        unresolved += !resolved;
        continue;
      }
      for (int j = 0; j < nloc; ++j) {
        ++rep[HRS_SCRUB_HEAD + locs[j]];
        if (data[locs[j]] == before[locs[j]]) continue;
        want[locs[j]][col] = static_cast<uint8_t>(data[locs[j]]);
        ++rep[HRS_SCRUB_PATCHED];
        ++patched;
      }
    }
    std::vector<uint32_t> got(HRS_SCRUB_HEAD + n, 0xA5A5A5A5u);
    check(hrs_heal_ragged_host(c, rows.data(), len, valid.data(), got.data()) == HRS_OK, "status", k, p, trial);
    check(got == rep, "report", k, p, trial);
    for (int l = 0; l < n; ++l)
      check(valid[l] == 0 || std::memcmp(rows[l], want[l].data(), valid[l]) == 0, "bytes", k, p, trial);
    for (int l = 0; l < n; ++l) std::free(rows[l]);
  }
  std::printf("RS(%d,%d) len %zu: %d stripes, %ld patched bytes, %ld unresolved and %ld demoted columns\n", k, p, len,
              trials, patched, unresolved, demoted);
  check(p < 2 || (patched > 0 && demoted > 0), "no patched or no demoted column in any trial", k, p, -1);
  hrs_destroy(c);
}

}  // namespace

int main() {
  const int shapes[][2] = {{10, 4}, {6, 3}, {3, 2}, {12, 4}, {4, 1}, {9, 5}, {8, 6}, {7, 7}, {20, 8}, {247, 8}};
  uint32_t seed = 1;
  for (const auto& s : shapes) run(s[0], s[1], s[0] > 100 ? 40 : 150, s[0] > 100 ? 3 : 12, seed++);
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("ragged_heal_logic: ok\n");
  return 0;
}
