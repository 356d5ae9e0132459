// Stripe scrubbing and healing behind the C ABI: the scalar
// computeErrorLocations on the host (hrs_compute_error_locations, host-only
// handles included), the device-resident batches (hrs_scrub_dev, hrs_heal_dev,
// hrs_scrub_crc_dev, hrs_heal_crc_dev with the cells' CRC-32s from the same
// pass, hrs_scrub_ragged_dev, hrs_heal_ragged_dev over cells with per-cell
// lengths (their gate scrub_ragged_args_ok, hrs_heal_ragged_host on the CPU), and hrs_heal_erased_dev / hrs_heal_erased_crc_dev with their erasure
// patterns: validated, de-duplicated, with the constants the kernels of
// hrs_heal_erased.hip and hrs_heal_erased_crc.hip multiply by) and one stripe
// healed on the CPU (hrs_heal_host, hrs_heal_erased_host), the kernels'
// byte-exact reference; also hrs_repair_checked_host, checked repair of one
// stripe over those same CPU pieces (its device call is hrs_repair_api.cpp).
// The host-memory batches are in hrs_hostbatch_api.cpp beside the pipeline they
// share. The per-column algorithm is hrs_locator.hpp, the same code the
// kernels run.
//
// The entry points share one argument gate (scrub_args_ok), the device calls
// one window / tail launcher (run_windows_tail), the one-pass CRC calls one
// body (scrub_crc_pass) and the CPU calls one column loop (heal_stripe).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/hrs.h"
#include "gf256.hpp"
#include "hrs_codec.hpp"
#include "hrs_crc.hpp"
#include "hrs_heal_erased.hpp"
#include "hrs_internal.hpp"
#include "hrs_launch.hpp"
#include "hrs_locator.hpp"
#include "hrs_repair_rule.hpp"
#include "hrs_scrub_ragged.hpp"

namespace hrs::api {

namespace {

constexpr hrs::gf::Tables kHostTables = hrs::gf::make_tables();
constexpr hrs::locator::Field kHostField{kHostTables.exp, kHostTables.log};

template <int P>
void column_syndromes(int n, const int* data, uint8_t* out) {
  uint8_t s[P] = {};
  for (int l = n - 1; l >= 0; --l) hrs::locator::horner_step<P>(kHostField, s, static_cast<uint8_t>(data[l]));
  for (int i = 0; i < P; ++i) out[i] = s[i];
}

}  // namespace

hrs_status scrub_code_ok(hrs_codec* c, size_t report_stride, bool with_reports) {
  if (c->kind != HRS_CODE_RS) return fail(c, HRS_EINVAL, "error location is defined for the rs code only");
  if (c->p > hrs::locator::kMaxSyndromes)
    return fail(c, HRS_EINVAL, "error location supports parity_size <= %d, this codec has %d",
                hrs::locator::kMaxSyndromes, c->p);
  if (c->n > hrs::kScrubMaxRows)  // hrs_create admits no such handle; ScrubArgs and the LDS histogram hold this many
    return fail(c, HRS_EINVAL, "scrubbing supports at most %d locations, this codec has %d", hrs::kScrubMaxRows, c->n);
  if (with_reports && report_stride < static_cast<size_t>(hrs::kScrubHead + c->n))
    return fail(c, HRS_EINVAL, "report_stride %zu is below 4 + n = %d words", report_stride, hrs::kScrubHead + c->n);
  return HRS_OK;
}

// A patch through one of two equal row pointers would change the other's column.
hrs_status heal_rows_ok(hrs_codec* c, const uint8_t* const* rows) {
  for (int l = 0; l < c->n; ++l)
    if (!rows[l]) return fail(c, HRS_EINVAL, "row %d is NULL", l);
  for (int l = 1; l < c->n; ++l)
    for (int m = 0; m < l; ++m)
      if (rows[l] == rows[m]) return fail(c, HRS_EINVAL, "rows %d and %d are one pointer: healing writes the rows", m, l);
  return HRS_OK;
}

hrs_status scrub_args_ok(hrs_codec* c, const void* cells, const uint32_t* reports, size_t report_stride, size_t len,
                         size_t nstripes, unsigned flags, const char* erased_what, int erased_count,
                         const int* erased) {
  if (!c) return HRS_EINVAL;
  const bool with_reports = flags & kScrubWithReports, image = flags & kScrubImage;
  hrs_status st = scrub_code_ok(c, report_stride, with_reports);
  if (st != HRS_OK) return st;
  if (!cells || !reports)
    return fail(c, HRS_EINVAL, "%s or %s is NULL", image ? "stripes" : "rows", with_reports ? "reports" : "report");
  if (!image) {
    const uint8_t* const* rows = static_cast<const uint8_t* const*>(cells);
    if (flags & kScrubRowsWritten) {
      st = heal_rows_ok(c, rows);
      if (st != HRS_OK) return st;
    } else {
      for (int l = 0; l < c->n; ++l)
        if (!rows[l]) return fail(c, HRS_EINVAL, "row %d is NULL", l);
    }
  }
  if (erased_what && (erased_count < 0 || (erased_count > 0 && !erased)))
    return fail(c, HRS_EINVAL, "%s %d with %s erased list", erased_what, erased_count, erased ? "an" : "no");
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  if (len > 0xffffffffu) return fail(c, HRS_EINVAL, "rows of %zu bytes: column indices are 32-bit", len);
  return HRS_OK;
}

namespace {

// Empty reports, then `windows` over the whole 2 KiB windows (rows and stride
// 16-byte aligned, not kernel mode 2) and `tail` over the columns from col0
// on, both reading the ScrubArgs `a` this fills. `what` names the call in
// launch errors. The handle's last kernel is the window kernel when one ran.
template <class Windows, class Tail>
hrs_status run_windows_tail(hrs_codec* c, hrs::ScrubArgs& a, const uint8_t* const* rows, size_t stride, size_t len,
                            size_t nstripes, uint32_t* reports, size_t report_stride, hipStream_t s,
                            const std::string& what, Windows windows, Tail tail) {
  hipError_t e = hrs::launch_scrub_init(reports, report_stride, c->n, nstripes, s);
  if (e != hipSuccess) return hip_fail(c, e, "scrub init launch");
  bool vec_ok = stride % 16 == 0 && c->kernel_mode != 2;
  for (int l = 0; l < c->n; ++l) {
    a.rows[l] = rows[l];
    vec_ok &= aligned16(rows[l]);
  }
  a.stride = stride;
  a.len = len;
  a.reports = reports;
  a.report_stride = report_stride;
  a.n = c->n;
  a.p = c->p;
  a.nwin = vec_ok ? len / hrs::kWindowBytes : 0;
  if (a.nwin > 0) {
    a.ntasks = a.nwin * nstripes;
    if ((e = windows()) != hipSuccess) return hip_fail(c, e, (what + " launch").c_str());
    c->last_kernel = hrs::last_kernel();
  }
  a.col0 = a.nwin * hrs::kWindowBytes;
  if (a.col0 < len) {
    a.ntasks = (len - a.col0) * nstripes;
    if ((e = tail()) != hipSuccess) return hip_fail(c, e, (what + " bytewise launch").c_str());
    if (a.nwin == 0) c->last_kernel = hrs::last_kernel();
  }
  return HRS_OK;
}

}  // namespace

hrs_status run_scrub(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                     uint32_t* reports, size_t report_stride, hipStream_t s, bool heal) {
  hrs::ScrubArgs a{};
  return run_windows_tail(
      c, a, rows, stride, len, nstripes, reports, report_stride, s, heal ? "heal" : "scrub",
      [&] { return heal ? hrs::launch_heal(a, s) : hrs::launch_scrub(a, s); },
      [&] { return heal ? hrs::launch_heal_bytewise(a, s) : hrs::launch_scrub_bytewise(a, s); });
}

// ---- ragged scrub and heal

hrs_status scrub_cells_apart_ok(hrs_codec* c, size_t row_stride, size_t stripe_stride, size_t len, size_t nstripes) {
  // Rows of a stripe packed inside the stripe stride, or stripes of a row packed inside the row stride.
  const size_t rows_span = static_cast<size_t>(c->n - 1) * row_stride + len;
  const size_t stripes_span = (nstripes - 1) * stripe_stride + len;
  const bool stripes_apart =
      nstripes == 1 || (stripe_stride >= len && (stripe_stride >= rows_span || row_stride >= stripes_span));
  if (row_stride < len || !stripes_apart)
    return fail(c, HRS_EINVAL, "cells overlap: row_stride %zu, stripe_stride %zu, len %zu, %d rows, %zu stripes",
                row_stride, stripe_stride, len, c->n, nstripes);
  return HRS_OK;
}

hrs_status scrub_ragged_args_ok(hrs_codec* c, const void* cells, const uint32_t* reports, size_t report_stride,
                                size_t len, size_t nstripes, unsigned flags, size_t row_stride, size_t stripe_stride,
                                const uint32_t* valid, bool* empty, bool* all_full) {
  *empty = *all_full = false;
  hrs_status st = scrub_args_ok(c, cells, reports, report_stride, len, nstripes, flags);
  if (st != HRS_OK) return st;
  const bool none = len == 0 || nstripes == 0;
  if ((flags & kScrubImage) && !none && (st = scrub_cells_apart_ok(c, row_stride, stripe_stride, len, nstripes)) != HRS_OK)
    return st;
  if (!valid) return fail(c, HRS_EINVAL, "valid is NULL");
  if (none) {
    *empty = true;
    return HRS_OK;
  }
  const size_t n = static_cast<size_t>(c->n);
  bool full = true;
  for (size_t s = 0; s < nstripes; ++s)
    for (size_t l = 0; l < n; ++l) {
      const uint32_t v = valid[s * n + l];
      if (v > len) return fail(c, HRS_EINVAL, "stripe %zu location %zu: valid %u exceeds len %zu", s, l, v, len);
      full &= v == len;
    }
  *all_full = full;
  return HRS_OK;
}

hrs_status scrub_ragged_table(hrs_codec* c, const uint32_t* valid, size_t nstripes, hipStream_t s,
                              hrs_codec::BatchSlot** slot, const uint32_t** dlens) {
  const size_t n = static_cast<size_t>(c->n), words = hrs::scrub_ragged_words(c->n);
  std::vector<uint32_t> table(nstripes * words);
  for (size_t i = 0; i < nstripes; ++i) {
    uint32_t most = 0;
    for (size_t l = 0; l < n; ++l) most = std::max(most, table[i * words + l] = valid[i * n + l]);
    table[i * words + n] = most;
  }
  const hrs_status st = upload(c, table.data(), table.size() * sizeof(uint32_t), table.data(), 0, s, slot);
  if (st != HRS_OK) return st;
  *dlens = reinterpret_cast<const uint32_t*>((*slot)->dev);
  return HRS_OK;
}

hrs_status run_scrub_ragged(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                            const uint32_t* dlens, uint32_t* reports, size_t report_stride, hipStream_t s, bool heal) {
  hrs::ScrubRaggedArgs a{};
  a.lens = dlens;
  return run_windows_tail(
      c, a.s, rows, stride, len, nstripes, reports, report_stride, s, heal ? "ragged heal" : "ragged scrub",
      [&] { return hrs::launch_scrub_ragged(a, heal, s); }, [&] { return hrs::launch_scrub_ragged_bytewise(a, heal, s); });
}

namespace {

// One stripe on the CPU: the column loop of hrs_heal_host (an empty pattern,
// locate() on the column's syndromes) and hrs_heal_erased_host (the erased
// cells count as zero and are rebuilt, locate_errata()). write = false (empty
// pattern only) is the scrub: the same report with nothing stored and word 3
// left at 0, pass 1 of hrs_repair_checked_host.
// Ragged (hrs_heal_ragged_host; empty pattern only): cell l counts as its
// valid[l] leading bytes followed by zeros, and a column resolved by blaming,
// with a nonzero error value, a cell it lies at or beyond is demoted to
// unresolved (include/hrs.h). Without it the loop is the code it always was.
template <int P, bool Ragged = false>
void heal_stripe(int n, uint8_t* const* rows, size_t len, const hrs::ErasePattern& pt, uint32_t* rep, bool write,
                 const uint32_t* valid = nullptr) {
  const hrs::locator::Field& f = kHostField;
  const int e = pt.e;
  for (size_t col = 0; col < len; ++col) {
    uint8_t s[P] = {};
    for (int l = n - 1; l >= 0; --l) {
      bool gone = (pt.mask[l >> 5] >> (l & 31)) & 1u;
      if constexpr (Ragged) gone |= col >= valid[l];
      hrs::locator::horner_step<P>(f, s, gone ? uint8_t{0} : rows[l][col]);
    }
    int nloc = 0, state;
    uint8_t loc[hrs::locator::kMaxErrors], u[hrs::locator::kMaxErrors], v[hrs::locator::kMaxErased];
    if (e == 0) {
      uint32_t nz = 0;
      for (int i = 0; i < P; ++i) nz |= s[i];
      if (nz == 0) continue;
      state = hrs::locator::locate(f, n, P, s, &nloc, loc, u) ? hrs::locator::kResolved : hrs::locator::kUnresolved;
      if constexpr (Ragged)
        for (int j = 0; j < nloc && state == hrs::locator::kResolved; ++j)
          if (u[j] != 0 && col >= valid[loc[j]]) state = hrs::locator::kUnresolved;  // a patch of a virtual zero
    } else {
      state = hrs::locator::locate_errata<P>(f, n, s, e, pt.loc, pt.gamma, &nloc, loc, u, v);
      for (int m = 0; m < e; ++m) rows[pt.loc[m]][col] = v[m];
      if (state == hrs::locator::kConsistent) continue;
    }
    ++rep[HRS_SCRUB_BAD];
    if (rep[HRS_SCRUB_FIRST_BAD] == HRS_SCRUB_NONE) rep[HRS_SCRUB_FIRST_BAD] = static_cast<uint32_t>(col);
    if (state == hrs::locator::kUnresolved) {  // left as it is, even where the Java wrote into it before returning false
      ++rep[HRS_SCRUB_UNRESOLVED];
      continue;
    }
    for (int j = 0; j < nloc; ++j) {
      ++rep[HRS_SCRUB_HEAD + loc[j]];
      if (u[j] == 0 || !write) continue;  // a blamed location whose value stands: nothing to store
      rows[loc[j]][col] ^= u[j];
      ++rep[HRS_SCRUB_PATCHED];
    }
  }
}

// hrs_heal_host and hrs_heal_erased_host after their argument checks.
// valid (hrs_heal_ragged_host, empty pattern): the cells' lengths.
hrs_status heal_host(hrs_codec* c, uint8_t* const* rows, size_t len, const hrs::ErasePattern& pt, uint32_t* report,
                     bool write = true, const uint32_t* valid = nullptr) {
  if (len == 0) return HRS_OK;
  for (int e = 0; e < HRS_SCRUB_HEAD + c->n; ++e) report[e] = e == HRS_SCRUB_FIRST_BAD ? HRS_SCRUB_NONE : 0u;
  (void)hrs::dispatch_p<1, 8>(c->p, [&](auto P) {
    if (valid) heal_stripe<P, true>(c->n, rows, len, pt, report, write, valid);
    else heal_stripe<P>(c->n, rows, len, pt, report, write);
  });
  return HRS_OK;
}

// CRC-32 (crc32.hpp) of one host cell, slicing by 4.
uint32_t host_crc32(const uint8_t* p, size_t len) {
  static const hrs::crc::Slice4 sl = hrs::crc::make_slice4();
  uint32_t c = 0xFFFFFFFFu;
  size_t i = 0;
  for (; i + 4 <= len; i += 4) {
    uint32_t w;
    std::memcpy(&w, p + i, 4);
    c ^= w;
    c = sl.s[3].t[c & 0xFFu] ^ sl.s[2].t[(c >> 8) & 0xFFu] ^ sl.s[1].t[(c >> 16) & 0xFFu] ^ sl.s[0].t[c >> 24];
  }
  for (; i < len; ++i) c = sl.s[0].t[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

}  // namespace

// The shapes of the one-pass kernel (hrs_scrub_crc.hip). Device-resident jobs
// take it too: measured 13 % faster than scrub + hrs_crc32_dev.
bool scrub_crc_one_pass(const hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len) {
  if (c->p < 2 || c->p > hrs::kScrubCrcMaxP || c->n > hrs::kScrubCrcMaxRows) return false;
  if (!(c->kernel_mode == 0 || c->kernel_mode == 3)) return false;
  if (len == 0 || len % hrs::kWindowBytes != 0 || stride % 16 != 0) return false;
  for (int l = 0; l < c->n; ++l)
    if (!aligned16(rows[l])) return false;
  return true;
}

namespace {

// hrs_scrub_dev and hrs_heal_dev.
hrs_status scrub_dev_entry(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                           uint32_t* reports, size_t report_stride, void* stream, bool heal) {
  const hrs_status st = scrub_args_ok(c, rows, reports, report_stride, len, nstripes,
                                      kScrubWithReports | (heal ? kScrubRowsWritten : 0u));
  if (st != HRS_OK || len == 0 || nstripes == 0) return st;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  return run_scrub(c, rows, stride, len, nstripes, reports, report_stride, static_cast<hipStream_t>(stream), heal);
}

// hrs_scrub_ragged_dev and hrs_heal_ragged_dev: the rules of scrub_ragged_args_ok,
// the device, then the sibling's route for an all-full batch in kernel modes 0
// and 1, else the length table through a batch slot and the ragged kernels.
hrs_status scrub_ragged_dev_entry(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                                  const uint32_t* valid, uint32_t* reports, size_t report_stride, void* stream,
                                  bool heal) {
  bool empty = false, all_full = false;
  hrs_status st = scrub_ragged_args_ok(c, rows, reports, report_stride, len, nstripes,
                                       kScrubWithReports | (heal ? kScrubRowsWritten : 0u), 0, 0, valid, &empty,
                                       &all_full);
  if (st != HRS_OK || empty) return st;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (scrub_ragged_takes_plain(c, all_full))
    return run_scrub(c, rows, stride, len, nstripes, reports, report_stride, s, heal);
  hrs_codec::BatchSlot* sl = nullptr;
  const uint32_t* dlens = nullptr;
  if ((st = scrub_ragged_table(c, valid, nstripes, s, &sl, &dlens)) != HRS_OK) return st;
  st = run_scrub_ragged(c, rows, stride, len, nstripes, dlens, reports, report_stride, s, heal);
  slot_used(sl, s);
  return st;
}

// hrs_scrub_crc_dev and hrs_heal_crc_dev: the sibling call's argument rules, then the CRC arrays'.
hrs_status scrub_crc_dev_entry(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                               uint32_t* reports, size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out,
                               void* stream, bool heal) {
  const hrs_status st = scrub_args_ok(c, rows, reports, report_stride, len, nstripes,
                                      kScrubWithReports | (heal ? kScrubRowsWritten : 0u));
  if (st != HRS_OK || len == 0 || nstripes == 0) return st;
  if (!crc_out) return fail(c, HRS_EINVAL, "crc_out is NULL");
  if (!crc_arrays_apart(crc_in, crc_out, nstripes * static_cast<size_t>(c->n)))
    return fail(c, HRS_EINVAL, "crc_in and crc_out overlap (crc_out may only be crc_in itself)");
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  return run_scrub_crc(c, rows, stride, len, nstripes, reports, report_stride, crc_in, crc_out,
                       static_cast<hipStream_t>(stream), heal);
}

}  // namespace

// ---- heal with known erasures

// The erased set of one stripe: entries up to the first negative one (or
// `cap`), sorted ascending into `key`. HRS_EINVAL for a location outside
// [0, n) or a repeated one, HRS_ETOOMANY for more than p of them.
hrs_status erased_key(hrs_codec* c, const int* erased, int cap, size_t stripe, std::vector<int>& key) {
  key.clear();
  for (int t = 0; t < cap && erased[t] >= 0; ++t) {
    if (erased[t] >= c->n)
      return fail(c, HRS_EINVAL, "stripe %zu: erased location %d is outside [0, %d)", stripe, erased[t], c->n);
    key.push_back(erased[t]);
  }
  std::sort(key.begin(), key.end());
  for (size_t t = 1; t < key.size(); ++t)
    if (key[t] == key[t - 1]) return fail(c, HRS_EINVAL, "stripe %zu: erased location %d is listed twice", stripe, key[t]);
  if (static_cast<int>(key.size()) > c->p)
    return fail(c, HRS_ETOOMANY, "stripe %zu: %zu erased locations, the code repairs %d", stripe, key.size(), c->p);
  return HRS_OK;
}

// The device table entry of an erased set (hrs_heal_erased.hpp).
hrs::ErasePattern make_pattern(int p, const std::vector<int>& key) {
  hrs::ErasePattern pt{};
  pt.e = static_cast<int>(key.size());
  for (int m = 0; m < pt.e; ++m) pt.loc[m] = static_cast<uint8_t>(key[m]);
  hrs::repair::PatternWork work;
  hrs::repair::fill_pattern(kHostField, p, pt, work);  // the code repair_plan_kernel runs (hrs_repair.hip)
  return pt;
}

// The erased sets of a batch, validated and de-duplicated (stripe by stripe,
// so the first bad stripe is the one named).
hrs_status erased_sets(hrs_codec* c, const int* erased, int max_erased, size_t nstripes, ErasedSets& es) {
  es.pats.clear();
  es.keys.clear();
  es.pat.assign(max_erased > 0 ? nstripes : 0, 0);
  if (max_erased <= 0) return HRS_OK;
  std::map<std::vector<int>, int32_t> ids;
  std::vector<int> key;
  for (size_t s = 0; s < nstripes; ++s) {
    const hrs_status st = erased_key(c, erased + s * static_cast<size_t>(max_erased), max_erased, s, key);
    if (st != HRS_OK) return st;
    auto it = ids.find(key);
    if (it == ids.end()) {
      it = ids.emplace(key, static_cast<int32_t>(es.pats.size())).first;
      es.pats.push_back(make_pattern(c->p, key));
      es.keys.push_back(key);
    }
    es.pat[s] = it->second;
  }
  return HRS_OK;
}

namespace {

// The pattern table and the pattern indices of `nstripes` stripes into the
// next batch slot and up to the device on s (upload). The caller calls
// slot_used after its launches.
hrs_status pattern_table(hrs_codec* c, const std::vector<hrs::ErasePattern>& pats, const int32_t* pat, size_t nstripes,
                         hipStream_t s, hrs_codec::BatchSlot** slot, const hrs::ErasePattern** dpats,
                         const int32_t** dpat) {
  const size_t pat_bytes = pats.size() * sizeof(hrs::ErasePattern);
  const hrs_status st = upload(c, pats.data(), pat_bytes, pat, nstripes * sizeof(int32_t), s, slot);
  if (st != HRS_OK) return st;
  *dpats = reinterpret_cast<const hrs::ErasePattern*>((*slot)->dev);
  *dpat = reinterpret_cast<const int32_t*>((*slot)->dev + pat_bytes);
  return HRS_OK;
}

}  // namespace

hrs_status run_heal_erased(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                           const std::vector<hrs::ErasePattern>& pats, const int32_t* pat, uint32_t* reports,
                           size_t report_stride, hipStream_t s) {
  hrs_codec::BatchSlot* sl = nullptr;
  hrs::HealErasedArgs a{};
  hrs_status st = pattern_table(c, pats, pat, nstripes, s, &sl, &a.pats, &a.pat);
  if (st != HRS_OK) return st;
  st = run_windows_tail(
      c, a.s, rows, stride, len, nstripes, reports, report_stride, s, "heal erased",
      [&] { return hrs::launch_heal_erased(a, s); }, [&] { return hrs::launch_heal_erased_bytewise(a, s); });
  slot_used(sl, s);
  return st;
}

// Kernel mode 0: whether a fused shape takes heal_erased_crc_kernel<P>. Mode
// 3 always does, mode 2 never. Measured (DESIGN 10.4,
// profiles/heal_erased/bench_heal_erased_crc.json): over pinned host memory
// the fused call takes 0.483 of the plain call plus a second zero-copy read,
// the ranges far apart; on device-resident stripes it ran at 1.006 of the two
// passes with overlapping ranges, so those keep the two passes.
bool heal_erased_crc_fused_default(bool host_memory) { return host_memory; }

namespace {

// The one-pass scrub, heal and heal with erasures with CRCs (hrs_scrub_crc.hip,
// hrs_heal_erased_crc.hip), once its caller's route rule holds: empty reports,
// the window tables and, with erasures (pats), their table through a batch
// slot; then, under one lease of the raw-CRC scratch, the memset of the dirty
// count (heal), `launch` (`what` names it in a launch error), the redo of the
// dirty windows (heal) and the fold. heal: the rows are written.
template <class Launch>
hrs_status scrub_crc_pass(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                          uint32_t* reports, size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out,
                          hipStream_t s, bool heal, const std::vector<hrs::ErasePattern>* pats, const int32_t* pat,
                          const char* what, Launch launch) {
  const int n = c->n;
  hipError_t e = hrs::launch_scrub_init(reports, report_stride, n, nstripes, s);
  if (e != hipSuccess) return hip_fail(c, e, "scrub init launch");
  hrs_status st = crc_window_tables(c);
  if (st != HRS_OK) return st;
  hrs::HealErasedCrcArgs h{};
  hrs::ScrubCrcArgs& a = h.c;
  for (int l = 0; l < n; ++l) a.rows[l] = rows[l];
  a.stride = stride;
  a.nwin = len / hrs::kWindowBytes;
  a.ntasks = a.nwin * nstripes;
  a.reports = reports;
  a.report_stride = report_stride;
  a.n = n;
  a.p = c->p;
  a.tables = c->crc_tables_a;
  hrs_codec::BatchSlot* sl = nullptr;
  if (pats && (st = pattern_table(c, *pats, pat, nstripes, s, &sl, &h.pats, &h.pat)) != HRS_OK) return st;
  // scratch: the raw window CRCs, then (heal) the dirty-task count and list
  const size_t raw_bytes = (a.ntasks * static_cast<size_t>(n) * 4 + 7) & ~static_cast<size_t>(7);
  const size_t list_bytes = heal ? (1 + a.ntasks) * sizeof(uint64_t) : 0;
  const int cus = hrs::device_cu_count();
  st = with_crc_scratch(c, raw_bytes + list_bytes, s, [&]() -> hrs_status {
    a.raw = c->crc_raw;
    a.dirty = heal ? reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(c->crc_raw) + raw_bytes) : nullptr;
    if (heal && (e = hipMemsetAsync(a.dirty, 0, sizeof(uint64_t), s)) != hipSuccess)
      return hip_fail(c, e, "hipMemsetAsync");
    if ((e = launch(h, cus)) != hipSuccess) return hip_fail(c, e, what);
    c->last_kernel = hrs::last_kernel();
    if (heal && (e = hrs::launch_scrub_crc_redo(a, cus, s)) != hipSuccess) return hip_fail(c, e, "crc redo launch");
    return crc_fold(c, len, nstripes * static_cast<uint64_t>(n), crc_in, crc_out, s, c->crc_raw, hrs::kWindowBytes);
  });
  if (sl) slot_used(sl, s);  // on every exit: the table may be in use whether or not every launch went out
  return st;
}

}  // namespace

hrs_status run_scrub_crc(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                         uint32_t* reports, size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out,
                         hipStream_t s, bool heal) {
  if (!scrub_crc_one_pass(c, rows, stride, len)) {
    // two passes: the scrub or heal as it is, then the CRC of the n rows (the
    // stream orders the heal's stores before the CRC pass reads them)
    const hrs_status st = run_scrub(c, rows, stride, len, nstripes, reports, report_stride, s, heal);
    return st != HRS_OK ? st : crc_rows(c, rows, c->n, stride, len, nstripes, crc_in, crc_out, s);
  }
  auto launch = [&](const hrs::HealErasedCrcArgs& h, int cus) { return hrs::launch_scrub_crc(h.c, heal, cus, s); };
  return scrub_crc_pass(c, rows, stride, len, nstripes, reports, report_stride, crc_in, crc_out, s, heal, nullptr,
                        nullptr, heal ? "heal+crc launch" : "scrub+crc launch", launch);
}

hrs_status run_heal_erased_crc(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                               const std::vector<hrs::ErasePattern>& pats, const int32_t* pat, uint32_t* reports,
                               size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out, hipStream_t s,
                               bool host_memory) {
  const bool fused = scrub_crc_one_pass(c, rows, stride, len) &&
                     (c->kernel_mode == 3 || heal_erased_crc_fused_default(host_memory));
  if (!fused) {
    // two passes: the heal as it is, then the CRC of the n rows (as above)
    const hrs_status st = run_heal_erased(c, rows, stride, len, nstripes, pats, pat, reports, report_stride, s);
    return st != HRS_OK ? st : crc_rows(c, rows, c->n, stride, len, nstripes, crc_in, crc_out, s);
  }
  auto launch = [&](const hrs::HealErasedCrcArgs& h, int cus) { return hrs::launch_heal_erased_crc(h, cus, s); };
  return scrub_crc_pass(c, rows, stride, len, nstripes, reports, report_stride, crc_in, crc_out, s, true, &pats, pat,
                        "heal erased+crc launch", launch);
}

namespace {

// hrs_heal_erased_dev and hrs_heal_erased_crc_dev (with_crc): the heal's
// argument rules with the erased list's, the erased sets, the empty batch,
// then the CRC arrays' rules, then the device.
hrs_status heal_erased_dev_entry(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                                 const int* erased, int max_erased, uint32_t* reports, size_t report_stride,
                                 bool with_crc, const uint32_t* crc_in, uint32_t* crc_out, void* stream) {
  hrs_status st = scrub_args_ok(c, rows, reports, report_stride, len, nstripes, kScrubWithReports | kScrubRowsWritten,
                                "max_erased", max_erased, erased);
  if (st != HRS_OK) return st;
  ErasedSets es;
  st = erased_sets(c, erased, max_erased, nstripes, es);
  if (st != HRS_OK) return st;
  if (len == 0 || nstripes == 0) return HRS_OK;
  if (with_crc) {
    if (!crc_out) return fail(c, HRS_EINVAL, "crc_out is NULL");
    if (!crc_arrays_apart(crc_in, crc_out, nstripes * static_cast<size_t>(c->n)))
      return fail(c, HRS_EINVAL, "crc_in and crc_out overlap (crc_out may only be crc_in itself)");
  }
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (max_erased == 0) {  // nothing can be erased: the heal itself
    if (!with_crc) return run_scrub(c, rows, stride, len, nstripes, reports, report_stride, s, true);
    return run_scrub_crc(c, rows, stride, len, nstripes, reports, report_stride, crc_in, crc_out, s, true);
  }
  if (!with_crc)
    return run_heal_erased(c, rows, stride, len, nstripes, es.pats, es.pat.data(), reports, report_stride, s);
  return run_heal_erased_crc(c, rows, stride, len, nstripes, es.pats, es.pat.data(), reports, report_stride, crc_in,
                             crc_out, s, false);
}

}  // namespace

// ---- checked repair (the device call is hrs_repair_api.cpp)

hrs_status repair_args_ok(hrs_codec* c, const uint8_t* const* rows, const uint32_t* reports, size_t report_stride,
                          size_t len, size_t nstripes, bool with_reports, const uint32_t* stored, int flags,
                          const uint32_t* verdicts, const uint32_t* crc_out, bool* empty) {
  *empty = false;
  const hrs_status st = scrub_args_ok(c, rows, reports, report_stride, len, nstripes,
                                      (with_reports ? kScrubWithReports : 0u) | kScrubRowsWritten);
  if (st != HRS_OK) return st;
  if (flags & ~HRS_REPAIR_JOIN_SYNDROMES) return fail(c, HRS_EINVAL, "flags %#x: only HRS_REPAIR_JOIN_SYNDROMES is defined", flags);
  if (len == 0 || nstripes == 0) {
    *empty = true;
    return HRS_OK;
  }
  if (!stored || !verdicts || !crc_out)
    return fail(c, HRS_EINVAL, "%s is NULL", !stored ? "stored" : !verdicts ? (with_reports ? "verdicts" : "verdict") : "crc_out");
  if (stored == crc_out || !crc_arrays_apart(stored, crc_out, nstripes * static_cast<size_t>(c->n)))
    return fail(c, HRS_EINVAL, "stored and crc_out overlap");
  return HRS_OK;
}

}  // namespace hrs::api

using namespace hrs::api;

extern "C" {

hrs_status hrs_compute_error_locations(const hrs_codec* cc, int* data, int* locations, int* num_locations,
                                       int* resolved) {
  auto* c = const_cast<hrs_codec*>(cc);
  if (!c) return HRS_EINVAL;
  if (!data || !locations || !num_locations || !resolved)
    return fail(c, HRS_EINVAL, "computeErrorLocations: an argument is NULL");
  hrs_status st = scrub_code_ok(c, 0, false);
  if (st != HRS_OK) return st;
  for (int l = 0; l < c->n; ++l)
    if (data[l] < 0 || data[l] > 255) return fail(c, HRS_EINVAL, "data[%d] = %d is outside [0, 255]", l, data[l]);
  uint8_t s[hrs::locator::kMaxSyndromes] = {};
  (void)hrs::dispatch_p<1, 8>(c->p, [&](auto P) { column_syndromes<P>(c->n, data, s); });
  *num_locations = 0;
  bool clean = true;
  for (int i = 0; i < c->p; ++i) clean &= s[i] == 0;
  if (clean) {
    *resolved = 1;
    return HRS_OK;
  }
  int nloc = 0;
  uint8_t loc[hrs::locator::kMaxErrors], err[hrs::locator::kMaxErrors];
  *resolved = hrs::locator::locate(kHostField, c->n, c->p, s, &nloc, loc, err) ? 1 : 0;
  for (int j = 0; j < nloc; ++j) {  // ReedSolomonCode.java:281-285: the decoded values are written back
    locations[j] = loc[j];
    data[loc[j]] ^= err[j];
  }
  *num_locations = nloc;
  return HRS_OK;
}

hrs_status hrs_scrub_dev(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                         uint32_t* reports, size_t report_stride, void* stream) {
  return scrub_dev_entry(c, rows, stride, len, nstripes, reports, report_stride, stream, false);
}

hrs_status hrs_heal_dev(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                        uint32_t* reports, size_t report_stride, void* stream) {
  return scrub_dev_entry(c, rows, stride, len, nstripes, reports, report_stride, stream, true);
}

hrs_status hrs_scrub_ragged_dev(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                                const uint32_t* valid, uint32_t* reports, size_t report_stride, void* stream) {
  return scrub_ragged_dev_entry(c, rows, stride, len, nstripes, valid, reports, report_stride, stream, false);
}

hrs_status hrs_heal_ragged_dev(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                               const uint32_t* valid, uint32_t* reports, size_t report_stride, void* stream) {
  return scrub_ragged_dev_entry(c, rows, stride, len, nstripes, valid, reports, report_stride, stream, true);
}

hrs_status hrs_heal_ragged_host(const hrs_codec* cc, uint8_t* const* rows, size_t len, const uint32_t* valid,
                                uint32_t* report) {
  auto* c = const_cast<hrs_codec*>(cc);
  bool empty = false, all_full = false;
  const hrs_status st =
      scrub_ragged_args_ok(c, rows, report, 0, len, 1, kScrubRowsWritten, 0, 0, valid, &empty, &all_full);
  if (st != HRS_OK || empty) return st;
  return heal_host(c, rows, len, hrs::ErasePattern{}, report, true, valid);
}

hrs_status hrs_scrub_crc_dev(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                             uint32_t* reports, size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out,
                             void* stream) {
  return scrub_crc_dev_entry(c, rows, stride, len, nstripes, reports, report_stride, crc_in, crc_out, stream, false);
}

hrs_status hrs_heal_crc_dev(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                            uint32_t* reports, size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out,
                            void* stream) {
  return scrub_crc_dev_entry(c, rows, stride, len, nstripes, reports, report_stride, crc_in, crc_out, stream, true);
}

hrs_status hrs_heal_host(const hrs_codec* cc, uint8_t* const* rows, size_t len, uint32_t* report) {
  auto* c = const_cast<hrs_codec*>(cc);
  const hrs_status st = scrub_args_ok(c, rows, report, 0, len, 1, kScrubRowsWritten);
  if (st != HRS_OK) return st;
  return heal_host(c, rows, len, hrs::ErasePattern{}, report);
}

hrs_status hrs_heal_erased_dev(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                               const int* erased, int max_erased, uint32_t* reports, size_t report_stride,
                               void* stream) {
  return heal_erased_dev_entry(c, rows, stride, len, nstripes, erased, max_erased, reports, report_stride, false,
                               nullptr, nullptr, stream);
}

hrs_status hrs_heal_erased_crc_dev(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                                   const int* erased, int max_erased, uint32_t* reports, size_t report_stride,
                                   const uint32_t* crc_in, uint32_t* crc_out, void* stream) {
  return heal_erased_dev_entry(c, rows, stride, len, nstripes, erased, max_erased, reports, report_stride, true,
                               crc_in, crc_out, stream);
}

hrs_status hrs_heal_erased_host(const hrs_codec* cc, uint8_t* const* rows, size_t len, const int* erased,
                                int num_erased, uint32_t* report) {
  auto* c = const_cast<hrs_codec*>(cc);
  hrs_status st = scrub_args_ok(c, rows, report, 0, len, 1, kScrubRowsWritten, "num_erased", num_erased, erased);
  if (st != HRS_OK) return st;
  std::vector<int> key;
  st = erased_key(c, erased, num_erased, 0, key);
  if (st != HRS_OK) return st;
  return heal_host(c, rows, len, make_pattern(c->p, key), report);
}

hrs_status hrs_repair_checked_host(const hrs_codec* cc, uint8_t* const* rows, size_t len, const uint32_t* stored,
                                   int flags, uint32_t* verdict, int32_t* erased_out, uint32_t* report,
                                   uint32_t* crc_out) {
  namespace rp = hrs::repair;
  auto* c = const_cast<hrs_codec*>(cc);
  bool empty = false;
  const hrs_status st = repair_args_ok(c, rows, report, 0, len, 1, false, stored, flags, verdict, crc_out, &empty);
  if (st != HRS_OK || empty) return st;
  const int n = c->n, p = c->p;
  // pass 1: the cells' CRCs and the scrub's report, nothing stored
  for (int l = 0; l < n; ++l) crc_out[l] = host_crc32(rows[l], len);
  (void)heal_host(c, rows, len, hrs::ErasePattern{}, report, false);
  int nd = 0;
  std::vector<int> key;
  for (int l = 0; l < n; ++l) {
    nd += rp::doubted(crc_out[l], stored[l]) ? 1 : 0;
    if (rp::suspected(crc_out[l], stored[l], report[HRS_SCRUB_HEAD + l], flags)) key.push_back(l);
  }
  if (erased_out)
    for (int m = 0; m < p; ++m) erased_out[m] = -1;
  *verdict = rp::plan_verdict(nd, static_cast<int>(key.size()), p, report[HRS_SCRUB_BAD], report[HRS_SCRUB_UNRESOLVED]);
  if (*verdict != rp::kListed) return HRS_OK;
  if (erased_out)
    for (size_t m = 0; m < key.size(); ++m) erased_out[m] = key[m];
  // pass 2: the heal with the erased set B, then the CRCs of the cells as it leaves them
  (void)heal_host(c, rows, len, make_pattern(p, key), report);
  bool any_f = false, any_fd = false;
  for (int l = 0; l < n; ++l) {
    const uint32_t now = host_crc32(rows[l], len);
    const bool in_f = rp::doubted(now, stored[l]);
    any_f |= in_f;
    any_fd |= in_f && rp::doubted(crc_out[l], stored[l]);
    crc_out[l] = now;
  }
  *verdict = rp::final_verdict(any_f, any_fd, report[HRS_SCRUB_UNRESOLVED]);
  return HRS_OK;
}

}  // extern "C"
