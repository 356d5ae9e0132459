// Stripe scrubbing and healing behind the C ABI: the scalar
// computeErrorLocations on the host (hrs_compute_error_locations, host-only
// handles included), the device-resident batches (hrs_scrub_dev, hrs_heal_dev,
// and hrs_scrub_crc_dev, hrs_heal_crc_dev with the cells' CRC-32s from the same
// pass) and one stripe healed on the CPU (hrs_heal_host). The host-memory batches are
// in hrs_batch_api.cpp beside the pipeline they share. The per-column algorithm
// is hrs_locator.hpp, the same code the kernels of hrs_scrub.hip run.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/hrs.h"
#include "gf256.hpp"
#include "hrs_codec.hpp"
#include "hrs_crc.hpp"
#include "hrs_internal.hpp"
#include "hrs_locator.hpp"

namespace hrs::api {

namespace {

constexpr hrs::gf::Tables kHostTables = hrs::gf::make_tables();

template <int P>
void column_syndromes(const hrs::locator::Field& f, int n, const int* data, uint8_t* out) {
  uint8_t s[P] = {};
  for (int l = n - 1; l >= 0; --l) hrs::locator::horner_step<P>(f, s, static_cast<uint8_t>(data[l]));
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

hrs_status run_scrub(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                     uint32_t* reports, size_t report_stride, hipStream_t s, bool heal) {
  hipError_t e = hrs::launch_scrub_init(reports, report_stride, c->n, nstripes, s);
  if (e != hipSuccess) return hip_fail(c, e, "scrub init launch");
  hrs::ScrubArgs a{};
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
    e = heal ? hrs::launch_heal(a, s) : hrs::launch_scrub(a, s);
    if (e != hipSuccess) return hip_fail(c, e, heal ? "heal launch" : "scrub launch");
    c->last_kernel = hrs::last_kernel();
  }
  a.col0 = a.nwin * hrs::kWindowBytes;
  if (a.col0 < len) {
    a.ntasks = (len - a.col0) * nstripes;
    e = heal ? hrs::launch_heal_bytewise(a, s) : hrs::launch_scrub_bytewise(a, s);
    if (e != hipSuccess) return hip_fail(c, e, heal ? "heal bytewise launch" : "scrub bytewise launch");
    if (a.nwin == 0) c->last_kernel = hrs::last_kernel();
  }
  return HRS_OK;
}

namespace {

// One stripe on the CPU: the column loop of hrs_heal_host.
template <int P>
void heal_stripe(const hrs::locator::Field& f, int n, uint8_t* const* rows, size_t len, uint32_t* rep) {
  for (size_t col = 0; col < len; ++col) {
    uint8_t s[P] = {};
    for (int l = n - 1; l >= 0; --l) hrs::locator::horner_step<P>(f, s, rows[l][col]);
    uint32_t nz = 0;
    for (int i = 0; i < P; ++i) nz |= s[i];
    if (nz == 0) continue;
    int nloc = 0;
    uint8_t loc[hrs::locator::kMaxErrors], err[hrs::locator::kMaxErrors];
    const bool resolved = hrs::locator::locate(f, n, P, s, &nloc, loc, err);
    ++rep[HRS_SCRUB_BAD];
    if (rep[HRS_SCRUB_FIRST_BAD] == HRS_SCRUB_NONE) rep[HRS_SCRUB_FIRST_BAD] = static_cast<uint32_t>(col);
    if (!resolved) {  // left as it is, even where the Java wrote into it before returning false
      ++rep[HRS_SCRUB_UNRESOLVED];
      continue;
    }
    for (int j = 0; j < nloc; ++j) {
      ++rep[HRS_SCRUB_HEAD + loc[j]];
      if (err[j] == 0) continue;  // a blamed location whose value stands: nothing to store
      rows[loc[j]][col] ^= err[j];
      ++rep[HRS_SCRUB_PATCHED];
    }
  }
}

}  // namespace

// A patch through one of two equal row pointers would change the other's column.
hrs_status heal_rows_ok(hrs_codec* c, const uint8_t* const* rows) {
  for (int l = 0; l < c->n; ++l)
    if (!rows[l]) return fail(c, HRS_EINVAL, "row %d is NULL", l);
  for (int l = 1; l < c->n; ++l)
    for (int m = 0; m < l; ++m)
      if (rows[l] == rows[m]) return fail(c, HRS_EINVAL, "rows %d and %d are one pointer: healing writes the rows", m, l);
  return HRS_OK;
}

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

hrs_status run_scrub_crc(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                         uint32_t* reports, size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out,
                         hipStream_t s, bool heal) {
  const int n = c->n;
  if (!scrub_crc_one_pass(c, rows, stride, len)) {
    // two passes: the scrub or heal as it is, then the CRC of the n rows (the
    // stream orders the heal's stores before the CRC pass reads them)
    hrs_status st = run_scrub(c, rows, stride, len, nstripes, reports, report_stride, s, heal);
    if (st != HRS_OK) return st;
    const std::string kernel = c->last_kernel;
    st = crc_scratch(c, crc_raw_bytes_for(len, nstripes, n), s);
    if (st != HRS_OK) return st;
    const std::vector<size_t> strides(n, stride);
    st = crc_scratch_release(c, s, run_crc(c, rows, strides.data(), n, len, nstripes, crc_in, crc_out, s, c->crc_raw));
    c->last_kernel = kernel;
    return st;
  }
  hipError_t e = hrs::launch_scrub_init(reports, report_stride, n, nstripes, s);
  if (e != hipSuccess) return hip_fail(c, e, "scrub init launch");
  hrs_status st = crc_window_tables(c);
  if (st != HRS_OK) return st;
  hrs::ScrubCrcArgs a{};
  for (int l = 0; l < n; ++l) a.rows[l] = rows[l];
  a.stride = stride;
  a.nwin = len / hrs::kWindowBytes;
  a.ntasks = a.nwin * nstripes;
  a.reports = reports;
  a.report_stride = report_stride;
  a.n = n;
  a.p = c->p;
  a.tables = c->crc_tables_a;
  // scratch: the raw window CRCs, then (heal) the dirty-task count and list
  const size_t raw_bytes = (a.ntasks * static_cast<size_t>(n) * 4 + 7) & ~static_cast<size_t>(7);
  const size_t list_bytes = heal ? (1 + a.ntasks) * sizeof(uint64_t) : 0;
  st = crc_scratch(c, raw_bytes + list_bytes, s);
  if (st != HRS_OK) return st;
  a.raw = c->crc_raw;
  a.dirty = heal ? reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(c->crc_raw) + raw_bytes) : nullptr;
  const int cus = hrs::device_cu_count();
  auto launches = [&]() -> hrs_status {
    if (heal && (e = hipMemsetAsync(a.dirty, 0, sizeof(uint64_t), s)) != hipSuccess)
      return hip_fail(c, e, "hipMemsetAsync");
    if ((e = hrs::launch_scrub_crc(a, heal, cus, s)) != hipSuccess)
      return hip_fail(c, e, heal ? "heal+crc launch" : "scrub+crc launch");
    c->last_kernel = hrs::last_kernel();
    if (heal && (e = hrs::launch_scrub_crc_redo(a, cus, s)) != hipSuccess) return hip_fail(c, e, "crc redo launch");
    return crc_fold_windows(c, len, nstripes * static_cast<uint64_t>(n), crc_in, crc_out, s, c->crc_raw,
                            hrs::kWindowBytes);
  };
  return crc_scratch_release(c, s, launches());
}

namespace {

// hrs_scrub_crc_dev and hrs_heal_crc_dev: the sibling call's argument rules, then the CRC arrays'.
hrs_status scrub_crc_dev_entry(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                               uint32_t* reports, size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out,
                               void* stream, bool heal) {
  if (!c) return HRS_EINVAL;
  hrs_status st = scrub_code_ok(c, report_stride, true);
  if (st != HRS_OK) return st;
  if (!rows || !reports) return fail(c, HRS_EINVAL, "rows or reports is NULL");
  if (heal) {
    st = heal_rows_ok(c, rows);
    if (st != HRS_OK) return st;
  } else {
    for (int l = 0; l < c->n; ++l)
      if (!rows[l]) return fail(c, HRS_EINVAL, "row %d is NULL", l);
  }
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  if (len > 0xffffffffu) return fail(c, HRS_EINVAL, "rows of %zu bytes: column indices are 32-bit", len);
  if (len == 0 || nstripes == 0) return HRS_OK;
  if (!crc_out) return fail(c, HRS_EINVAL, "crc_out is NULL");
  if (!crc_arrays_apart(crc_in, crc_out, nstripes * static_cast<size_t>(c->n)))
    return fail(c, HRS_EINVAL, "crc_in and crc_out overlap (crc_out may only be crc_in itself)");
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  return run_scrub_crc(c, rows, stride, len, nstripes, reports, report_stride, crc_in, crc_out,
                       static_cast<hipStream_t>(stream), heal);
}

}  // namespace

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
  const hrs::locator::Field f{kHostTables.exp, kHostTables.log};
  uint8_t s[hrs::locator::kMaxSyndromes] = {};
  switch (c->p) {
    case 1: column_syndromes<1>(f, c->n, data, s); break;
    case 2: column_syndromes<2>(f, c->n, data, s); break;
    case 3: column_syndromes<3>(f, c->n, data, s); break;
    case 4: column_syndromes<4>(f, c->n, data, s); break;
    case 5: column_syndromes<5>(f, c->n, data, s); break;
    case 6: column_syndromes<6>(f, c->n, data, s); break;
    case 7: column_syndromes<7>(f, c->n, data, s); break;
    default: column_syndromes<8>(f, c->n, data, s); break;
  }
  *num_locations = 0;
  bool clean = true;
  for (int i = 0; i < c->p; ++i) clean &= s[i] == 0;
  if (clean) {
    *resolved = 1;
    return HRS_OK;
  }
  int nloc = 0;
  uint8_t loc[hrs::locator::kMaxErrors], err[hrs::locator::kMaxErrors];
  *resolved = hrs::locator::locate(f, c->n, c->p, s, &nloc, loc, err) ? 1 : 0;
  for (int j = 0; j < nloc; ++j) {  // ReedSolomonCode.java:281-285: the decoded values are written back
    locations[j] = loc[j];
    data[loc[j]] ^= err[j];
  }
  *num_locations = nloc;
  return HRS_OK;
}

hrs_status hrs_scrub_dev(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                         uint32_t* reports, size_t report_stride, void* stream) {
  if (!c) return HRS_EINVAL;
  hrs_status st = scrub_code_ok(c, report_stride, true);
  if (st != HRS_OK) return st;
  if (!rows || !reports) return fail(c, HRS_EINVAL, "rows or reports is NULL");
  for (int l = 0; l < c->n; ++l)
    if (!rows[l]) return fail(c, HRS_EINVAL, "row %d is NULL", l);
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  if (len > 0xffffffffu) return fail(c, HRS_EINVAL, "rows of %zu bytes: column indices are 32-bit", len);
  if (len == 0 || nstripes == 0) return HRS_OK;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  return run_scrub(c, rows, stride, len, nstripes, reports, report_stride, static_cast<hipStream_t>(stream), false);
}

hrs_status hrs_heal_dev(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                        uint32_t* reports, size_t report_stride, void* stream) {
  if (!c) return HRS_EINVAL;
  hrs_status st = scrub_code_ok(c, report_stride, true);
  if (st != HRS_OK) return st;
  if (!rows || !reports) return fail(c, HRS_EINVAL, "rows or reports is NULL");
  st = heal_rows_ok(c, rows);
  if (st != HRS_OK) return st;
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  if (len > 0xffffffffu) return fail(c, HRS_EINVAL, "rows of %zu bytes: column indices are 32-bit", len);
  if (len == 0 || nstripes == 0) return HRS_OK;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  return run_scrub(c, rows, stride, len, nstripes, reports, report_stride, static_cast<hipStream_t>(stream), true);
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
  if (!c) return HRS_EINVAL;
  hrs_status st = scrub_code_ok(c, 0, false);
  if (st != HRS_OK) return st;
  if (!rows || !report) return fail(c, HRS_EINVAL, "rows or report is NULL");
  st = heal_rows_ok(c, rows);
  if (st != HRS_OK) return st;
  if (len > 0xffffffffu) return fail(c, HRS_EINVAL, "rows of %zu bytes: column indices are 32-bit", len);
  if (len == 0) return HRS_OK;
  for (int e = 0; e < HRS_SCRUB_HEAD + c->n; ++e) report[e] = e == HRS_SCRUB_FIRST_BAD ? HRS_SCRUB_NONE : 0u;
  const hrs::locator::Field f{kHostTables.exp, kHostTables.log};
  switch (c->p) {
    case 1: heal_stripe<1>(f, c->n, rows, len, report); break;
    case 2: heal_stripe<2>(f, c->n, rows, len, report); break;
    case 3: heal_stripe<3>(f, c->n, rows, len, report); break;
    case 4: heal_stripe<4>(f, c->n, rows, len, report); break;
    case 5: heal_stripe<5>(f, c->n, rows, len, report); break;
    case 6: heal_stripe<6>(f, c->n, rows, len, report); break;
    case 7: heal_stripe<7>(f, c->n, rows, len, report); break;
    default: heal_stripe<8>(f, c->n, rows, len, report); break;
  }
  return HRS_OK;
}

}  // extern "C"
