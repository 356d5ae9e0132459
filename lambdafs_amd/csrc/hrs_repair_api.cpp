// Checked repair behind the C ABI, the device call (hrs_repair_checked_dev,
// include/hrs.h): stored checksums in, verdicts out. Everything between the
// first launch and the last is queued on the caller's stream: pass 1
// (run_scrub_crc as it is), the plan kernel, the listed heal, the listed CRC
// pass and the fold + verdict kernel (hrs_repair.hip). The host waits for
// nothing, copies nothing back and builds no table: the tables a launch needs
// from the host (the CRC images) are fetched before the first launch. The
// one-stripe CPU reference, hrs_repair_checked_host, is in hrs_scrub_api.cpp
// beside the host pieces it runs.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/hrs.h"
#include "hrs_codec.hpp"
#include "hrs_crc.hpp"
#include "hrs_heal_erased.hpp"
#include "hrs_internal.hpp"
#include "hrs_launch.hpp"
#include "hrs_repair.hpp"

namespace hrs::api {

namespace {

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// After the argument checks, on the codec's device.
hrs_status run_repair_checked(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                              const uint32_t* stored, int flags, uint32_t* verdicts, int32_t* erased_out,
                              uint32_t* reports, size_t report_stride, uint32_t* crc_out, hipStream_t s) {
  const int n = c->n;
  // host-built tables first: a miss uploads, which no launch of this call may wait behind
  hrs_status st = crc_window_tables(c);
  if (st != HRS_OK) return st;
  hrs_codec::FoldTables* ft = nullptr;
  st = crc_fold_tables(c, len, hrs::kCrcWindow, &ft);
  if (st != HRS_OK) return st;
  // One scratch for the whole call, taken before pass 1 so that pass 1's own
  // request finds it large enough and nothing is reallocated between the
  // passes: pass 1's raw window CRCs (reused for the listed stripes' once it
  // has folded them), then the list and the pattern table.
  const size_t raw_bytes = round_up(crc_raw_bytes_for(len, nstripes, n) + 8, 256);  // either path of pass 1 fits
  const size_t list_bytes = round_up((1 + nstripes) * sizeof(uint32_t), 256);
  const size_t pats_bytes = nstripes * sizeof(hrs::ErasePattern);
  return with_crc_scratch(c, raw_bytes + list_bytes + pats_bytes, s, [&]() -> hrs_status {
    hrs_status r = run_scrub_crc(c, rows, stride, len, nstripes, reports, report_stride, nullptr, crc_out, s, false);
    if (r != HRS_OK) return r;
    const std::string kernel = c->last_kernel;  // hrs_last_kernel names pass 1's kernel
    uint8_t* base = reinterpret_cast<uint8_t*>(c->crc_raw);
    uint32_t* list = reinterpret_cast<uint32_t*>(base + raw_bytes);
    hrs::ErasePattern* pats = reinterpret_cast<hrs::ErasePattern*>(base + raw_bytes + list_bytes);
    hipError_t e = hipMemsetAsync(list, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return hip_fail(c, e, "hipMemsetAsync");
    hrs::RepairPlanArgs pa{};
    pa.stored = stored;
    pa.crcs = crc_out;
    pa.reports = reports;
    pa.report_stride = report_stride;
    pa.verdicts = verdicts;
    pa.erased_out = erased_out;
    pa.list = list;
    pa.pats = pats;
    pa.nstripes = static_cast<uint32_t>(nstripes);
    pa.n = n;
    pa.p = c->p;
    pa.flags = flags;
    if ((e = hrs::launch_repair_plan(pa, s)) != hipSuccess) return hip_fail(c, e, "repair plan launch");
    // pass 2 over the listed stripes: the siblings' split into whole 2 KiB
    // windows and the byte-granular rest; the task counts are upper bounds
    hrs::HealListedArgs ha{};
    hrs::ScrubArgs& a = ha.h.s;
    bool vec_ok = stride % 16 == 0 && c->kernel_mode != 2, aligned = stride % 16 == 0;
    for (int l = 0; l < n; ++l) {
      a.rows[l] = rows[l];
      vec_ok &= aligned16(rows[l]);
      aligned &= aligned16(rows[l]);
    }
    a.stride = stride;
    a.len = len;
    a.reports = reports;
    a.report_stride = report_stride;
    a.n = n;
    a.p = c->p;
    ha.h.pats = pats;
    ha.h.pat = nullptr;
    ha.list = list;
    ha.nstripes = static_cast<uint32_t>(nstripes);
    a.nwin = vec_ok ? len / hrs::kWindowBytes : 0;
    if (a.nwin > 0) {
      a.ntasks = a.nwin * nstripes;
      if ((e = hrs::launch_heal_listed(ha, s)) != hipSuccess) return hip_fail(c, e, "listed heal launch");
    }
    a.col0 = a.nwin * hrs::kWindowBytes;
    if (a.col0 < len) {
      a.ntasks = (len - a.col0) * nstripes;
      if ((e = hrs::launch_heal_listed_bytewise(ha, s)) != hipSuccess) return hip_fail(c, e, "listed heal bytewise launch");
    }
    // the CRCs of the listed stripes' cells as pass 2 left them, then the verdicts
    const int cus = hrs::device_cu_count();
    hrs::RepairCrcArgs ca{};
    for (int l = 0; l < n; ++l) ca.rows[l] = rows[l];
    ca.stride = stride;
    ca.len = len;
    ca.list = list;
    ca.nstripes = static_cast<uint32_t>(nstripes);
    ca.n = n;
    ca.raw = c->crc_raw;
    ca.tables = c->crc_tables_a;
    if ((e = hrs::launch_repair_crc_windows(ca, aligned, cus, s)) != hipSuccess) return hip_fail(c, e, "listed crc launch");
    hrs::RepairFoldArgs fa{};
    fa.raw = c->crc_raw;
    fa.list = list;
    fa.stored = stored;
    fa.crc_out = crc_out;
    fa.reports = reports;
    fa.report_stride = report_stride;
    fa.verdicts = verdicts;
    fa.nwin = len / hrs::kCrcWindow;
    fa.tail = len % hrs::kCrcWindow;
    fa.nstripes = static_cast<uint32_t>(nstripes);
    fa.n = n;
    fa.G = static_cast<int>((fa.nwin + 63) / 64);
    fa.tables = ft->dev;
    if ((e = hrs::launch_repair_fold_verdict(fa, cus, s)) != hipSuccess) return hip_fail(c, e, "repair verdict launch");
    c->last_kernel = kernel;
    return fold_tables_used(c, ft, s);
  });
}

}  // namespace

}  // namespace hrs::api

using namespace hrs::api;

extern "C" {

hrs_status hrs_repair_checked_dev(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                                  const uint32_t* stored, int flags, uint32_t* verdicts, int32_t* erased_out,
                                  uint32_t* reports, size_t report_stride, uint32_t* crc_out, void* stream) {
  bool empty = false;
  const hrs_status st =
      repair_args_ok(c, rows, reports, report_stride, len, nstripes, true, stored, flags, verdicts, crc_out, &empty);
  if (st != HRS_OK || empty) return st;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  return run_repair_checked(c, rows, stride, len, nstripes, stored, flags, verdicts, erased_out, reports,
                            report_stride, crc_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
