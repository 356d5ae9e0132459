// Internal interface shared by libhrs's host translation units (hrs_api.cpp,
// hrs_matrix.cpp, hrs_dispatch.cpp, hrs_crc_api.cpp, hrs_hostpath.cpp,
// hrs_batch_api.cpp, hrs_hostbatch_api.cpp): the
// codec handle behind the C ABI's opaque hrs_codec, error reporting, and the
// functions one unit calls in another. Not part of the ABI (hidden symbols).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/hrs.h"
#include "crc32.hpp"
#include "hrs_heal_erased.hpp"
#include "hrs_internal.hpp"

namespace hrs {
class CopyPool;  // hrs_host.hpp
}

struct hrs_codec {
  int kind = HRS_CODE_RS;
  int k = 0;
  int p = 0;
  int n = 0;
  int device = 0;
  int kernel_mode = 0;
  std::vector<uint8_t> g;  // p x k
  // SimpleRegeneratingCode: s SRC parities (after init's adjustment), r RS
  // parities, group degree d, and each location's group neighbours
  int src_s = 0, src_r = 0, src_d = 0;
  std::vector<std::vector<int>> groups;
  hipStream_t stream = nullptr;
  std::map<std::vector<int>, std::vector<uint8_t>> decode_cache;
  // CRC-32 state (hrs_crc32_dev): fixed window tables, per-length fold tables, scratch
  uint32_t* crc_tables_a = nullptr;
  // fold tables per (row length, window), LRU: an entry is freed only once the
  // event recorded after its latest fold launch has completed
  struct FoldTables {
    uint32_t* dev = nullptr;
    // the latest fold that read the tables on each stream that has used them
    // (slot streams, caller streams): the tables may be freed once every one
    // of these events has completed
    struct Use {
      hipStream_t stream;
      hipEvent_t ev;
    };
    std::vector<Use> uses;
    uint64_t tick = 0;
  };
  std::map<uint64_t, FoldTables> crc_fold_tables;
  uint64_t crc_fold_tick = 0;
  uint32_t* crc_raw = nullptr;
  size_t crc_raw_bytes = 0;
  hipEvent_t crc_raw_done = nullptr;  // recorded after the latest use (crc_scratch)
  bool crc_raw_used = false;
  std::map<uint64_t, hrs::crc::Mat> crc_zmats;  // host-side Z_len, chaining chunk CRCs
  // hrs_decode_batch_dev: two slots (plans + per-stripe pattern index), each
  // a device buffer and its pinned staging; a slot is reused once the event
  // recorded after its launches has completed.
  struct BatchSlot {
    uint8_t* dev = nullptr;
    uint8_t* host = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
  } batch[2];
  int batch_next = 0;
  // host-buffer calls (hrs_hostpath.cpp): a staging slot is pinned staging,
  // device rows of the same size and its own stream, with the event recorded
  // after the work queued on it (stage_slot sizes one, free_stage_slot frees it)
  struct StageSlot {
    uint8_t* pin = nullptr;
    uint8_t* pin_dev = nullptr;  // device address of `pin` (zero-copy kernels)
    uint8_t* dev = nullptr;
    size_t bytes = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
  };
  // synchronous calls: the chunk slots (8 by default, HRS_HOST_SLOTS 2-8); a
  // slot is reused once its chunk's event has completed
  StageSlot host[hrs::kHostSlots];
  std::map<uint64_t, std::vector<uint32_t>> crc_ztabs;  // Z_n as 4 x 256 tables, by n (host folds)
  // host-memory batches (hrs_*_batch_host): a ring of chunk slots, each a
  // device image + output block, pinned staging (pageable callers only) and
  // its own compute stream; every slot's H2D goes on one copy-in stream and
  // every D2H on one copy-out stream, so the two directions of the link run
  // at once (the link is full duplex: profiles/r04/duplex/). Per slot:
  // in_done after its H2D, comp_done after its kernels, done after its D2H.
  struct HostBatchSlot {
    uint8_t* dev = nullptr;
    size_t dev_bytes = 0;
    uint8_t* pin = nullptr;
    uint8_t* pin_dev = nullptr;  // device address of `pin` (zero-copy kernels)
    size_t pin_bytes = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t in_done = nullptr;
    hipEvent_t comp_done = nullptr;
  } hbatch[hrs::kHostBatchSlots];
  // hrs_scrub_batch_host: the reports accumulate here (device) and come back
  // in one copy when the batch has run
  uint32_t* scrub_reports = nullptr;
  size_t scrub_reports_bytes = 0;
  // hrs_*_batch_host_crc: the CRCs accumulate here (device; filled from
  // crc_in first) and come back in one copy when the batch has run
  uint32_t* hbatch_crc = nullptr;
  size_t hbatch_crc_bytes = 0;
  hipStream_t hbatch_in = nullptr;   // H2D of every host-batch slot
  hipStream_t hbatch_out = nullptr;  // D2H of every host-batch slot
  // asynchronous host-buffer calls (hrs_*_submit / hrs_collect): a ring of
  // operation slots, each a staging slot plus the state of its ticket; an
  // operation occupies its slot from submit until it is collected
  struct AsyncSlot : StageSlot {
    hipEvent_t t_start = nullptr;  // timing events (hrs_set_timing)
    hipEvent_t t_end = nullptr;
    bool timed = false;   // this operation recorded t_start / t_end
    bool busy = false;
    bool queued = false;  // GPU work was queued (len > 0)
    uint64_t ticket = 0;
    int nout = 0, nlive = 0, ncrc = 0;
    size_t len = 0, pitch = 0, crc_off = 0;
  } async[hrs::kAsyncSlots];
  uint64_t async_tickets = 0;
  bool timing = false;  // hrs_set_timing: asynchronous operations record timing events
  std::string err;
  std::string last_kernel;  // main kernel of the latest coding call (hrs_last_kernel)
  const char* last_host_path = "";  // hrs_last_host_path: "pinned" | "staged" | "copy_engine"
  int numa_node = -2;               // NUMA node of the device's PCI function (-1 unknown, -2 not read yet)
};


#pragma GCC visibility push(hidden)
namespace hrs::api {

// ---- errors (hrs_api.cpp): record the message on the handle (or, for
// create errors, per thread) and return st
hrs_status fail(hrs_codec* c, hrs_status st, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
hrs_status hip_fail(hrs_codec* c, hipError_t e, const char* what);

// Keeps the caller's current device across a call on codec->device.
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (dev < 0) {  // host-only handle
      ok = false;
      return;
    }
    if (hipGetDevice(&prev) != hipSuccess) {
      ok = false;
      return;
    }
    if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- zero copy (hrs_hostbatch_api.cpp): kernels read and write pinned host
// memory across the host link directly instead of H2D -> kernel -> D2H — the
// link then carries both directions at once with no copy-engine calls
// (profiles/r04/NOTES.md). HRS_ZEROCOPY=0 turns it off (A/B runs; read per
// call); HRS_ZC_BLOCKS caps the grid of such launches (hrs::GridCap).
bool zero_copy_on();
unsigned zero_copy_blocks();
// Host memory the runtime allocated pinned (hipHostMalloc, torch
// pin_memory), [p, p + len) inside one allocation. Caller-registered
// (hipHostRegister) pageable memory is not: its pages can move.
bool runtime_pinned(const void* p, size_t len);
// Device address of runtime-pinned host memory [p, p + len) when it equals
// the host address, or false (pageable or registered memory: staged).
bool host_device_ptr(const void* p, size_t len, uint8_t** dp);
// The host copy pool (hrs_host.hpp), its workers placed for this handle's
// GPU: on the GPU's NUMA node, where its pinned staging lives, unless
// HRS_HOST_HOME=caller (hrs_hostpath.cpp).
hrs::CopyPool& copy_pool(hrs_codec* c);
// How copy-ins store into pinned staging (hrs::kStore*; HRS_HOST_NT).
uint8_t host_store_mode();
// Drains a staging slot's stream and frees everything the slot holds
// (hrs_hostpath.cpp; hrs_destroy).
void free_stage_slot(hrs_codec::StageSlot& h);

// The compile-time encode kernels hold the hops RS generator (rs) or the
// ISA-L Cauchy rows (nrs) of a (k, p) shape; only those families' G may take
// them. SRC's G (XOR groups over RS(k, r)) and XOR's all-ones row may not.
inline bool static_encode_family(const hrs_codec* c) { return c->kind == HRS_CODE_RS || c->kind == HRS_CODE_NRS; }

bool decode_locations_ok(const hrs_codec* c, const int* erased, int ne, const int* to_read, int nr, const int* ntr,
                         int nn);

// ---- matrices (hrs_matrix.cpp)
bool gf_invert(std::vector<uint8_t>& a, int m);
void rs_decode_rows(int n, const int* erased, int ne, const int* ntr, int nn, int zero_ntr, std::vector<uint8_t>& d);
hrs_status build_decode_matrix(hrs_codec* c, const int* erased, int ne, const int* ntr, int nn, int zero_ntr,
                               std::vector<uint8_t>& d);
hrs_status build_nrs_decode_matrix(hrs_codec* c, int ne, const int* ntr, int nn, std::vector<uint8_t>& d);
const std::vector<uint8_t>* cached_decode_matrix(hrs_codec* c, const int* erased, int ne, const int* ntr, int nn,
                                                 int zero_ntr, hrs_status* st);
std::vector<int> src_neighbors(const hrs_codec* c, int loc);
void src_params(int k, int p, int s_in, int* s, int* r, int* d);
hrs_status src_locations(hrs_codec* c, const int* erased, int ne, std::vector<int>& out);
hrs_status decode5_matrix(hrs_codec* c, const int* erased, int ne, const int* ntr, int nn,
                          const uint8_t* const* rows, std::vector<uint8_t>& tmp, const uint8_t** out,
                          const int* to_read = nullptr, int nr = -1);
void init_encode_matrix(hrs_codec* c);

// ---- device dispatch (hrs_dispatch.cpp)
hrs_status run_apply(hrs_codec* c, const uint8_t* m, int nout, int nin, const uint8_t* const* in_rows,
                     size_t in_stride, uint8_t* const* out_rows, size_t out_stride, size_t len, size_t nstripes,
                     hipStream_t s, bool static_kp);

// ---- ragged encode (hrs_dispatch.cpp; kernels: hrs_ragged.hip)
// Rule 4 of the ragged entry points (include/hrs.h): len <= UINT32_MAX and
// every one of the nstripes * k HOST words of `valid` <= len, the stripe and
// row named. *all_full: every word equals len.
hrs_status ragged_valid_ok(hrs_codec* c, const uint32_t* valid, size_t len, size_t nstripes, bool* all_full);
// Whether a ragged batch takes the plain encode: every cell full, and the
// kernel mode does not pin the ragged kernels (2, 3).
inline bool ragged_takes_plain(const hrs_codec* c, bool all_full) {
  return all_full && c->kernel_mode != 2 && c->kernel_mode != 3;
}
// encodeBulk over data cells that read as zero from dvalid[s * k + j] on
// (DEVICE words, at the range's first stripe): the vector kernel over the
// whole 2 KiB windows of aligned rows of a static shape, the byte-granular
// kernel over the rest. in_rows[k], out_rows[p]: none NULL. len, nstripes > 0.
hrs_status run_ragged(hrs_codec* c, const uint8_t* const* in_rows, size_t in_stride, uint8_t* const* out_rows,
                      size_t out_stride, size_t len, size_t nstripes, const uint32_t* dvalid, hipStream_t s);

// ---- CRC-32 (hrs_crc_api.cpp)
size_t crc_raw_bytes_for(size_t len, size_t nstripes, int nrows);
hrs_status run_crc(hrs_codec* c, const uint8_t* const* rows, const size_t* strides, int nrows, size_t len,
                   size_t nstripes, const uint32_t* crc_in, uint32_t* crc_out, hipStream_t s, uint32_t* raw);
// The handle's raw-CRC scratch (c->crc_raw, at least `bytes`) for a call on
// stream s, its uses chained by an event across streams; release records it.
// with_crc_scratch is the only caller of the two and the only way to
// c->crc_raw: it takes the scratch, runs `body` (hrs_status(); its launches go
// on s) and releases on s with body's status, whether or not body succeeded.
// A lease inside a lease (run_repair_checked around run_scrub_crc) asks for no
// more than the outer one, so nothing is reallocated under it. A template, so
// that the body is inlined into its caller.
hrs_status crc_scratch(hrs_codec* c, size_t bytes, hipStream_t s);
hrs_status crc_scratch_release(hrs_codec* c, hipStream_t s, hrs_status st);
template <class Body>
hrs_status with_crc_scratch(hrs_codec* c, size_t bytes, hipStream_t s, Body body) {
  const hrs_status st = crc_scratch(c, bytes, s);
  return st != HRS_OK ? st : crc_scratch_release(c, s, body());
}
// The CRC-32 of nrows rows of one stride after a pass that left them on
// stream s (the stream orders that pass's stores before the window pass
// reads them): a lease of crc_raw_bytes_for, then run_crc. The handle's last
// kernel stays the pass's. crc_out[s * nrows + r].
hrs_status crc_rows(hrs_codec* c, const uint8_t* const* rows, int nrows, size_t stride, size_t len, size_t nstripes,
                    const uint32_t* crc_in, uint32_t* crc_out, hipStream_t s);
hrs_status crc_window_tables(hrs_codec* c);  // c->crc_tables_a, uploaded once
// The fold tables (kCrcLdsWordsB words, device) for rows of `len` bytes cut in
// windows of `win` bytes, cached per handle; a caller with a fold kernel of its
// own fetches them before its first launch (a miss uploads them) and calls
// fold_tables_used after the launch that reads them.
hrs_status crc_fold_tables(hrs_codec* c, uint64_t len, uint64_t win, hrs_codec::FoldTables** out);
hrs_status fold_tables_used(hrs_codec* c, hrs_codec::FoldTables* ft, hipStream_t s);
// run_crc's window pass alone, raw rows laid out for a fold over nrows_total rows.
hrs_status crc_windows(hrs_codec* c, const uint8_t* const* rows, const size_t* strides, int nrows, int nrows_total,
                       size_t len, size_t nstripes, hipStream_t s, uint32_t* raw);
// The fold alone: raw window CRCs of nsr (stripe, row) pairs, windows of `win`
// bytes, into crc_out, continuing crc_in. mask: the fold of a repair batch
// (nsr = stripes * rows_per_stripe): output t of stripe s past the stripe's
// losses (t >= plans[pat[s]].nout; device tables) yields crc_in (0 when NULL)
// without reading raw. crc_out[s * rows_per_stripe + t].
struct BatchCrcMask {
  const hrs::BatchPlan* plans;
  const int32_t* pat;
  int rows_per_stripe;
};
hrs_status crc_fold(hrs_codec* c, size_t len, uint64_t nsr, const uint32_t* crc_in, uint32_t* crc_out, hipStream_t s,
                    uint32_t* raw, uint64_t win, const BatchCrcMask* mask = nullptr);
// host_fold_win != NULL: when the fused one-pass kernel runs, no fold is
// launched; the raw window CRCs stay in `raw` (layout [stripe][row][window])
// and *host_fold_win receives the window size for the caller's host fold
// (0: the two-pass path ran and wrote crc_out itself).
hrs_status encode_crc_impl(hrs_codec* c, const uint8_t* const* in_rows, size_t in_stride, uint8_t* const* out_rows,
                           size_t out_stride, size_t len, size_t nstripes, const uint32_t* crc_in, uint32_t* crc_out,
                           hipStream_t s, uint32_t* raw, uint64_t* host_fold_win = nullptr);
hrs_status apply_crc_impl(hrs_codec* c, const uint8_t* m, int nout, int nin, const uint8_t* const* in_rows,
                          size_t in_stride, uint8_t* const* out_rows, size_t out_stride, size_t len, size_t nstripes,
                          const uint32_t* crc_in, uint32_t* crc_out, hipStream_t s, uint32_t* raw,
                          uint64_t* host_fold_win = nullptr);
// Whether encode_crc_impl / apply_crc_impl (nlive live inputs) take their
// one-pass kernel for a job of this shape, rows 16-byte aligned: the
// zero-copy host calls checksum through host memory only then (a two-pass CRC
// would read the cells across the link a second time).
bool encode_crc_one_pass(const hrs_codec* c, size_t len, size_t nstripes);
bool apply_crc_one_pass(const hrs_codec* c, int nout, int nlive, size_t len);
// Whether a ragged batch with CRCs takes the plain encode + CRC: every cell
// full, in kernel modes 0 and 1 (2 keeps the byte-granular ragged route, 3 the
// ragged fused kernel).
inline bool ragged_crc_takes_plain(const hrs_codec* c, bool all_full) {
  return all_full && (c->kernel_mode == 0 || c->kernel_mode == 1);
}
// hrs_encode_ragged_crc_dev after its checks, the valid words on the device
// (dvalid, at the range's first stripe): the one-pass ragged kernel under
// encode_crc_impl's rule, else run_ragged, the ragged window pass and the
// fold. raw: crc_raw_bytes_for(len, nstripes, n) under the caller's lease.
hrs_status encode_ragged_crc_impl(hrs_codec* c, const uint8_t* const* in_rows, size_t in_stride,
                                  uint8_t* const* out_rows, size_t out_stride, size_t len, size_t nstripes,
                                  const uint32_t* dvalid, const uint32_t* crc_in, uint32_t* crc_out, hipStream_t s,
                                  uint32_t* raw);

// ---- stripe scrubbing (hrs_scrub_api.cpp)
// The code and report_stride checks of the scrub entry points (rs only,
// p <= 8, report_stride >= 4 + n when with_reports).
hrs_status scrub_code_ok(hrs_codec* c, size_t report_stride, bool with_reports);
// The argument rules every scrub / heal entry point shares, in this order: the
// handle (NULL: HRS_EINVAL, no message), scrub_code_ok, `cells` and `reports`
// not NULL, the n row pointers `cells` holds, the erased list when
// `erased_what` names its count ("max_erased %d with no erased list"), then
// nstripes < 2^31 and len < 2^32. The empty batch and the device are the
// caller's.
enum : unsigned {
  kScrubWithReports = 1u,  // one report per stripe: report_stride is checked ("reports"; else one "report")
  kScrubRowsWritten = 2u,  // the rows are written: heal_rows_ok instead of the NULL check of each row
  kScrubImage = 4u,        // `cells` is one batch image ("stripes") with no row pointers to check
};
hrs_status scrub_args_ok(hrs_codec* c, const void* cells, const uint32_t* reports, size_t report_stride, size_t len,
                         size_t nstripes, unsigned flags, const char* erased_what = nullptr, int erased_count = 0,
                         const int* erased = nullptr);
// Empty reports, then the vector kernel over the whole 2 KiB windows and the
// byte-granular kernel over the rest, all on stream s. rows[n]: none NULL.
// heal: the kernels' heal variants, which also write the resolved columns
// back through rows[] (writable, no two equal) and count the bytes in word 3.
hrs_status run_scrub(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                     uint32_t* reports, size_t report_stride, hipStream_t s, bool heal);
// The rows of a heal call: none NULL, no two equal (HRS_EINVAL).
hrs_status heal_rows_ok(hrs_codec* c, const uint8_t* const* rows);
// run_scrub plus the CRC-32 of every cell (hrs_scrub_crc_dev's semantics:
// crc_out[s * n + l], hops order, DEVICE arrays; the heal's cover the cells
// after the write-back). One pass (hrs_scrub_crc.hip) when
// scrub_crc_one_pass holds, else run_scrub, then the CRC pass over the n
// rows. Takes and releases the handle's raw-CRC scratch on stream s.
hrs_status run_scrub_crc(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                         uint32_t* reports, size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out,
                         hipStream_t s, bool heal);
// 2 <= p <= 4, n <= 16, whole 2 KiB windows, 16-byte aligned rows and stride,
// kernel mode 0 or 3.
bool scrub_crc_one_pass(const hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len);

// ---- ragged scrub and heal (hrs_scrub_api.cpp; kernels: hrs_scrub_ragged.hip)
// The cells of a host batch must not overlap (hrs_scrub_batch_host's rule,
// include/hrs.h): HRS_EINVAL with the strides named. len, nstripes > 0.
hrs_status scrub_cells_apart_ok(hrs_codec* c, size_t row_stride, size_t stripe_stride, size_t len, size_t nstripes);
// The argument rules of the ragged scrub / heal entry points (include/hrs.h),
// before the device is selected: scrub_args_ok with `flags`, for a batch image
// (kScrubImage) with bytes in it scrub_cells_apart_ok, valid not NULL, the
// empty batch (*empty = true: return HRS_OK and touch nothing), every one of
// the nstripes * n HOST words of `valid` <= len (the stripe and location
// named). *all_full: every word equals len.
hrs_status scrub_ragged_args_ok(hrs_codec* c, const void* cells, const uint32_t* reports, size_t report_stride,
                                size_t len, size_t nstripes, unsigned flags, size_t row_stride, size_t stripe_stride,
                                const uint32_t* valid, bool* empty, bool* all_full);
// Whether a ragged scrub / heal batch takes the plain route: every cell full,
// in kernel modes 0 and 1 (2 and 3 keep the ragged kernels).
inline bool scrub_ragged_takes_plain(const hrs_codec* c, bool all_full) {
  return all_full && (c->kernel_mode == 0 || c->kernel_mode == 1);
}
// The device length table of a ragged scrub / heal (hrs_scrub_ragged.hpp:
// n + 1 words per stripe) from valid[nstripes * n], through a batch slot and up
// to the device on s. The caller calls slot_used after its launches.
hrs_status scrub_ragged_table(hrs_codec* c, const uint32_t* valid, size_t nstripes, hipStream_t s,
                              hrs_codec::BatchSlot** slot, const uint32_t** dlens);
// run_scrub over cells that read as zero from their length on: dlens is the
// device table at the range's first stripe. The ragged window kernel over the
// whole 2 KiB windows of aligned rows, the byte-granular ragged kernel over the
// rest (everything in kernel mode 2).
hrs_status run_scrub_ragged(hrs_codec* c, const uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                            const uint32_t* dlens, uint32_t* reports, size_t report_stride, hipStream_t s, bool heal);

// ---- heal with known erasures (hrs_scrub_api.cpp)
// The erased set of one stripe: entries up to the first negative one (or
// `cap`), sorted ascending into `key`. HRS_EINVAL for a location outside
// [0, n) or a repeated one, HRS_ETOOMANY for more than p, the stripe named.
hrs_status erased_key(hrs_codec* c, const int* erased, int cap, size_t stripe, std::vector<int>& key);
// The device table entry of an erased set (hrs_heal_erased.hpp).
hrs::ErasePattern make_pattern(int p, const std::vector<int>& key);
// The erased sets of a batch, validated and de-duplicated: the table entries,
// each entry's locations (ascending) and every stripe's entry. max_erased <= 0
// leaves all three empty.
struct ErasedSets {
  std::vector<hrs::ErasePattern> pats;
  std::vector<std::vector<int>> keys;
  std::vector<int32_t> pat;
};
hrs_status erased_sets(hrs_codec* c, const int* erased, int max_erased, size_t nstripes, ErasedSets& es);
// hrs_heal_erased_dev after its checks: uploads the table and pat[nstripes]
// through a batch slot on s, then the window and tail kernels.
hrs_status run_heal_erased(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                           const std::vector<hrs::ErasePattern>& pats, const int32_t* pat, uint32_t* reports,
                           size_t report_stride, hipStream_t s);
// run_heal_erased plus the CRC-32 of every cell as the call leaves it
// (crc_out[s * n + l], hops order, DEVICE arrays). One pass
// (hrs_heal_erased_crc.hip) for the shapes of scrub_crc_one_pass in kernel
// mode 3, and in mode 0 where heal_erased_crc_fused_default says so for the
// memory the rows lie in; else run_heal_erased, then the CRC pass over the n
// rows. Takes and releases the handle's raw-CRC scratch on stream s.
hrs_status run_heal_erased_crc(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                               const std::vector<hrs::ErasePattern>& pats, const int32_t* pat, uint32_t* reports,
                               size_t report_stride, const uint32_t* crc_in, uint32_t* crc_out, hipStream_t s,
                               bool host_memory);
bool heal_erased_crc_fused_default(bool host_memory);

// ---- checked repair (hrs_scrub_api.cpp, hrs_repair_api.cpp)
// The argument rules of hrs_repair_checked_dev (with_reports) and
// hrs_repair_checked_host, in the family's order: scrub_args_ok for a call
// that writes the rows, the flag bits, then the empty call (*empty = true:
// return HRS_OK and touch nothing), then stored, verdicts and crc_out not NULL
// and stored apart from crc_out. The device is the caller's.
hrs_status repair_args_ok(hrs_codec* c, const uint8_t* const* rows, const uint32_t* reports, size_t report_stride,
                          size_t len, size_t nstripes, bool with_reports, const uint32_t* stored, int flags,
                          const uint32_t* verdicts, const uint32_t* crc_out, bool* empty);

// ---- per-call device tables (hrs_batch_api.cpp)
// Two byte ranges, a table and the per-stripe indices into it, through the
// next of the handle's two batch slots (pinned staging + device buffer, waited
// idle) and up to the device on s: the table at (*slot)->dev, the indices
// a_bytes after it. After its launches the caller calls slot_used, on every
// exit: the slot's table may be in use whether or not every launch went out.
hrs_status upload(hrs_codec* c, const void* a, size_t a_bytes, const void* b, size_t b_bytes, hipStream_t s,
                  hrs_codec::BatchSlot** slot);
void slot_used(hrs_codec::BatchSlot* sl, hipStream_t s);

// ---- repair batches (hrs_batch_api.cpp)
// The plans of a heterogeneous repair batch: one per distinct erasure
// pattern (its live survivor locations and packed coefficients), the pattern
// index of every stripe, and each pattern's full ne x n matrix (for the
// per-stripe fallback when a pattern exceeds the batch kernel's shape).
struct BatchPlanSet {
  std::vector<hrs::BatchPlan> plans;
  std::vector<int32_t> pat;
  std::vector<std::vector<uint8_t>> mats;
  bool fused = true;  // every pattern fits one batch_bitsliced launch
  int max_nout = 0, max_nin = 0;
  // ragged batches only (plan_order_lengths): every stripe's cell lengths in
  // the order of its plan, len_words = max_nin + max_nout words per stripe
  // (hrs_batch_ragged.hpp); empty for a plain batch
  std::vector<uint32_t> lens;
  int len_words = 0;
  // the device copies (upload_plans; pat and lens indexed by the absolute stripe number) and their slot
  const hrs::BatchPlan* dplans = nullptr;
  const int32_t* dpat = nullptr;
  const uint32_t* dlens = nullptr;
  hrs_codec::BatchSlot* slot = nullptr;
};
hrs_status build_batch_plans(hrs_codec* c, const int* erased, int max_erased, size_t nstripes, BatchPlanSet& ps);
// The plans and pattern indices, and ps.lens behind them when it is not empty,
// in one slot upload.
hrs_status upload_plans(hrs_codec* c, BatchPlanSet& ps, hipStream_t s);
// Where a batch lies: stripe i's row l at stripes + i * stripe_stride +
// l * row_stride, its output t at out + i * out_stripe_stride + t * out_row_stride.
struct BatchGeom {
  const uint8_t* stripes;
  size_t row_stride, stripe_stride;
  uint8_t* out;
  size_t out_row_stride, out_stripe_stride;
  size_t len;
};
// The CRC-32s of a repair batch (DEVICE arrays at the range's first stripe):
// out[i * max_erased + t] continues in[...] (NULL = fresh) over output t of
// stripe i, and over no bytes for t past the stripe's losses.
struct BatchCrcs {
  int max_erased;
  const uint32_t* in;
  uint32_t* out;
};
// Repairs stripes [s0, s0 + ns) of a batch on stream s; g points at stripe s0.
// crc != NULL: with their CRCs, through the handle's raw-CRC scratch (taken and
// released on s); the plans must have been uploaded. Without CRCs they must
// have been when ps.fused (else: one run_apply per stripe).
// ragged (ps.fused, ps.lens uploaded): the ragged kernels
// (hrs_batch_ragged.hip; with CRCs hrs_batch_ragged_crc.hip, each CRC over
// exactly its cell's length) with the stripes' slice of the length table.
hrs_status run_batch(hrs_codec* c, const BatchPlanSet& ps, const BatchGeom& g, size_t s0, size_t ns,
                     const BatchCrcs* crc, hipStream_t s, bool ragged = false);
// The argument rules of the decode-batch entry points, in this order: the
// handle (NULL: HRS_EINVAL, no message), the argument block, the empty batch
// (*empty = true: return HRS_OK and touch nothing), nstripes < 2^31 unless
// kBatchDeviceSet (the members check their ranges), then with kBatchWithCrc
// crc_args_ok over nstripes * max_erased words. The device is the caller's.
enum : unsigned { kBatchWithCrc = 1u, kBatchDeviceSet = 2u };
hrs_status decode_batch_args_ok(hrs_codec* c, const BatchGeom& g, const int* erased, int max_erased, size_t nstripes,
                                unsigned flags, const uint32_t* crc_in, const uint32_t* crc_out, bool* empty);

// ---- ragged repair batches (hrs_batch_api.cpp; kernels: hrs_batch_ragged.hip)
// Rules 1-7 of hrs_decode_batch_ragged_dev / _host (include/hrs.h), before the
// device is selected: the handle, decode_batch_args_ok, valid not NULL, the
// empty batch (*empty = true: return HRS_OK and touch nothing), len <=
// UINT32_MAX and every one of the nstripes * n HOST words of `valid` <= len
// (the stripe and location named), the plans, and no pattern beyond the batch
// kernels' kBatchMaxIn survivors. *all_full: every word equals len. The CRC
// forms pass kBatchWithCrc and their arrays on to decode_batch_args_ok, whose
// crc_args_ok then stands between the argument block and `valid`.
hrs_status ragged_batch_args_ok(hrs_codec* c, const BatchGeom& g, const int* erased, int max_erased, size_t nstripes,
                                const uint32_t* valid, BatchPlanSet& ps, bool* empty, bool* all_full,
                                unsigned flags = 0u, const uint32_t* crc_in = nullptr,
                                const uint32_t* crc_out = nullptr);
// Whether a ragged repair batch takes the plain batch's route: every cell
// full, in kernel modes 0 and 1 (2 and 3 keep the ragged kernels).
inline bool ragged_batch_takes_plain(const hrs_codec* c, bool all_full) {
  return all_full && (c->kernel_mode == 0 || c->kernel_mode == 1);
}
// Fills ps.lens / ps.len_words from valid[s * n + l] (hops order): per stripe
// the lengths of its plan's inputs in plan order, then of its outputs; the
// words a stripe's plan does not use are 0.
void plan_order_lengths(const hrs_codec* c, const int* erased, int max_erased, size_t nstripes, const uint32_t* valid,
                        BatchPlanSet& ps);

// ---- shared by the CRC entry points
// crc_out may be crc_in itself; any other overlap of the two n-word arrays is refused (hrs_batch_api.cpp).
bool crc_arrays_apart(const uint32_t* crc_in, const uint32_t* crc_out, size_t n);
// crc_out not NULL and crc_arrays_apart, or HRS_EINVAL (hrs_batch_api.cpp).
hrs_status crc_args_ok(hrs_codec* c, const uint32_t* crc_in, const uint32_t* crc_out, size_t n);

}  // namespace hrs::api
#pragma GCC visibility pop
