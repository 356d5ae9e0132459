// Batches: heterogeneous repair batches on the device (one erasure pattern
// per stripe, plans uploaded through pinned slots, one batch launch) and the
// host-memory batch pipelines (hrs_decode_batch_host / hrs_encode_batch_host:
// chunks of stripes through a ring of device slots, H2D of exactly the rows
// read, D2H of exactly the rows written), each with its block-CRC-32 form
// (hrs_decode_batch_crc_dev, hrs_decode_batch_host_crc, hrs_encode_batch_host_crc).
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/hrs.h"
#include "hrs_codec.hpp"
#include "hrs_crc.hpp"
#include "hrs_host.hpp"
#include "hrs_internal.hpp"
#include "hrs_launch.hpp"

namespace hrs::api {

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
};

hrs_status build_batch_plans(hrs_codec* c, const int* erased, int max_erased, size_t nstripes, BatchPlanSet& ps) {
  std::map<std::vector<int>, int> ids;
  ps.pat.assign(nstripes, 0);
  std::vector<int> key, to_read(c->n), ntr;
  for (size_t s = 0; s < nstripes; ++s) {
    key.clear();
    for (int t = 0; t < max_erased && erased[s * max_erased + t] >= 0; ++t) key.push_back(erased[s * max_erased + t]);
    auto it = ids.find(key);
    if (it != ids.end()) {
      ps.pat[s] = it->second;
      continue;
    }
    const int ne = static_cast<int>(key.size());
    for (int e : key)
      if (e >= c->n) return fail(c, HRS_EINVAL, "stripe %zu: erased location %d out of range", s, e);
    hrs::BatchPlan pl{};
    std::vector<uint8_t> m(static_cast<size_t>(ne) * c->n, 0);
    if (ne > 0) {
      int nr = 0;
      hrs_status st = hrs_locations_to_read_list(c, key.data(), ne, to_read.data(), &nr);
      if (st != HRS_OK) return st;
      ntr.clear();  // Decoder.java:303-338: everything not read, erased included
      for (int l = 0; l < c->n; ++l)
        if (std::find(to_read.begin(), to_read.begin() + nr, l) == to_read.begin() + nr ||
            std::find(key.begin(), key.end(), l) != key.end())
          ntr.push_back(l);
      std::vector<int> tr_sorted(to_read.begin(), to_read.begin() + nr);
      std::sort(tr_sorted.begin(), tr_sorted.end());
      std::vector<uint8_t> tmp;
      const uint8_t* d = nullptr;
      st = decode5_matrix(c, key.data(), ne, ntr.data(), static_cast<int>(ntr.size()), nullptr, tmp, &d,
                          tr_sorted.data(), nr);
      if (st != HRS_OK) return st;
      std::memcpy(m.data(), d, m.size());
      for (int l = 0; l < c->n; ++l) {  // live inputs, ascending location
        bool live = false;
        for (int o = 0; o < ne; ++o) live |= m[static_cast<size_t>(o) * c->n + l] != 0;
        if (!live) continue;
        if (pl.nin < hrs::kBatchMaxIn) {
          pl.loc[pl.nin] = l;
          for (int o = 0; o < ne; ++o)
            pl.cw[pl.nin] |= static_cast<uint64_t>(m[static_cast<size_t>(o) * c->n + l]) << (8 * o);
        }
        ++pl.nin;
      }
    }
    pl.nout = ne;
    if (pl.nin > hrs::kBatchMaxIn) ps.fused = false;
    ps.max_nout = std::max(ps.max_nout, ne);
    ps.max_nin = std::max(ps.max_nin, pl.nin);
    const int id = static_cast<int>(ps.plans.size());
    ids.emplace(key, id);
    ps.plans.push_back(pl);
    ps.mats.push_back(std::move(m));
    ps.pat[s] = id;
  }
  // one launch covers every pattern at (max_nout, max_nin); shapes beyond the
  // register-resident batch kernel take its streaming form (hrs_batch.hip)
  return HRS_OK;
}

// Repairs stripes [s0, s0 + ns) of a batch whose plans live at dplans / dpat
// (device; dpat indexed by the absolute stripe number) on stream hs. `stripes`
// and `out` point at stripe s0. ps.fused == false: one run_apply per stripe.
hrs_status launch_batch(hrs_codec* c, const BatchPlanSet& ps, const hrs::BatchPlan* dplans, const int32_t* dpat,
                        const uint8_t* stripes, size_t row_stride, size_t stripe_stride, uint8_t* out,
                        size_t out_row_stride, size_t out_stripe_stride, size_t len, size_t s0, size_t ns,
                        hipStream_t hs) {
  if (!ps.fused) {
    std::vector<const uint8_t*> rows(c->n);
    std::vector<uint8_t*> outs(hrs::kMaxOut);
    for (size_t i = 0; i < ns; ++i) {
      const int id = ps.pat[s0 + i];
      const hrs::BatchPlan& pl = ps.plans[id];
      if (pl.nout == 0) continue;
      for (int l = 0; l < c->n; ++l) rows[l] = stripes + i * stripe_stride + l * row_stride;
      for (int o = 0; o < pl.nout; ++o) outs[o] = out + i * out_stripe_stride + o * out_row_stride;
      hrs_status st = run_apply(c, ps.mats[id].data(), pl.nout, c->n, rows.data(), 0, outs.data(), 0, len, 1, hs, false);
      if (st != HRS_OK) return st;
    }
    return HRS_OK;
  }
  hrs::BatchArgs a{};
  a.base = stripes;
  a.out = out;
  a.row_stride = row_stride;
  a.stripe_stride = stripe_stride;
  a.out_row_stride = out_row_stride;
  a.out_stripe_stride = out_stripe_stride;
  a.len = len;
  a.plans = dplans;
  a.pat = dpat + s0;
  const bool vec = c->kernel_mode != 2 && aligned16(stripes) && aligned16(out) && row_stride % 16 == 0 &&
                   stripe_stride % 16 == 0 && out_row_stride % 16 == 0 && out_stripe_stride % 16 == 0;
  a.nwin = vec ? len / hrs::kWindowBytes : 0;
  if (a.nwin > 0) {
    a.ntasks = a.nwin * ns;
    hipError_t e = hrs::launch_batch_bitsliced(a, ps.max_nout, ps.max_nin, hs);
    if (e != hipSuccess) return hip_fail(c, e, "batch launch");
    c->last_kernel = hrs::last_kernel();
  }
  a.col0 = a.nwin * hrs::kWindowBytes;
  if (a.col0 < len) {
    a.ntasks = (len - a.col0) * ns;
    hipError_t e = hrs::launch_batch_bytewise(a, hs);
    if (e != hipSuccess) return hip_fail(c, e, "batch bytewise launch");
    if (a.nwin == 0) c->last_kernel = hrs::last_kernel();  // the call's only kernel
  }
  return HRS_OK;
}

// launch_batch + the CRC-32 of every repaired cell of stripes [s0, s0 + ns):
// crc_out[i * max_erased + t] (device; i counts from s0) continues
// crc_in[...] (NULL = fresh) over output t of stripe s0 + i, and over no bytes
// for t past the stripe's losses. dplans / dpat are always uploaded (the fold
// reads every stripe's loss count from them, the per-stripe fallback's too).
// raw: crc_raw_bytes_for(len, ns, max_erased) bytes of scratch.
// One pass (batch_decode_crc_kernel) for aligned whole-window batches of the
// one-pattern fused kernel's shapes; else launch_batch, the CRC window pass
// over the outputs (rows past a stripe's losses lie inside `out` and are read;
// the fold discards them) and the same fold.
hrs_status launch_batch_crc(hrs_codec* c, const BatchPlanSet& ps, const hrs::BatchPlan* dplans, const int32_t* dpat,
                            const uint8_t* stripes, size_t row_stride, size_t stripe_stride, uint8_t* out,
                            size_t out_row_stride, size_t out_stripe_stride, size_t len, size_t s0, size_t ns,
                            int max_erased, const uint32_t* crc_in, uint32_t* crc_out, hipStream_t hs, uint32_t* raw) {
  const BatchCrcMask mask{dplans, dpat + s0, max_erased};
  if (ps.max_nout == 0)  // nothing lost anywhere: every CRC continues over no bytes
    return batch_crc_fold(c, len, ns, mask, crc_in, crc_out, hs, raw, hrs::kCrcWindow);
  const bool one_pass = ps.fused && (c->kernel_mode == 0 || c->kernel_mode == 3) && len % hrs::kWindowBytes == 0 &&
                        aligned16(stripes) && aligned16(out) && row_stride % 16 == 0 && stripe_stride % 16 == 0 &&
                        out_row_stride % 16 == 0 && out_stripe_stride % 16 == 0 && ps.max_nout <= 4 &&
                        ps.max_nin <= (ps.max_nout == 4 ? 8 : 12);
  if (one_pass) {
    hrs_status st = crc_window_tables(c);
    if (st != HRS_OK) return st;
    hrs::BatchCrcArgs d{};
    d.b.base = stripes;
    d.b.out = out;
    d.b.row_stride = row_stride;
    d.b.stripe_stride = stripe_stride;
    d.b.out_row_stride = out_row_stride;
    d.b.out_stripe_stride = out_stripe_stride;
    d.b.len = len;
    d.b.nwin = len / hrs::kWindowBytes;
    d.b.ntasks = d.b.nwin * ns;
    d.b.plans = dplans;
    d.b.pat = dpat + s0;
    d.raw = raw;
    d.tables = c->crc_tables_a;
    d.rows_per_stripe = max_erased;
    hipError_t e = hrs::launch_batch_decode_crc(d, ps.max_nout, ps.max_nin, hrs::device_cu_count(), hs);
    if (e != hipSuccess) return hip_fail(c, e, "batch decode+crc launch");
    c->last_kernel = hrs::last_kernel();
    return batch_crc_fold(c, len, ns, mask, crc_in, crc_out, hs, raw, hrs::kWindowBytes);
  }
  hrs_status st = launch_batch(c, ps, dplans, dpat, stripes, row_stride, stripe_stride, out, out_row_stride,
                               out_stripe_stride, len, s0, ns, hs);
  if (st != HRS_OK) return st;
  const uint8_t* rows[hrs::kMaxOut];
  size_t strides[hrs::kMaxOut];
  for (int t = 0; t < ps.max_nout; ++t) {
    rows[t] = out + static_cast<size_t>(t) * out_row_stride;
    strides[t] = out_stripe_stride;
  }
  st = crc_windows(c, rows, strides, ps.max_nout, max_erased, len, ns, hs, raw);
  if (st != HRS_OK) return st;
  return batch_crc_fold(c, len, ns, mask, crc_in, crc_out, hs, raw, hrs::kCrcWindow);
}

// crc_out may be crc_in itself; any other overlap of the two n-word arrays is refused.
bool crc_arrays_apart(const uint32_t* crc_in, const uint32_t* crc_out, size_t n) {
  if (!crc_in || crc_in == crc_out) return true;
  const uintptr_t a = reinterpret_cast<uintptr_t>(crc_in), b = reinterpret_cast<uintptr_t>(crc_out);
  return a + n * 4 <= b || b + n * 4 <= a;
}

// The device CRC buffer of a host batch (n words), filled from crc_in (host).
hrs_status hbatch_crc_buffer(hrs_codec* c, size_t n, const uint32_t* crc_in) {
  const size_t bytes = n * sizeof(uint32_t);
  if (c->hbatch_crc_bytes < bytes) {  // every earlier batch has completed: the calls are synchronous
    if (c->hbatch_crc) (void)hipFree(c->hbatch_crc);
    c->hbatch_crc = nullptr;
    c->hbatch_crc_bytes = 0;
    const hipError_t e = hipMalloc(&c->hbatch_crc, bytes);
    if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    c->hbatch_crc_bytes = bytes;
  }
  if (crc_in) {
    const hipError_t e = hipMemcpy(c->hbatch_crc, crc_in, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(c, e, "hipMemcpy crc_in");
  }
  return HRS_OK;
}

hrs_status hbatch_crc_fetch(hrs_codec* c, size_t n, uint32_t* crc_out) {
  const hipError_t e = hipMemcpy(crc_out, c->hbatch_crc, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
  return e == hipSuccess ? HRS_OK : hip_fail(c, e, "hipMemcpy crc_out");
}

// Uploads plans + pattern indices through the next of the handle's two
// batch slots (pinned staging + device buffer; a slot is reused once the
// event recorded after its last launch has completed). Returns the device
// copies in *dplans / *dpat; the caller records sl.done after its launches.
hrs_status upload_batch_plans(hrs_codec* c, const BatchPlanSet& ps, hipStream_t hs, hrs_codec::BatchSlot** slot,
                              const hrs::BatchPlan** dplans, const int32_t** dpat) {
  const size_t plan_bytes = ps.plans.size() * sizeof(hrs::BatchPlan);
  const size_t need = plan_bytes + ps.pat.size() * sizeof(int32_t);
  hrs_status st = batch_slot_acquire(c, need, slot);
  if (st != HRS_OK) return st;
  hrs_codec::BatchSlot& sl = **slot;
  std::memcpy(sl.host, ps.plans.data(), plan_bytes);
  std::memcpy(sl.host + plan_bytes, ps.pat.data(), ps.pat.size() * sizeof(int32_t));
  hipError_t e = hipMemcpyAsync(sl.dev, sl.host, need, hipMemcpyHostToDevice, hs);
  if (e != hipSuccess) return hip_fail(c, e, "hipMemcpyAsync plans");
  *dplans = reinterpret_cast<const hrs::BatchPlan*>(sl.dev);
  *dpat = reinterpret_cast<const int32_t*>(sl.dev + plan_bytes);
  return HRS_OK;
}

// The next batch slot, idle and at least `need` bytes on both sides.
hrs_status batch_slot_acquire(hrs_codec* c, size_t need, hrs_codec::BatchSlot** slot) {
  hrs_codec::BatchSlot& sl = c->batch[c->batch_next];
  c->batch_next ^= 1;
  if (sl.pending) {
    hipError_t e = hipEventSynchronize(sl.done);
    if (e != hipSuccess) return hip_fail(c, e, "hipEventSynchronize");
    sl.pending = false;
  }
  if (!sl.done) {
    hipError_t e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
    if (e != hipSuccess) return hip_fail(c, e, "hipEventCreate");
  }
  if (sl.bytes < need) {
    if (sl.dev) (void)hipFree(sl.dev);
    if (sl.host) (void)hipHostFree(sl.host);
    sl.dev = nullptr;
    sl.host = nullptr;
    sl.bytes = 0;
    const size_t bytes = std::max<size_t>(need, 64 << 10);
    hipError_t e = hipMalloc(&sl.dev, bytes);
    if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    e = hipHostMalloc(&sl.host, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
    sl.bytes = bytes;
  }
  *slot = &sl;
  return HRS_OK;
}

// ------------------------------------------------ host-memory batches
// (hrs_decode_batch_host / hrs_encode_batch_host). Stripes start and end in
// host memory (DataNode sockets, local block files). Chunks of stripes flow
// through a ring of device slots: H2D of exactly the rows the chunk's codes
// read (on the copy-in stream) -> kernel (on the slot's stream) -> D2H of
// exactly the rows they write (on the copy-out stream), chained by events,
// so one chunk's D2H overlaps the next chunks' H2D on the full-duplex link.
// Pinned caller buffers are DMA'd directly and the whole job is queued before
// the host waits once; pageable ones go through each slot's pinned staging
// (copy pool), the host then waits for a slot before refilling it.

// Host memory the runtime allocated pinned, [p, p + len) inside one
// allocation: hipHostMalloc'd (torch pin_memory included) is an HSA pool
// allocation whose pages the driver holds for the allocation's lifetime.
// The GPU reads and writes only such memory in place (zero copy, or DMA by
// the copy engines). Pageable memory the caller registered with
// hipHostRegister reports HSA_EXT_POINTER_TYPE_LOCKED: the registration maps
// its pages for the GPU without pinning them, and a page that moves while a
// kernel writes it loses the writes into the freed old page (round 5: 5 of 11
// long fuzz runs; DESIGN.md §7 "Platform constraint"). It is staged like any
// pageable memory. So is device memory (HSA type too, but not host memory).
bool runtime_pinned(const void* p, size_t len) {
  if (!p) return false;
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory is reported as an error: clear it
    return false;
  }
  if (attr.type != hipMemoryTypeHost) return false;
  hsa_amd_pointer_info_t info{};
  info.size = sizeof info;
  if (hsa_amd_pointer_info(p, &info, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS) return false;
  if (info.type != HSA_EXT_POINTER_TYPE_HSA || !info.hostBaseAddress) return false;
  const uintptr_t b = reinterpret_cast<uintptr_t>(info.hostBaseAddress), a = reinterpret_cast<uintptr_t>(p);
  return a >= b && len <= info.sizeInBytes && a - b <= info.sizeInBytes - len;
}

// Whether a kernel reaches p across the host link (the caller's pinned
// stripes or a slot's zero-copy staging) and not in a device image.
bool on_host(const void* p) {
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

bool zero_copy_on() {
  const char* e = getenv("HRS_ZEROCOPY");
  return !(e && e[0] == '0');
}

// 64 blocks (256 waves) keep the host link as busy as a full grid does:
// config 5's repair 28.99 ms at 64 vs 29.66 uncapped, its encode 28.55 vs
// 29.57 (tools/bench_hbatch.py, profiles/r04/d/) — and leave 3/4 of the chip
// free for other work. HRS_ZC_BLOCKS=0 lifts the cap.
unsigned zero_copy_blocks() {
  const char* e = getenv("HRS_ZC_BLOCKS");
  const long x = e ? atol(e) : 64;
  return x > 0 ? static_cast<unsigned>(x) : 0u;
}

// Zero copy is taken only where the device address IS the host address
// (HIP's unified addressing on these systems): then any pointer into a pinned
// allocation, base or interior, is valid in a kernel as it stands, with no
// question of how an interior pointer's offset maps. Anything else (pageable
// or caller-registered memory, another mapping) is staged.
bool host_device_ptr(const void* p, size_t len, uint8_t** dp) {
  if (!p || !runtime_pinned(p, len)) return false;
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess || !d) {
    (void)hipGetLastError();
    return false;
  }
  if (d != p) return false;
  *dp = static_cast<uint8_t*>(d);
  return true;
}

// Bytes a strided batch spans from its base: the last stripe's last row end.
size_t batch_span(size_t nstripes, size_t stripe_stride, int rows, size_t row_stride, size_t len) {
  return (nstripes - 1) * stripe_stride + static_cast<size_t>(rows - 1) * row_stride + len;
}

size_t hbatch_target_bytes() {  // read per call (A/B runs in one process)
  const char* e = getenv("HRS_HBATCH_BYTES");
  const long x = e ? atol(e) : 0;
  return static_cast<size_t>(x > 0 ? x : 48l << 20);  // device image per chunk
}

// A staged batch's copy-out of a finished slot goes to the copy pool in one
// batch with the slot's next copy-in (HRS_HBATCH_MERGE=0: two batches, the
// round-5 form; read per call, A/B runs).
bool hbatch_merge() {
  const char* e = getenv("HRS_HBATCH_MERGE");
  return !(e && e[0] == '0');
}

// H2D and D2H on their own streams (one per direction, shared by the slots),
// or on each slot's stream behind and ahead of its kernels (HRS_HBATCH_DUPLEX=0:
// the round-3 pipeline, kept for A/B runs; read per call so one process can
// interleave both: tools/bench_hbatch.py).
bool hbatch_duplex() {
  const char* e = getenv("HRS_HBATCH_DUPLEX");
  return e && e[0] == '1';
}

hrs_status hbatch_slot(hrs_codec* c, int i, size_t dev_bytes, size_t pin_bytes) {
  hrs_codec::HostBatchSlot& h = c->hbatch[i];
  if (!h.stream) {
    hipError_t e = hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail(c, e, "hipStreamCreate");
    for (hipEvent_t* ev : {&h.done, &h.in_done, &h.comp_done}) {
      e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
      if (e != hipSuccess) return hip_fail(c, e, "hipEventCreate");
    }
  }
  for (hipStream_t* s : {&c->hbatch_in, &c->hbatch_out})
    if (!*s) {
      hipError_t e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
      if (e != hipSuccess) return hip_fail(c, e, "hipStreamCreate");
    }
  if (h.dev_bytes < dev_bytes) {
    (void)hipStreamSynchronize(c->hbatch_in);
    (void)hipStreamSynchronize(c->hbatch_out);
    (void)hipStreamSynchronize(h.stream);
    if (h.dev) (void)hipFree(h.dev);
    h.dev = nullptr;
    h.dev_bytes = 0;
    hipError_t e = hipMalloc(&h.dev, dev_bytes);
    if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipMalloc(%zu): %s", dev_bytes, hipGetErrorString(e));
    h.dev_bytes = dev_bytes;
  }
  if (h.pin_bytes < pin_bytes) {
    (void)hipStreamSynchronize(c->hbatch_in);
    (void)hipStreamSynchronize(c->hbatch_out);
    (void)hipStreamSynchronize(h.stream);
    if (h.pin) (void)hipHostFree(h.pin);
    h.pin = nullptr;
    h.pin_dev = nullptr;
    h.pin_bytes = 0;
    hipError_t e = hipHostMalloc(&h.pin, pin_bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipHostMalloc(%zu): %s", pin_bytes, hipGetErrorString(e));
    if (!host_device_ptr(h.pin, pin_bytes, &h.pin_dev)) h.pin_dev = nullptr;
    h.pin_bytes = pin_bytes;
  }
  return HRS_OK;
}

// Rows moved for one stripe: runs of consecutive locations [l0, l0 + cnt).
struct RowRun {
  int l0, cnt;
};

// H2D of `runs` of stripe i of the chunk: host rows at hsrc + l * hrow (host
// stripe base), device rows at ddst + l * dpitch.
hrs_status h2d_runs(hrs_codec* c, const std::vector<RowRun>& runs, uint8_t* ddst, size_t dpitch, const uint8_t* hsrc,
                    size_t hrow, size_t len, hipStream_t s) {
  for (const RowRun& r : runs) {
    hipError_t e;
    if (r.cnt == 1 || (hrow == len && dpitch == len))
      e = hipMemcpyAsync(ddst + r.l0 * dpitch, hsrc + r.l0 * hrow, (r.cnt - 1) * dpitch + len, hipMemcpyHostToDevice, s);
    else
      e = hipMemcpy2DAsync(ddst + r.l0 * dpitch, dpitch, hsrc + r.l0 * hrow, hrow, len, r.cnt, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(c, e, "H2D");
  }
  return HRS_OK;
}

hrs_status d2h_rows(hrs_codec* c, uint8_t* hdst, size_t hrow, const uint8_t* dsrc, size_t dpitch, size_t len, int cnt,
                    hipStream_t s) {
  if (cnt <= 0) return HRS_OK;
  hipError_t e;
  if (cnt == 1 || (hrow == len && dpitch == len))
    e = hipMemcpyAsync(hdst, dsrc, (cnt - 1) * dpitch + len, hipMemcpyDeviceToHost, s);
  else
    e = hipMemcpy2DAsync(hdst, hrow, dsrc, dpitch, len, cnt, hipMemcpyDeviceToHost, s);
  return e == hipSuccess ? HRS_OK : hip_fail(c, e, "D2H");
}

std::vector<RowRun> runs_of(const int* locs, int nlocs) {  // locs ascending
  std::vector<RowRun> v;
  for (int i = 0; i < nlocs; ++i) {
    if (!v.empty() && v.back().l0 + v.back().cnt == locs[i])
      ++v.back().cnt;
    else
      v.push_back({locs[i], 1});
  }
  return v;
}

// The whole-job driver. Per chunk [s0, s0 + ns): `reads(i)` lists the row
// runs stripe s0 + i needs on the device, `compute(slot, s0, ns, dimg,
// dout)` queues the kernels on the slot's stream, `writes(i)` = how many
// output rows stripe s0 + i has (rows 0.. of its output block). Host
// stripe s: rows at hin + s * in_stripe + l * in_row; outputs at
// hout + s * out_stripe + t * out_row. out_rows_max may be 0 (the scrub
// reads only): no output block, nothing copied back.
// `dirty` (optional; the heal): for jobs whose kernels write into the image.
// Once a chunk's kernels have finished, dirty(s0, ns, cells) lists the cells
// (stripe index in the chunk, location) they changed; exactly those go back
// from the slot's image to the caller's rows at hin, before the slot is
// refilled: out of the pinned staging through the copy pool (zero copy), or
// with a synchronous D2H out of the device image (copy engines; a rare path).
struct DirtyCell {
  size_t i;
  int l;
};
template <typename Reads, typename Compute, typename Writes, typename Dirty = std::nullptr_t>
hrs_status host_batch(hrs_codec* c, const uint8_t* hin, size_t in_row, size_t in_stripe, int img_rows, uint8_t* hout,
                      size_t out_row, size_t out_stripe, int out_rows_max, size_t len, size_t nstripes, Reads reads,
                      Compute compute, Writes writes, Dirty dirty = nullptr) {
  constexpr bool has_dirty = !std::is_same_v<Dirty, std::nullptr_t>;
  const size_t dpitch = (len + 255) & ~static_cast<size_t>(255);
  const size_t img_stripe = dpitch * static_cast<size_t>(img_rows);
  const size_t out_stripe_dev = dpitch * static_cast<size_t>(out_rows_max);
  size_t chunk = std::max<size_t>(1, hbatch_target_bytes() / std::max<size_t>(1, img_stripe));
  chunk = std::min(chunk, nstripes);
  // out_rows_max == 0: a read-only job (the scrub), hout is not touched
  const bool pinned = runtime_pinned(hin, batch_span(nstripes, in_stripe, img_rows, in_row, len)) &&
                      (out_rows_max == 0 ||
                       runtime_pinned(hout, batch_span(nstripes, out_stripe, out_rows_max, out_row, len)));
  const size_t dev_bytes = chunk * (img_stripe + out_stripe_dev);
  const size_t pin_bytes = pinned ? 0 : dev_bytes;  // staging mirrors the device image
  // pageable callers, zero copy: the kernels read each chunk's image from the
  // slot's pinned staging and write its outputs there (no device image, no
  // H2D / D2H); the host copies in and out of staging as before
  bool zc = !pinned && zero_copy_on();
  for (int i = 0; i < hrs::kHostBatchSlots; ++i) {
    hrs_status st = hbatch_slot(c, i, zc ? 0 : dev_bytes, pin_bytes);
    if (st != HRS_OK) return st;
  }
  uint8_t* zc_img[hrs::kHostBatchSlots] = {};
  for (int i = 0; i < hrs::kHostBatchSlots && zc; ++i) zc &= (zc_img[i] = c->hbatch[i].pin_dev) != nullptr;
  for (int i = 0; i < hrs::kHostBatchSlots && !zc && !pinned; ++i) {  // staging not device-mapped: copy engine
    hrs_status st = hbatch_slot(c, i, dev_bytes, pin_bytes);
    if (st != HRS_OK) return st;
  }
  hrs::GridCap cap(zc ? zero_copy_blocks() : 0u);
  hrs::CopyPool& pool = copy_pool(c);
  const uint8_t nt = host_store_mode();
  std::vector<hrs::CopyJob> jobs;
  const bool duplex = hbatch_duplex();
  const bool merge = hbatch_merge();
  struct Pending {
    bool busy = false;
    bool used = false;  // the slot's events have been recorded by this call
    size_t s0 = 0, ns = 0;
  } pend[hrs::kHostBatchSlots];
  std::vector<DirtyCell> cells;
  // wait for a slot; pageable: queue the copies of its outputs out of
  // staging in `jobs` (the caller runs them, merged with the slot's next
  // copy-in: the output block and the input image are disjoint)
  auto finish = [&](int sl) -> hrs_status {
    if (!pend[sl].busy) return HRS_OK;
    hrs_codec::HostBatchSlot& h = c->hbatch[sl];
    hipError_t e = hipEventSynchronize(h.done);
    if (e != hipSuccess) return hip_fail(c, e, "hipEventSynchronize");
    if (!pinned) {
      const uint8_t* pout = h.pin + chunk * img_stripe;
      for (size_t i = 0; i < pend[sl].ns; ++i) {
        const size_t s = pend[sl].s0 + i;
        for (int t = 0; t < writes(s); ++t)
          jobs.push_back({hout + s * out_stripe + t * out_row, pout + i * out_stripe_dev + t * dpitch, len});
      }
    }
    if constexpr (has_dirty) {
      cells.clear();
      hrs_status st = dirty(pend[sl].s0, pend[sl].ns, cells);
      if (st != HRS_OK) return st;
      for (const DirtyCell& d : cells) {
        uint8_t* dst = const_cast<uint8_t*>(hin) + (pend[sl].s0 + d.i) * in_stripe + d.l * in_row;
        const size_t at = d.i * img_stripe + d.l * dpitch;
        if (zc) {
          jobs.push_back({dst, h.pin + at, len});
        } else if ((e = hipMemcpy(dst, h.dev + at, len, hipMemcpyDeviceToHost)) != hipSuccess) {
          return hip_fail(c, e, "D2H of a healed cell");
        }
      }
    }
    pend[sl].busy = false;
    return HRS_OK;
  };
  size_t j = 0;
  for (size_t s0 = 0; s0 < nstripes; s0 += chunk, ++j) {
    const int sl = static_cast<int>(j % hrs::kHostBatchSlots);
    hrs_codec::HostBatchSlot& h = c->hbatch[sl];
    const size_t ns = std::min(chunk, nstripes - s0);
    if (!pinned || has_dirty) {
      jobs.clear();
      hrs_status st = finish(sl);
      if (st != HRS_OK) return st;
      // dirty cells leave the staging image before the next copy-in overwrites it
      if ((!merge || has_dirty) && !jobs.empty()) {
        pool.run(jobs);
        jobs.clear();
      }
    }
    if (!pinned) {
      for (size_t i = 0; i < ns; ++i)
        for (const RowRun& r : reads(s0 + i))
          for (int q = 0; q < r.cnt; ++q) {
            const int l = r.l0 + q;
            jobs.push_back({h.pin + i * img_stripe + l * dpitch, hin + (s0 + i) * in_stripe + l * in_row, len, nt});
          }
      pool.run(jobs);
    }
    // stream of each stage; in duplex mode the H2D waits until the slot's
    // previous kernels have read its image, the kernels until the previous
    // D2H has read its output block, the D2H until this chunk's kernels
    hipError_t e = hipSuccess;
    if (zc) {  // the kernels work on the staging itself
      uint8_t* zimg = zc_img[sl];
      hrs_status st = compute(h.stream, s0, ns, zimg, img_stripe, dpitch, zimg + chunk * img_stripe, out_stripe_dev);
      if (st != HRS_OK) return st;
      if ((e = hipEventRecord(h.done, h.stream)) != hipSuccess) return hip_fail(c, e, "hipEventRecord");
      pend[sl].busy = pend[sl].used = true;
      pend[sl].s0 = s0;
      pend[sl].ns = ns;
      continue;
    }
    const hipStream_t s_in = duplex ? c->hbatch_in : h.stream;
    const hipStream_t s_out = duplex ? c->hbatch_out : h.stream;
    if (duplex && pend[sl].used && (e = hipStreamWaitEvent(s_in, h.comp_done, 0)) != hipSuccess)
      return hip_fail(c, e, "hipStreamWaitEvent");
    uint8_t* dimg = h.dev;
    uint8_t* dout = h.dev + chunk * img_stripe;
    for (size_t i = 0; i < ns; ++i) {
      const uint8_t* src = pinned ? hin + (s0 + i) * in_stripe : h.pin + i * img_stripe;
      hrs_status st = h2d_runs(c, reads(s0 + i), dimg + i * img_stripe, dpitch, src, pinned ? in_row : dpitch, len,
                               s_in);
      if (st != HRS_OK) return st;
    }
    if (duplex) {
      if ((e = hipEventRecord(h.in_done, s_in)) != hipSuccess) return hip_fail(c, e, "hipEventRecord");
      if ((e = hipStreamWaitEvent(h.stream, h.in_done, 0)) != hipSuccess) return hip_fail(c, e, "hipStreamWaitEvent");
      if (pend[sl].used && (e = hipStreamWaitEvent(h.stream, h.done, 0)) != hipSuccess)
        return hip_fail(c, e, "hipStreamWaitEvent");
    }
    hrs_status st = compute(h.stream, s0, ns, dimg, img_stripe, dpitch, dout, out_stripe_dev);
    if (st != HRS_OK) return st;
    if (duplex) {
      if ((e = hipEventRecord(h.comp_done, h.stream)) != hipSuccess) return hip_fail(c, e, "hipEventRecord");
      if ((e = hipStreamWaitEvent(s_out, h.comp_done, 0)) != hipSuccess) return hip_fail(c, e, "hipStreamWaitEvent");
    }
    for (size_t i = 0; i < ns; ++i) {
      const size_t s = s0 + i;
      st = pinned ? d2h_rows(c, hout + s * out_stripe, out_row, dout + i * out_stripe_dev, dpitch, len, writes(s), s_out)
                  : d2h_rows(c, h.pin + chunk * img_stripe + i * out_stripe_dev, dpitch, dout + i * out_stripe_dev,
                             dpitch, len, writes(s), s_out);
      if (st != HRS_OK) return st;
    }
    if ((e = hipEventRecord(h.done, s_out)) != hipSuccess) return hip_fail(c, e, "hipEventRecord");
    pend[sl].busy = true;
    pend[sl].used = true;
    pend[sl].s0 = s0;
    pend[sl].ns = ns;
  }
  for (int k = 1; k <= hrs::kHostBatchSlots; ++k) {  // in chunk order
    jobs.clear();
    hrs_status st = finish(static_cast<int>((j + k - 1) % hrs::kHostBatchSlots));
    if (st != HRS_OK) return st;
    if (!jobs.empty()) pool.run(jobs);
  }
  return HRS_OK;
}

// A failed host batch may leave slot work in flight: drain every slot stream.
hrs_status drain_hbatch(hrs_codec* c, hrs_status st) {
  if (st != HRS_OK) {
    for (hipStream_t s : {c->hbatch_in, c->hbatch_out})
      if (s) (void)hipStreamSynchronize(s);
    for (auto& h : c->hbatch)
      if (h.stream) (void)hipStreamSynchronize(h.stream);
  }
  return st;
}

// hrs_decode_batch_host with pinned stripes and outputs: one batch launch
// whose kernels read the survivors and write the repaired cells across the
// host link directly (zero copy). The plans go up first on slot 0's stream;
// the call returns once the launch has completed. dcrc_out (device, with
// dcrc_in; hrs_decode_batch_host_crc): launch_batch_crc over max_erased rows.
hrs_status zero_copy_batch(hrs_codec* c, const BatchPlanSet& ps, const uint8_t* ds, size_t row_stride,
                           size_t stripe_stride, uint8_t* dout, size_t out_row_stride, size_t out_stripe_stride,
                           size_t len, size_t nstripes, int max_erased = 0, const uint32_t* dcrc_in = nullptr,
                           uint32_t* dcrc_out = nullptr) {
  hrs_status st = hbatch_slot(c, 0, 0, 0);
  if (st != HRS_OK) return st;
  const hipStream_t hs = c->hbatch[0].stream;
  hrs_codec::BatchSlot* bsl = nullptr;
  const hrs::BatchPlan* dplans = nullptr;
  const int32_t* dpat = nullptr;
  if (ps.fused || dcrc_out) {
    st = upload_batch_plans(c, ps, hs, &bsl, &dplans, &dpat);
    if (st != HRS_OK) return st;
  }
  if (dcrc_out) {
    st = crc_scratch(c, crc_raw_bytes_for(len, nstripes, max_erased), hs);
    if (st != HRS_OK) return st;
    hrs::GridCap cap(zero_copy_blocks());
    st = crc_scratch_release(c, hs,
                             launch_batch_crc(c, ps, dplans, dpat, ds, row_stride, stripe_stride, dout, out_row_stride,
                                              out_stripe_stride, len, 0, nstripes, max_erased, dcrc_in, dcrc_out, hs,
                                              c->crc_raw));
  } else {
    hrs::GridCap cap(zero_copy_blocks());
    st = launch_batch(c, ps, dplans, dpat, ds, row_stride, stripe_stride, dout, out_row_stride, out_stripe_stride,
                      len, 0, nstripes, hs);
  }
  if (st != HRS_OK) return st;
  if (bsl) {
    const hipError_t e = hipEventRecord(bsl->done, hs);
    if (e != hipSuccess) return hip_fail(c, e, "hipEventRecord");
    bsl->pending = true;
  }
  const hipError_t e = hipStreamSynchronize(hs);
  return e == hipSuccess ? HRS_OK : hip_fail(c, e, "hipStreamSynchronize");
}

// ---------------------------------------------- device sets (hrs_*_multi)
// contiguous stripe ranges, one host thread per device, no data
// exchange. Each range is an ordinary single-handle host batch; the handles
// are independent (their own slots, streams and staging), so the ranges run
// concurrently with no shared state beyond the process-wide copy pool, which
// takes batches from every open call in turn.

hrs_status check_device_set(hrs_codec* const* cs, int nc) {
  if (!cs || nc < 1) return fail(nullptr, HRS_EINVAL, "device set: need at least one codec");
  for (int i = 0; i < nc; ++i)
    if (!cs[i]) return fail(cs[0] ? cs[0] : nullptr, HRS_EINVAL, "device set: codecs[%d] is NULL", i);
  hrs_codec* c0 = cs[0];
  if (nc > 1024) return fail(c0, HRS_EINVAL, "device set: %d codecs (at most 1024)", nc);
  for (int i = 0; i < nc; ++i) {
    const hrs_codec* c = cs[i];
    if (c->kind != c0->kind || c->k != c0->k || c->p != c0->p || c->src_s != c0->src_s)
      return fail(c0, HRS_EINVAL, "device set: codecs[%d] is another code than codecs[0]", i);
    for (int j = 0; j < i; ++j)
      if (cs[j] == c) return fail(c0, HRS_EINVAL, "device set: codecs[%d] and codecs[%d] are one handle", j, i);
  }
  for (int i = 0; i < nc; ++i)
    if (cs[i]->device < 0) return fail(c0, HRS_EDEVICE, "device set: codecs[%d] is a host-only handle", i);
  return HRS_OK;
}

// Runs f(codec, first stripe, stripe count) for each member's range on its
// own thread (member 0 on the caller's); returns the first failing member's
// status with its message moved to codecs[0].
template <typename F>
hrs_status run_device_set(hrs_codec* const* cs, int nc, size_t nstripes, F f) {
  std::vector<hrs_status> st(nc, HRS_OK);
  auto lo = [&](int i) { return static_cast<size_t>((static_cast<unsigned __int128>(nstripes) * i) / nc); };
  auto member = [&](int i) {
    const size_t a = lo(i), b = lo(i + 1);
    if (b > a) st[i] = f(cs[i], a, b - a);
  };
  std::vector<std::thread> th;
  th.reserve(nc);
  int inline_from = nc;  // members a thread could not be started for run here
  for (int i = 1; i < nc; ++i) {
    try {
      th.emplace_back(member, i);
    } catch (const std::exception&) {
      inline_from = i;
      break;
    }
  }
  member(0);
  for (int i = inline_from; i < nc; ++i) member(i);
  for (auto& t : th) t.join();
  for (int i = 0; i < nc; ++i)
    if (st[i] != HRS_OK) {
      if (i > 0) {
        const std::string msg = cs[i]->err;
        fail(cs[0], st[i], "device set member %d (device %d), stripes [%zu, %zu): %s", i, cs[i]->device, lo(i),
             lo(i + 1), msg.c_str());
      }
      return st[i];
    }
  return HRS_OK;
}

}  // namespace hrs::api

using namespace hrs::api;

namespace {

// hrs_last_host_path of a host batch: "pinned" when the stripes (and a
// decode's outputs) lie in runtime-pinned memory and zero copy is on.
const char* batch_path(bool pinned) {
  if (!zero_copy_on()) return "copy_engine";
  return pinned ? "pinned" : "staged";
}

hrs_status decode_batch_host_impl(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                  const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                  size_t out_stripe_stride, size_t len, size_t nstripes,
                                  const uint32_t* crc_in = nullptr, uint32_t* crc_out = nullptr) {
  if (!c) return HRS_EINVAL;
  if (!stripes || !out || max_erased < 0 || max_erased > hrs::kMaxOut || (max_erased > 0 && !erased))
    return fail(c, HRS_EINVAL, "bad batch decode arguments (max_erased must be in [0, %d])", hrs::kMaxOut);
  if (nstripes == 0 || len == 0 || max_erased == 0) return HRS_OK;
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  BatchPlanSet ps;
  hrs_status st = build_batch_plans(c, erased, max_erased, nstripes, ps);
  if (st != HRS_OK) return st;
  if (ps.max_nout == 0 && !crc_out) return HRS_OK;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  // hrs_decode_batch_host_crc (crc_out != NULL; HOST arrays): the CRCs
  // accumulate in the handle's device buffer, filled from crc_in, written by
  // the slot streams' folds, and come back in one copy after the last chunk
  const size_t ncrc = nstripes * static_cast<size_t>(max_erased);
  const uint32_t* dcrc_in = nullptr;
  if (crc_out) {
    if (ps.max_nout == 0) {  // nothing lost anywhere: every CRC continues over no bytes
      if (crc_in) std::memmove(crc_out, crc_in, ncrc * sizeof(uint32_t));
      else std::memset(crc_out, 0, ncrc * sizeof(uint32_t));
      return HRS_OK;
    }
    st = hbatch_crc_buffer(c, ncrc, crc_in);
    if (st != HRS_OK) return st;
    if (crc_in) dcrc_in = c->hbatch_crc;
  }
  uint32_t* const dcrc = crc_out ? c->hbatch_crc : nullptr;
  uint8_t *zs = nullptr, *zo = nullptr;
  if (zero_copy_on() && host_device_ptr(stripes, batch_span(nstripes, stripe_stride, c->n, row_stride, len), &zs) &&
      host_device_ptr(out, batch_span(nstripes, out_stripe_stride, max_erased, out_row_stride, len), &zo)) {
    st = drain_hbatch(c, zero_copy_batch(c, ps, zs, row_stride, stripe_stride, zo, out_row_stride, out_stripe_stride,
                                         len, nstripes, max_erased, dcrc_in, dcrc));
    return st == HRS_OK && crc_out ? hbatch_crc_fetch(c, ncrc, crc_out) : st;
  }
  // rows each pattern reads: its live locations (every location for the
  // per-stripe fallback of wide patterns, which reads what its matrix needs)
  std::vector<std::vector<RowRun>> pruns(ps.plans.size());
  for (size_t id = 0; id < ps.plans.size(); ++id) {
    const hrs::BatchPlan& pl = ps.plans[id];
    if (pl.nin <= hrs::kBatchMaxIn) {
      pruns[id] = runs_of(pl.loc, pl.nin);
    } else {
      std::vector<int> live;
      for (int l = 0; l < c->n; ++l)
        for (int o = 0; o < pl.nout; ++o)
          if (ps.mats[id][static_cast<size_t>(o) * c->n + l]) {
            live.push_back(l);
            break;
          }
      pruns[id] = runs_of(live.data(), static_cast<int>(live.size()));
    }
  }
  // plans + pattern indices: one upload for the whole job, on slot 0's
  // stream; the other slot streams wait for it
  hrs_codec::BatchSlot* bsl = nullptr;
  const hrs::BatchPlan* dplans = nullptr;
  const int32_t* dpat = nullptr;
  st = hbatch_slot(c, 0, 0, 0);
  if (st != HRS_OK) return st;
  if (ps.fused || crc_out) {
    st = upload_batch_plans(c, ps, c->hbatch[0].stream, &bsl, &dplans, &dpat);
    if (st != HRS_OK) return st;
    hipError_t e = hipEventRecord(bsl->done, c->hbatch[0].stream);
    if (e != hipSuccess) return hip_fail(c, e, "hipEventRecord");
    bsl->pending = true;
    for (int i = 1; i < hrs::kHostBatchSlots; ++i) {
      st = hbatch_slot(c, i, 0, 0);
      if (st != HRS_OK) return st;
      e = hipStreamWaitEvent(c->hbatch[i].stream, bsl->done, 0);
      if (e != hipSuccess) return hip_fail(c, e, "hipStreamWaitEvent");
    }
  }
  auto reads = [&](size_t s) -> const std::vector<RowRun>& { return pruns[ps.pat[s]]; };
  auto writes = [&](size_t s) -> int { return ps.plans[ps.pat[s]].nout; };
  auto compute = [&](hipStream_t hs, size_t s0, size_t ns, uint8_t* dimg, size_t img_stripe, size_t dpitch,
                     uint8_t* dout, size_t out_stripe_dev) -> hrs_status {
    if (!dcrc)
      return launch_batch(c, ps, dplans, dpat, dimg, dpitch, img_stripe, dout, dpitch, out_stripe_dev, len, s0, ns, hs);
    // the slots share the handle's raw-CRC scratch: crc_scratch chains its
    // uses by an event, so the slots' CRC kernels run one after another
    // (each fills the chip); their copies still overlap them
    hrs_status cs = crc_scratch(c, crc_raw_bytes_for(len, ns, max_erased), hs);
    if (cs != HRS_OK) return cs;
    const size_t at = s0 * static_cast<size_t>(max_erased);
    return crc_scratch_release(c, hs,
                               launch_batch_crc(c, ps, dplans, dpat, dimg, dpitch, img_stripe, dout, dpitch,
                                                out_stripe_dev, len, s0, ns, max_erased,
                                                dcrc_in ? dcrc_in + at : nullptr, dcrc + at, hs, c->crc_raw));
  };
  st = host_batch(c, stripes, row_stride, stripe_stride, c->n, out, out_row_stride, out_stripe_stride, ps.max_nout,
                  len, nstripes, reads, compute, writes);
  if (st == HRS_OK && bsl) {  // the plan slot is reused only after this job's kernels
    hipError_t e = hipEventRecord(bsl->done, c->hbatch[0].stream);
    if (e != hipSuccess) st = hip_fail(c, e, "hipEventRecord");
  }
  st = drain_hbatch(c, st);
  return st == HRS_OK && crc_out ? hbatch_crc_fetch(c, ncrc, crc_out) : st;
}

// crc_out != NULL (hrs_encode_batch_host_crc; HOST arrays of nstripes * n
// words): encode_crc_impl instead of run_apply, the CRCs through the handle's
// device buffer as in decode_batch_host_impl.
hrs_status encode_batch_host_impl(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride, size_t len,
                                  size_t nstripes, const uint32_t* crc_in = nullptr, uint32_t* crc_out = nullptr) {
  if (!c) return HRS_EINVAL;
  if (!stripes) return fail(c, HRS_EINVAL, "stripes is NULL");
  if (nstripes == 0 || len == 0) return HRS_OK;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  const int k = c->k, p = c->p;
  const size_t n = static_cast<size_t>(c->n), ncrc = nstripes * n;
  const uint32_t* dcrc_in = nullptr;
  if (crc_out) {
    hrs_status st = hbatch_crc_buffer(c, ncrc, crc_in);
    if (st != HRS_OK) return st;
    if (crc_in) dcrc_in = c->hbatch_crc;
  }
  uint32_t* const dcrc = crc_out ? c->hbatch_crc : nullptr;
  // encode + CRC of stripes [s0, s0 + ns) on hs, the raw scratch chained across the slot streams
  auto encode_crc = [&](const uint8_t* const* in, size_t in_stride, uint8_t* const* outp, size_t out_stride, size_t s0,
                        size_t ns, hipStream_t hs) -> hrs_status {
    hrs_status cs = crc_scratch(c, crc_raw_bytes_for(len, ns, c->n), hs);
    if (cs != HRS_OK) return cs;
    return crc_scratch_release(c, hs,
                               encode_crc_impl(c, in, in_stride, outp, out_stride, len, ns,
                                               dcrc_in ? dcrc_in + s0 * n : nullptr, dcrc + s0 * n, hs, c->crc_raw));
  };
  uint8_t* zs = nullptr;
  if (zero_copy_on() && host_device_ptr(stripes, batch_span(nstripes, stripe_stride, c->n, row_stride, len), &zs)) {
    // runtime-pinned: the kernel works on the caller's stripes in place
    hrs_status st = hbatch_slot(c, 0, 0, 0);
    if (st != HRS_OK) return st;
    const hipStream_t hs = c->hbatch[0].stream;
    std::vector<const uint8_t*> in(k);
    std::vector<uint8_t*> outp(p);
    for (int i = 0; i < k; ++i) in[i] = zs + static_cast<size_t>(p + i) * row_stride;
    for (int r = 0; r < p; ++r) outp[r] = zs + static_cast<size_t>(r) * row_stride;
    {
      hrs::GridCap cap(zero_copy_blocks());
      st = dcrc ? encode_crc(in.data(), stripe_stride, outp.data(), stripe_stride, 0, nstripes, hs)
                : run_apply(c, c->g.data(), p, k, in.data(), stripe_stride, outp.data(), stripe_stride, len, nstripes,
                            hs, static_encode_family(c));
    }
    if (st == HRS_OK) {
      const hipError_t e = hipStreamSynchronize(hs);
      if (e != hipSuccess) st = hip_fail(c, e, "hipStreamSynchronize");
    }
    st = drain_hbatch(c, st);
    return st == HRS_OK && crc_out ? hbatch_crc_fetch(c, ncrc, crc_out) : st;
  }
  const std::vector<RowRun> data_rows{{p, k}};  // hops locations p..n-1: one run
  auto reads = [&](size_t) -> const std::vector<RowRun>& { return data_rows; };
  auto writes = [&](size_t) -> int { return p; };
  std::vector<const uint8_t*> in(k);
  std::vector<uint8_t*> outp(p);
  auto compute = [&](hipStream_t hs, size_t s0, size_t ns, uint8_t* dimg, size_t img_stripe, size_t dpitch,
                     uint8_t* dout, size_t out_stripe_dev) -> hrs_status {
    for (int i = 0; i < k; ++i) in[i] = dimg + static_cast<size_t>(p + i) * dpitch;
    for (int r = 0; r < p; ++r) outp[r] = dout + static_cast<size_t>(r) * dpitch;
    if (dcrc) return encode_crc(in.data(), img_stripe, outp.data(), out_stripe_dev, s0, ns, hs);
    return run_apply(c, c->g.data(), p, k, in.data(), img_stripe, outp.data(), out_stripe_dev, len, ns, hs,
                     static_encode_family(c));
  };
  // parity rows 0..p-1 of each stripe are written in place
  const hrs_status st = drain_hbatch(c, host_batch(c, stripes, row_stride, stripe_stride, c->n, stripes, row_stride,
                                                   stripe_stride, p, len, nstripes, reads, compute, writes));
  return st == HRS_OK && crc_out ? hbatch_crc_fetch(c, ncrc, crc_out) : st;
}

// hrs_scrub_batch_host: every stripe's n rows are its reads, there are no
// output rows; the reports accumulate in the handle's device buffer (dense,
// 4 + n words per stripe) and come back in one copy.
// heal (hrs_heal_batch_host): the heal kernels, which patch the image they
// read. Pinned stripes are patched in place across the link; a staged chunk's
// reports are fetched when its kernels have finished and the cells with a
// nonzero count in word 4 + l go back to the caller (host_batch's dirty hook).
// crc_out != NULL (hrs_scrub_batch_host_crc, hrs_heal_batch_host_crc; HOST
// arrays of nstripes * n words, hops order): run_scrub_crc instead of
// run_scrub, the CRCs through the handle's device buffer as in
// encode_batch_host_impl. A pinned cell crosses the link once when the shape
// takes the one-pass kernel (the heal's dirty windows twice).
// es != NULL (hrs_heal_erased_batch_host[_crc]; heal is set): run_heal_erased
// / run_heal_erased_crc with each chunk's slice of pattern indices, uploaded
// with the table through a batch slot on the chunk's stream (two slots:
// acquiring one waits for the chunk that used it two chunks earlier). A
// stripe's erased cells are never read, so a staged chunk copies in only the
// survivor rows (the slot image keeps stale bytes at erased rows; the kernels
// write every byte of them) and copies back the erased cells plus the cells
// with a nonzero count in word 4 + l.
hrs_status scrub_batch_host_impl(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                 size_t len, size_t nstripes, uint32_t* reports, size_t report_stride, bool heal,
                                 const uint32_t* crc_in = nullptr, uint32_t* crc_out = nullptr,
                                 const ErasedSets* es = nullptr) {
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  const int n = c->n;
  const size_t ncrc = nstripes * static_cast<size_t>(n);
  const uint32_t* dcrc_in = nullptr;
  if (crc_out) {
    hrs_status cs = hbatch_crc_buffer(c, ncrc, crc_in);
    if (cs != HRS_OK) return cs;
    if (crc_in) dcrc_in = c->hbatch_crc;
  }
  uint32_t* const dcrc = crc_out ? c->hbatch_crc : nullptr;
  // the scrub or heal of stripes [s0, s0 + ns) on hs, with their CRCs when asked
  auto scrub = [&](const uint8_t* const* r, size_t stride, size_t s0, size_t ns, uint32_t* rep,
                   hipStream_t hs) -> hrs_status {
    if (es) {
      uint8_t* const* w = reinterpret_cast<uint8_t* const*>(const_cast<uint8_t**>(r));
      if (!dcrc)
        return run_heal_erased(c, w, stride, len, ns, es->pats, es->pat.data() + s0, rep,
                               static_cast<size_t>(hrs::kScrubHead + n), hs);
      return run_heal_erased_crc(c, w, stride, len, ns, es->pats, es->pat.data() + s0, rep,
                                 static_cast<size_t>(hrs::kScrubHead + n), dcrc_in ? dcrc_in + s0 * n : nullptr,
                                 dcrc + s0 * n, hs, on_host(r[0]));
    }
    if (!dcrc) return run_scrub(c, r, stride, len, ns, rep, static_cast<size_t>(hrs::kScrubHead + n), hs, heal);
    return run_scrub_crc(c, r, stride, len, ns, rep, static_cast<size_t>(hrs::kScrubHead + n),
                         dcrc_in ? dcrc_in + s0 * n : nullptr, dcrc + s0 * n, hs, heal);
  };
  const size_t nwords = static_cast<size_t>(hrs::kScrubHead + n);
  const size_t bytes = nstripes * nwords * sizeof(uint32_t);
  if (c->scrub_reports_bytes < bytes) {  // every earlier batch has completed: the calls are synchronous
    if (c->scrub_reports) (void)hipFree(c->scrub_reports);
    c->scrub_reports = nullptr;
    c->scrub_reports_bytes = 0;
    const hipError_t e = hipMalloc(&c->scrub_reports, bytes);
    if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    c->scrub_reports_bytes = bytes;
  }
  uint32_t* drep = c->scrub_reports;
  std::vector<const uint8_t*> rows(n);
  hrs_status st = hbatch_slot(c, 0, 0, 0);
  if (st != HRS_OK) return st;
  uint8_t* zs = nullptr;
  if (zero_copy_on() && host_device_ptr(stripes, batch_span(nstripes, stripe_stride, n, row_stride, len), &zs)) {
    // runtime-pinned: one launch reads the caller's stripes across the host link
    const hipStream_t hs = c->hbatch[0].stream;
    for (int l = 0; l < n; ++l) rows[l] = zs + static_cast<size_t>(l) * row_stride;
    {
      hrs::GridCap cap(zero_copy_blocks());
      st = scrub(rows.data(), stripe_stride, 0, nstripes, drep, hs);
    }
    if (st == HRS_OK) {
      const hipError_t e = hipStreamSynchronize(hs);
      if (e != hipSuccess) st = hip_fail(c, e, "hipStreamSynchronize");
    }
  } else {
    const std::vector<RowRun> all_rows{{0, n}};
    std::vector<std::vector<RowRun>> survivor_runs(es ? es->keys.size() : 0);  // per pattern
    for (size_t id = 0; id < survivor_runs.size(); ++id) {
      std::vector<int> live;
      for (int l = 0; l < n; ++l)
        if (!std::binary_search(es->keys[id].begin(), es->keys[id].end(), l)) live.push_back(l);
      survivor_runs[id] = runs_of(live.data(), static_cast<int>(live.size()));
    }
    auto reads = [&](size_t s) -> const std::vector<RowRun>& { return es ? survivor_runs[es->pat[s]] : all_rows; };
    auto writes = [&](size_t) -> int { return 0; };
    auto compute = [&](hipStream_t hs, size_t s0, size_t ns, uint8_t* dimg, size_t img_stripe, size_t dpitch, uint8_t*,
                       size_t) -> hrs_status {
      for (int l = 0; l < n; ++l) rows[l] = dimg + static_cast<size_t>(l) * dpitch;
      return scrub(rows.data(), img_stripe, s0, ns, drep + s0 * nwords, hs);
    };
    std::vector<uint32_t> chunk_rep;
    auto dirty = [&](size_t s0, size_t ns, std::vector<DirtyCell>& cells) -> hrs_status {
      chunk_rep.resize(ns * nwords);
      const hipError_t e = hipMemcpy(chunk_rep.data(), drep + s0 * nwords, ns * nwords * sizeof(uint32_t),
                                     hipMemcpyDeviceToHost);
      if (e != hipSuccess) return hip_fail(c, e, "hipMemcpy chunk reports");
      for (size_t i = 0; i < ns; ++i) {
        if (es)  // the rebuilt cells (never blamed: their count is 0)
          for (int l : es->keys[es->pat[s0 + i]]) cells.push_back({i, l});
        for (int l = 0; l < n; ++l)
          if (chunk_rep[i * nwords + hrs::kScrubHead + l] != 0) cells.push_back({i, l});
      }
      return HRS_OK;
    };
    st = heal ? host_batch(c, stripes, row_stride, stripe_stride, n, const_cast<uint8_t*>(stripes), row_stride,
                           stripe_stride, 0, len, nstripes, reads, compute, writes, dirty)
              : host_batch(c, stripes, row_stride, stripe_stride, n, const_cast<uint8_t*>(stripes), row_stride,
                           stripe_stride, 0, len, nstripes, reads, compute, writes);
  }
  st = drain_hbatch(c, st);
  if (st != HRS_OK) return st;
  std::vector<uint32_t> host(nstripes * nwords);
  const hipError_t e = hipMemcpy(host.data(), drep, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(c, e, "hipMemcpy reports");
  for (size_t s = 0; s < nstripes; ++s)
    std::memcpy(reports + s * report_stride, host.data() + s * nwords, nwords * sizeof(uint32_t));
  return crc_out ? hbatch_crc_fetch(c, ncrc, crc_out) : HRS_OK;
}

// hrs_scrub_batch_host and hrs_heal_batch_host: one set of argument rules.
// with_erased (hrs_heal_erased_batch_host[_crc]; heal is set): the erased
// list's rules follow the sibling's, before the empty batch as in
// hrs_heal_erased_dev, so a bad list is refused before any copy.
hrs_status scrub_batch_host_entry(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                  size_t len, size_t nstripes, uint32_t* reports, size_t report_stride, bool heal,
                                  bool with_crc = false, const uint32_t* crc_in = nullptr,
                                  uint32_t* crc_out = nullptr, bool with_erased = false, const int* erased = nullptr,
                                  int max_erased = 0) {
  hrs_status st = scrub_args_ok(c, stripes, reports, report_stride, len, nstripes, kScrubWithReports | kScrubImage,
                                with_erased ? "max_erased" : nullptr, max_erased, erased);
  if (st != HRS_OK) return st;
  ErasedSets es;
  if (with_erased && (st = erased_sets(c, erased, max_erased, nstripes, es)) != HRS_OK) return st;
  if (nstripes == 0 || len == 0) return HRS_OK;
  // A read-only pass over a mis-strided batch would report "clean" or "bad"
  // with no error: the cells must not overlap. Rows of a stripe packed inside
  // the stripe stride, or stripes of a row packed inside the row stride.
  const size_t rows_span = static_cast<size_t>(c->n - 1) * row_stride + len;
  const size_t stripes_span = (nstripes - 1) * stripe_stride + len;
  const bool stripes_apart =
      nstripes == 1 || (stripe_stride >= len && (stripe_stride >= rows_span || row_stride >= stripes_span));
  if (row_stride < len || !stripes_apart)
    return fail(c, HRS_EINVAL, "cells overlap: row_stride %zu, stripe_stride %zu, len %zu, %d rows, %zu stripes",
                row_stride, stripe_stride, len, c->n, nstripes);
  if (with_crc) {
    if (!crc_out) return fail(c, HRS_EINVAL, "crc_out is NULL");
    if (!crc_arrays_apart(crc_in, crc_out, nstripes * static_cast<size_t>(c->n)))
      return fail(c, HRS_EINVAL, "crc_in and crc_out overlap (crc_out may only be crc_in itself)");
  }
  // max_erased == 0: nothing can be erased, the heal itself
  st = scrub_batch_host_impl(c, stripes, row_stride, stripe_stride, len, nstripes, reports, report_stride, heal,
                             crc_in, crc_out, with_erased && max_erased > 0 ? &es : nullptr);
  if (st == HRS_OK) {
    DeviceGuard g(c->device);
    c->last_host_path =
        batch_path(g.ok && runtime_pinned(stripes, batch_span(nstripes, stripe_stride, c->n, row_stride, len)));
  }
  return st;
}

}  // namespace

extern "C" {

hrs_status hrs_scrub_batch_host(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                size_t len, size_t nstripes, uint32_t* reports, size_t report_stride) {
  return scrub_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, reports, report_stride, false);
}

hrs_status hrs_heal_batch_host(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride, size_t len,
                               size_t nstripes, uint32_t* reports, size_t report_stride) {
  return scrub_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, reports, report_stride, true);
}

hrs_status hrs_scrub_batch_host_crc(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                    size_t len, size_t nstripes, uint32_t* reports, size_t report_stride,
                                    const uint32_t* crc_in, uint32_t* crc_out) {
  return scrub_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, reports, report_stride, false,
                                true, crc_in, crc_out);
}

hrs_status hrs_heal_batch_host_crc(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride, size_t len,
                                   size_t nstripes, uint32_t* reports, size_t report_stride, const uint32_t* crc_in,
                                   uint32_t* crc_out) {
  return scrub_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, reports, report_stride, true,
                                true, crc_in, crc_out);
}

hrs_status hrs_heal_erased_batch_host(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                      size_t len, size_t nstripes, const int* erased, int max_erased,
                                      uint32_t* reports, size_t report_stride) {
  return scrub_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, reports, report_stride, true,
                                false, nullptr, nullptr, true, erased, max_erased);
}

hrs_status hrs_heal_erased_batch_host_crc(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                          size_t len, size_t nstripes, const int* erased, int max_erased,
                                          uint32_t* reports, size_t report_stride, const uint32_t* crc_in,
                                          uint32_t* crc_out) {
  return scrub_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, reports, report_stride, true,
                                true, crc_in, crc_out, true, erased, max_erased);
}

hrs_status hrs_decode_batch_dev(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                size_t out_stripe_stride, size_t len, size_t nstripes, void* stream) {
  if (!c) return HRS_EINVAL;
  if (!stripes || !out || max_erased < 0 || max_erased > hrs::kMaxOut || (max_erased > 0 && !erased))
    return fail(c, HRS_EINVAL, "bad batch decode arguments (max_erased must be in [0, %d])", hrs::kMaxOut);
  if (nstripes == 0 || len == 0 || max_erased == 0) return HRS_OK;
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  BatchPlanSet ps;
  hrs_status st = build_batch_plans(c, erased, max_erased, nstripes, ps);
  if (st != HRS_OK) return st;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (ps.max_nout == 0) return HRS_OK;
  if (!ps.fused)  // shapes beyond the batch kernel (wide codes): one launch per stripe
    return launch_batch(c, ps, nullptr, nullptr, stripes, row_stride, stripe_stride, out, out_row_stride,
                        out_stripe_stride, len, 0, nstripes, hs);
  hrs_codec::BatchSlot* sl = nullptr;
  const hrs::BatchPlan* dplans = nullptr;
  const int32_t* dpat = nullptr;
  st = upload_batch_plans(c, ps, hs, &sl, &dplans, &dpat);
  if (st != HRS_OK) return st;
  st = launch_batch(c, ps, dplans, dpat, stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride,
                    len, 0, nstripes, hs);
  if (st != HRS_OK) return st;
  hipError_t e = hipEventRecord(sl->done, hs);
  if (e != hipSuccess) return hip_fail(c, e, "hipEventRecord");
  sl->pending = true;
  return HRS_OK;
}

hrs_status hrs_decode_batch_host(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                 const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                 size_t out_stripe_stride, size_t len, size_t nstripes) {
  if (!c) return HRS_EINVAL;
  if (!stripes || !out || max_erased < 0 || max_erased > hrs::kMaxOut || (max_erased > 0 && !erased))
    return fail(c, HRS_EINVAL, "bad batch decode arguments (max_erased must be in [0, %d])", hrs::kMaxOut);
  if (nstripes == 0 || len == 0 || max_erased == 0) return HRS_OK;
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  const hrs_status st = decode_batch_host_impl(c, stripes, row_stride, stripe_stride, erased, max_erased, out,
                                               out_row_stride, out_stripe_stride, len, nstripes);
  if (st == HRS_OK) {
    DeviceGuard g(c->device);
    c->last_host_path =
        batch_path(g.ok && runtime_pinned(stripes, batch_span(nstripes, stripe_stride, c->n, row_stride, len)) &&
                   runtime_pinned(out, batch_span(nstripes, out_stripe_stride, max_erased, out_row_stride, len)));
  }
  return st;
}

hrs_status hrs_encode_batch_host(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride, size_t len,
                                 size_t nstripes) {
  if (!c) return HRS_EINVAL;
  if (!stripes) return fail(c, HRS_EINVAL, "stripes is NULL");
  if (nstripes == 0 || len == 0) return HRS_OK;
  const hrs_status st = encode_batch_host_impl(c, stripes, row_stride, stripe_stride, len, nstripes);
  if (st == HRS_OK) {
    DeviceGuard g(c->device);
    c->last_host_path =
        batch_path(g.ok && runtime_pinned(stripes, batch_span(nstripes, stripe_stride, c->n, row_stride, len)));
  }
  return st;
}

hrs_status hrs_decode_batch_crc_dev(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                    const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                    size_t out_stripe_stride, size_t len, size_t nstripes, const uint32_t* crc_in,
                                    uint32_t* crc_out, void* stream) {
  if (!c) return HRS_EINVAL;
  if (!stripes || !out || max_erased < 0 || max_erased > hrs::kMaxOut || (max_erased > 0 && !erased))
    return fail(c, HRS_EINVAL, "bad batch decode arguments (max_erased must be in [0, %d])", hrs::kMaxOut);
  if (nstripes == 0 || len == 0 || max_erased == 0) return HRS_OK;
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  if (!crc_out) return fail(c, HRS_EINVAL, "crc_out is NULL");
  if (!crc_arrays_apart(crc_in, crc_out, nstripes * static_cast<size_t>(max_erased)))
    return fail(c, HRS_EINVAL, "crc_in and crc_out overlap (crc_out may only be crc_in itself)");
  BatchPlanSet ps;
  hrs_status st = build_batch_plans(c, erased, max_erased, nstripes, ps);
  if (st != HRS_OK) return st;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  hrs_codec::BatchSlot* sl = nullptr;
  const hrs::BatchPlan* dplans = nullptr;
  const int32_t* dpat = nullptr;
  st = upload_batch_plans(c, ps, hs, &sl, &dplans, &dpat);
  if (st != HRS_OK) return st;
  st = crc_scratch(c, crc_raw_bytes_for(len, nstripes, max_erased), hs);
  if (st != HRS_OK) return st;
  st = crc_scratch_release(c, hs,
                           launch_batch_crc(c, ps, dplans, dpat, stripes, row_stride, stripe_stride, out,
                                            out_row_stride, out_stripe_stride, len, 0, nstripes, max_erased, crc_in,
                                            crc_out, hs, c->crc_raw));
  if (st != HRS_OK) return st;
  hipError_t e = hipEventRecord(sl->done, hs);
  if (e != hipSuccess) return hip_fail(c, e, "hipEventRecord");
  sl->pending = true;
  return HRS_OK;
}

hrs_status hrs_decode_batch_host_crc(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                     const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                     size_t out_stripe_stride, size_t len, size_t nstripes, const uint32_t* crc_in,
                                     uint32_t* crc_out) {
  if (!c) return HRS_EINVAL;
  if (!stripes || !out || max_erased < 0 || max_erased > hrs::kMaxOut || (max_erased > 0 && !erased))
    return fail(c, HRS_EINVAL, "bad batch decode arguments (max_erased must be in [0, %d])", hrs::kMaxOut);
  if (nstripes == 0 || len == 0 || max_erased == 0) return HRS_OK;
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  if (!crc_out) return fail(c, HRS_EINVAL, "crc_out is NULL");
  if (!crc_arrays_apart(crc_in, crc_out, nstripes * static_cast<size_t>(max_erased)))
    return fail(c, HRS_EINVAL, "crc_in and crc_out overlap (crc_out may only be crc_in itself)");
  const hrs_status st = decode_batch_host_impl(c, stripes, row_stride, stripe_stride, erased, max_erased, out,
                                               out_row_stride, out_stripe_stride, len, nstripes, crc_in, crc_out);
  if (st == HRS_OK) {
    DeviceGuard g(c->device);
    c->last_host_path =
        batch_path(g.ok && runtime_pinned(stripes, batch_span(nstripes, stripe_stride, c->n, row_stride, len)) &&
                   runtime_pinned(out, batch_span(nstripes, out_stripe_stride, max_erased, out_row_stride, len)));
  }
  return st;
}

hrs_status hrs_encode_batch_host_crc(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                     size_t len, size_t nstripes, const uint32_t* crc_in, uint32_t* crc_out) {
  if (!c) return HRS_EINVAL;
  if (!stripes) return fail(c, HRS_EINVAL, "stripes is NULL");
  if (nstripes == 0 || len == 0) return HRS_OK;
  if (!crc_out) return fail(c, HRS_EINVAL, "crc_out is NULL");
  if (!crc_arrays_apart(crc_in, crc_out, nstripes * static_cast<size_t>(c->n)))
    return fail(c, HRS_EINVAL, "crc_in and crc_out overlap (crc_out may only be crc_in itself)");
  const hrs_status st = encode_batch_host_impl(c, stripes, row_stride, stripe_stride, len, nstripes, crc_in, crc_out);
  if (st == HRS_OK) {
    DeviceGuard g(c->device);
    c->last_host_path =
        batch_path(g.ok && runtime_pinned(stripes, batch_span(nstripes, stripe_stride, c->n, row_stride, len)));
  }
  return st;
}

hrs_status hrs_decode_batch_host_multi(hrs_codec* const* codecs, int ncodecs, const uint8_t* stripes,
                                       size_t row_stride, size_t stripe_stride, const int* erased, int max_erased,
                                       uint8_t* out, size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                       size_t nstripes) {
  hrs_status st = check_device_set(codecs, ncodecs);
  if (st != HRS_OK) return st;
  if (!stripes || !out || max_erased < 0 || max_erased > hrs::kMaxOut || (max_erased > 0 && !erased))
    return fail(codecs[0], HRS_EINVAL, "bad batch decode arguments (max_erased must be in [0, %d])", hrs::kMaxOut);
  if (nstripes == 0 || len == 0 || max_erased == 0) return HRS_OK;
  return run_device_set(codecs, ncodecs, nstripes, [&](hrs_codec* c, size_t s0, size_t ns) {
    return hrs_decode_batch_host(c, stripes + s0 * stripe_stride, row_stride, stripe_stride,
                                 erased + s0 * static_cast<size_t>(max_erased), max_erased,
                                 out + s0 * out_stripe_stride, out_row_stride, out_stripe_stride, len, ns);
  });
}

hrs_status hrs_encode_batch_host_multi(hrs_codec* const* codecs, int ncodecs, uint8_t* stripes, size_t row_stride,
                                       size_t stripe_stride, size_t len, size_t nstripes) {
  hrs_status st = check_device_set(codecs, ncodecs);
  if (st != HRS_OK) return st;
  if (!stripes) return fail(codecs[0], HRS_EINVAL, "stripes is NULL");
  if (nstripes == 0 || len == 0) return HRS_OK;
  return run_device_set(codecs, ncodecs, nstripes, [&](hrs_codec* c, size_t s0, size_t ns) {
    return hrs_encode_batch_host(c, stripes + s0 * stripe_stride, row_stride, stripe_stride, len, ns);
  });
}

}  // extern "C"
