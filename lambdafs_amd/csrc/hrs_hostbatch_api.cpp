// Host-memory batches (hrs_decode_batch_host, hrs_encode_batch_host, the
// scrub / heal / heal-erased host batches, each with its block-CRC-32 form,
// the ragged scrub and heal hrs_scrub_ragged_batch_host / hrs_heal_ragged_batch_host,
// the ragged encodes hrs_encode_ragged_batch_host[_crc] and the ragged repairs
// hrs_decode_batch_ragged_host[_crc]):
// memory classification and the zero-copy knobs, the chunk pipeline (chunks of
// stripes through a ring of device slots, H2D of exactly the rows read, D2H of
// exactly the rows written), its three jobs, and the device sets. The repair
// batch a decode chunk runs is hrs_batch_api.cpp's run_batch.
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hrs.h"
#include "hrs_codec.hpp"
#include "hrs_host.hpp"
#include "hrs_internal.hpp"
#include "hrs_launch.hpp"
#include "hrs_scrub_ragged.hpp"

namespace hrs::api {

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

}  // namespace hrs::api

using namespace hrs::api;

namespace {

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

// H2D and D2H on each slot's stream behind and ahead of its kernels (the
// default, the round-3 pipeline), or on their own streams, one per direction,
// shared by the slots (HRS_HBATCH_DUPLEX=1, kept for A/B runs; read per call so
// one process can interleave both: tools/bench_hbatch.py).
bool hbatch_duplex() {
  const char* e = getenv("HRS_HBATCH_DUPLEX");
  return e && e[0] == '1';
}

// ------------------------------------------------ the chunk pipeline
// Stripes start and end in host memory (DataNode sockets, local block files).
// Chunks of stripes flow through a ring of device slots: H2D of exactly the
// rows the chunk's codes read -> kernel (on the slot's stream) -> D2H of
// exactly the rows they write, chained by events, so one chunk's D2H overlaps
// the next chunks' H2D on the full-duplex link. Pinned caller buffers are
// DMA'd directly and the whole job is queued before the host waits once;
// pageable ones go through each slot's pinned staging (copy pool), the host
// then waits for a slot before refilling it.

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
  auto idle = [&] {  // before a buffer of the slot is freed
    for (hipStream_t s : {c->hbatch_in, c->hbatch_out, h.stream}) (void)hipStreamSynchronize(s);
  };
  if (h.dev_bytes < dev_bytes) {
    idle();
    if (h.dev) (void)hipFree(h.dev);
    h.dev = nullptr;
    h.dev_bytes = 0;
    hipError_t e = hipMalloc(&h.dev, dev_bytes);
    if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipMalloc(%zu): %s", dev_bytes, hipGetErrorString(e));
    h.dev_bytes = dev_bytes;
  }
  if (h.pin_bytes < pin_bytes) {
    idle();
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

// `cnt` rows of len bytes across the link on s, `dpitch` apart on the device
// and `hrow` apart on the host: one copy when the rows are packed on both sides.
hrs_status copy_rows(hrs_codec* c, void* dst, const void* src, size_t hrow, size_t dpitch, size_t len, int cnt,
                     hipMemcpyKind kind, hipStream_t s) {
  if (cnt <= 0) return HRS_OK;
  const bool h2d = kind == hipMemcpyHostToDevice;
  hipError_t e;
  if (cnt == 1 || (hrow == len && dpitch == len))
    e = hipMemcpyAsync(dst, src, (cnt - 1) * dpitch + len, kind, s);
  else
    e = hipMemcpy2DAsync(dst, h2d ? dpitch : hrow, src, h2d ? hrow : dpitch, len, cnt, kind, s);
  return e == hipSuccess ? HRS_OK : hip_fail(c, e, h2d ? "H2D" : "D2H");
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

// One chunk [s0, s0 + ns) as its kernels see it, on the slot's stream hs: stripe
// s0 + i's row l at img + i * img_stripe + l * pitch, its output t at
// out + i * out_stripe + t * pitch.
struct Chunk {
  hipStream_t hs;
  size_t s0, ns;
  uint8_t* img;
  size_t img_stripe, pitch;
  uint8_t* out;
  size_t out_stripe;
};

struct DirtyCell {
  size_t i;
  int l;
};

// A whole job for host_batch. Host stripe s: its img_rows rows at
// hin + s * in_stripe + l * in_row; outputs at hout + s * out_stripe +
// t * out_row. out_rows_max may be 0 (the scrub reads only): no output block,
// nothing copied back, hout not touched. Per chunk: reads(s) lists the row runs
// stripe s needs on the device, compute queues the kernels on the chunk's
// stream, writes(s) = how many output rows stripe s has (rows 0.. of its
// output block).
// dirty (optional; the heal): for jobs whose kernels write into the image.
// Once a chunk's kernels have finished, dirty(s0, ns, cells) lists the cells
// (stripe index in the chunk, location) they changed; exactly those go back
// from the slot's image to the caller's rows at hin, before the slot is
// refilled: out of the pinned staging through the copy pool (zero copy), or
// with a synchronous D2H out of the device image (copy engines; a rare path).
struct HostJob {
  const uint8_t* hin;
  size_t in_row, in_stripe;
  int img_rows;
  uint8_t* hout;
  size_t out_row, out_stripe;
  int out_rows_max;
  size_t len, nstripes;
  std::function<const std::vector<RowRun>&(size_t)> reads;
  std::function<hrs_status(const Chunk&)> compute;
  std::function<int(size_t)> writes;
  std::function<hrs_status(size_t, size_t, std::vector<DirtyCell>&)> dirty;
  // (optional; the ragged calls) in_bytes(s, l): the leading bytes of cell l of
  // stripe s that are copied in, and copied back when the cell is dirty.
  std::function<size_t(size_t, int)> in_bytes;
  // (optional; the ragged repair) out_bytes(s, t): the leading bytes of output
  // t of stripe s that go back to the caller; 0 skips the copy.
  std::function<size_t(size_t, int)> out_bytes;
};

hrs_status host_batch(hrs_codec* c, const HostJob& job) {
  const uint8_t* const hin = job.hin;
  uint8_t* const hout = job.hout;
  const size_t len = job.len, nstripes = job.nstripes;
  const bool has_dirty = static_cast<bool>(job.dirty);
  const bool ragged = static_cast<bool>(job.in_bytes);
  const bool ragged_out = static_cast<bool>(job.out_bytes);
  const size_t dpitch = (len + 255) & ~static_cast<size_t>(255);
  const size_t img_stripe = dpitch * static_cast<size_t>(job.img_rows);
  const size_t out_stripe_dev = dpitch * static_cast<size_t>(job.out_rows_max);
  size_t chunk = std::max<size_t>(1, hbatch_target_bytes() / std::max<size_t>(1, img_stripe));
  chunk = std::min(chunk, nstripes);
  const bool pinned =
      runtime_pinned(hin, batch_span(nstripes, job.in_stripe, job.img_rows, job.in_row, len)) &&
      (job.out_rows_max == 0 ||
       runtime_pinned(hout, batch_span(nstripes, job.out_stripe, job.out_rows_max, job.out_row, len)));
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
        for (int t = 0, nw = job.writes(s); t < nw; ++t) {
          const size_t nb = ragged_out ? job.out_bytes(s, t) : len;
          if (nb == 0) continue;
          jobs.push_back({hout + s * job.out_stripe + t * job.out_row, pout + i * out_stripe_dev + t * dpitch, nb});
        }
      }
    }
    if (has_dirty) {
      cells.clear();
      hrs_status st = job.dirty(pend[sl].s0, pend[sl].ns, cells);
      if (st != HRS_OK) return st;
      for (const DirtyCell& d : cells) {
        uint8_t* dst = const_cast<uint8_t*>(hin) + (pend[sl].s0 + d.i) * job.in_stripe + d.l * job.in_row;
        const size_t at = d.i * img_stripe + d.l * dpitch;
        const size_t nb = ragged ? job.in_bytes(pend[sl].s0 + d.i, d.l) : len;  // a ragged cell: its leading bytes
        if (nb == 0) continue;
        if (zc) {
          jobs.push_back({dst, h.pin + at, nb});
        } else if ((e = hipMemcpy(dst, h.dev + at, nb, hipMemcpyDeviceToHost)) != hipSuccess) {
          return hip_fail(c, e, "D2H of a healed cell");
        }
      }
    }
    pend[sl].busy = false;
    return HRS_OK;
  };
  // the copy engines' chunk: H2D, kernels, D2H, each on its stage's stream; in
  // duplex mode the H2D waits until the slot's previous kernels have read its
  // image, the kernels until the previous D2H has read its output block, the
  // D2H until this chunk's kernels. Leaves the stream the chunk ends on in *last.
  auto engines = [&](int sl, size_t s0, size_t ns, hipStream_t* last) -> hrs_status {
    hrs_codec::HostBatchSlot& h = c->hbatch[sl];
    hipError_t e = hipSuccess;
    const hipStream_t s_in = duplex ? c->hbatch_in : h.stream;
    const hipStream_t s_out = *last = duplex ? c->hbatch_out : h.stream;
    if (duplex && pend[sl].used && (e = hipStreamWaitEvent(s_in, h.comp_done, 0)) != hipSuccess)
      return hip_fail(c, e, "hipStreamWaitEvent");
    uint8_t* dimg = h.dev;
    uint8_t* dout = h.dev + chunk * img_stripe;
    const size_t hrow = pinned ? job.in_row : dpitch;  // the caller's rows, or their copy in staging
    for (size_t i = 0; i < ns; ++i) {
      const uint8_t* src = pinned ? hin + (s0 + i) * job.in_stripe : h.pin + i * img_stripe;
      for (const RowRun& r : job.reads(s0 + i)) {
        if (!ragged) {
          hrs_status st = copy_rows(c, dimg + i * img_stripe + r.l0 * dpitch, src + r.l0 * hrow, hrow, dpitch, len,
                                    r.cnt, hipMemcpyHostToDevice, s_in);
          if (st != HRS_OK) return st;
          continue;
        }
        for (int l = r.l0; l < r.l0 + r.cnt; ++l) {  // cell by cell, its leading bytes only
          const size_t nb = job.in_bytes(s0 + i, l);
          if (nb == 0) continue;
          hrs_status st = copy_rows(c, dimg + i * img_stripe + l * dpitch, src + l * hrow, hrow, dpitch, nb, 1,
                                    hipMemcpyHostToDevice, s_in);
          if (st != HRS_OK) return st;
        }
      }
    }
    if (duplex) {
      if ((e = hipEventRecord(h.in_done, s_in)) != hipSuccess) return hip_fail(c, e, "hipEventRecord");
      if ((e = hipStreamWaitEvent(h.stream, h.in_done, 0)) != hipSuccess) return hip_fail(c, e, "hipStreamWaitEvent");
      if (pend[sl].used && (e = hipStreamWaitEvent(h.stream, h.done, 0)) != hipSuccess)
        return hip_fail(c, e, "hipStreamWaitEvent");
    }
    hrs_status st = job.compute({h.stream, s0, ns, dimg, img_stripe, dpitch, dout, out_stripe_dev});
    if (st != HRS_OK) return st;
    if (duplex) {
      if ((e = hipEventRecord(h.comp_done, h.stream)) != hipSuccess) return hip_fail(c, e, "hipEventRecord");
      if ((e = hipStreamWaitEvent(s_out, h.comp_done, 0)) != hipSuccess) return hip_fail(c, e, "hipStreamWaitEvent");
    }
    for (size_t i = 0; i < ns; ++i) {
      const size_t s = s0 + i;
      uint8_t* dst = pinned ? hout + s * job.out_stripe : h.pin + chunk * img_stripe + i * out_stripe_dev;
      const size_t hrow_out = pinned ? job.out_row : dpitch;
      if (!ragged_out) {
        st = copy_rows(c, dst, dout + i * out_stripe_dev, hrow_out, dpitch, len, job.writes(s), hipMemcpyDeviceToHost,
                       s_out);
        if (st != HRS_OK) return st;
        continue;
      }
      for (int t = 0, nw = job.writes(s); t < nw; ++t) {  // cell by cell, its leading bytes only
        const size_t nb = job.out_bytes(s, t);
        if (nb == 0) continue;
        st = copy_rows(c, dst + t * hrow_out, dout + i * out_stripe_dev + t * dpitch, hrow_out, dpitch, nb, 1,
                       hipMemcpyDeviceToHost, s_out);
        if (st != HRS_OK) return st;
      }
    }
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
        for (const RowRun& r : job.reads(s0 + i))
          for (int q = 0; q < r.cnt; ++q) {
            const int l = r.l0 + q;
            const size_t nb = ragged ? job.in_bytes(s0 + i, l) : len;
            if (nb == 0) continue;
            jobs.push_back(
                {h.pin + i * img_stripe + l * dpitch, hin + (s0 + i) * job.in_stripe + l * job.in_row, nb, nt});
          }
      pool.run(jobs);
    }
    hipStream_t last = h.stream;
    const hrs_status st =
        zc ? job.compute({h.stream, s0, ns, zc_img[sl], img_stripe, dpitch, zc_img[sl] + chunk * img_stripe,
                          out_stripe_dev})  // the kernels work on the staging itself
           : engines(sl, s0, ns, &last);
    if (st != HRS_OK) return st;
    const hipError_t e = hipEventRecord(h.done, last);
    if (e != hipSuccess) return hip_fail(c, e, "hipEventRecord");
    pend[sl].busy = pend[sl].used = true;
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

// A pinned batch in one call: on slot 0's stream, its grid capped (the host
// link bounds it), the caller's launches run and the call waits for them.
template <typename Launch>
hrs_status zero_copy_call(hrs_codec* c, Launch launch) {
  hrs_status st = hbatch_slot(c, 0, 0, 0);
  if (st != HRS_OK) return st;
  const hipStream_t hs = c->hbatch[0].stream;
  {
    hrs::GridCap cap(zero_copy_blocks());
    st = launch(hs);
  }
  if (st != HRS_OK) return st;
  const hipError_t e = hipStreamSynchronize(hs);
  return e == hipSuccess ? HRS_OK : hip_fail(c, e, "hipStreamSynchronize");
}

// A grow-only device buffer of the handle. Every earlier batch that used it
// has completed: the calls are synchronous.
hrs_status grow_words(hrs_codec* c, uint32_t** buf, size_t* have, size_t bytes) {
  if (*have >= bytes) return HRS_OK;
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *have = 0;
  const hipError_t e = hipMalloc(buf, bytes);
  if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
  *have = bytes;
  return HRS_OK;
}

// The CRCs of a host batch (HOST arrays of n words; crc_out NULL: none asked
// for). A job that computes them on the device calls on_device first: they
// accumulate in the handle's device buffer, filled from crc_in, written by the
// slot streams' folds at in(at) / out(at), and come back in one copy (fetch)
// after the last chunk.
struct HostCrcs {
  hrs_codec* c;
  size_t n;
  const uint32_t* crc_in;
  uint32_t* crc_out;
  bool device = false;
  explicit operator bool() const { return crc_out != nullptr; }
  hrs_status on_device() {
    if (!crc_out) return HRS_OK;
    const hrs_status st = grow_words(c, &c->hbatch_crc, &c->hbatch_crc_bytes, n * sizeof(uint32_t));
    if (st != HRS_OK) return st;
    device = true;
    if (!crc_in) return HRS_OK;
    const hipError_t e = hipMemcpy(c->hbatch_crc, crc_in, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    return e == hipSuccess ? HRS_OK : hip_fail(c, e, "hipMemcpy crc_in");
  }
  const uint32_t* in(size_t at) const { return crc_in ? c->hbatch_crc + at : nullptr; }
  uint32_t* out(size_t at) const { return crc_out ? c->hbatch_crc + at : nullptr; }
  hrs_status fetch() const {
    if (!device) return HRS_OK;
    const hipError_t e = hipMemcpy(crc_out, c->hbatch_crc, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? HRS_OK : hip_fail(c, e, "hipMemcpy crc_out");
  }
};

// Every host batch from the device to its end: job(crcs) under the handle's
// device; a failed one may leave slot work in flight, so every slot stream is
// drained; a good one fetches its CRCs and names its path for
// hrs_last_host_path: "copy_engine" when zero copy is off, else "pinned" when
// the stripes' span (and a decode's outputs': out != NULL) is runtime-pinned,
// else "staged". needs_device == false: a job with nothing to launch, which a
// host-only handle answers too.
template <typename Job>
hrs_status host_batch_call(hrs_codec* c, const void* stripes, size_t span, const void* out, size_t out_span,
                           HostCrcs crcs, bool needs_device, Job job) {
  DeviceGuard g(c->device);
  if (!g.ok && needs_device) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  const bool pinned = g.ok && runtime_pinned(stripes, span) && (!out || runtime_pinned(out, out_span));
  hrs_status st = job(crcs);
  if (st != HRS_OK) {
    for (hipStream_t s : {c->hbatch_in, c->hbatch_out})
      if (s) (void)hipStreamSynchronize(s);
    for (auto& h : c->hbatch)
      if (h.stream) (void)hipStreamSynchronize(h.stream);
    return st;
  }
  if ((st = crcs.fetch()) != HRS_OK) return st;
  c->last_host_path = !zero_copy_on() ? "copy_engine" : pinned ? "pinned" : "staged";
  return HRS_OK;
}

// hrs_decode_batch_host and hrs_decode_batch_host_crc (with_crc; HOST arrays
// of nstripes * max_erased words). Pinned stripes and outputs: one batch launch
// whose kernels read the survivors and write the repaired cells across the
// host link directly (zero copy), the plans going up first on the same stream.
// The batch after its argument rules, its plans built. valid != NULL
// (hrs_decode_batch_ragged_host; with_crc too: hrs_decode_batch_ragged_host_crc,
// each CRC over exactly its cell's length): cell l of stripe s holds valid[s * n + l]
// leading bytes; the length table goes up with the plans, a staged chunk
// copies in only those bytes of each survivor and copies back only those of
// each output, and what the slot images keep behind them the ragged kernels
// neither read into an output nor overwrite.
hrs_status decode_batch_host_run(hrs_codec* c, const BatchGeom& g, const int* erased, int max_erased, size_t nstripes,
                                 BatchPlanSet& ps, bool with_crc, const uint32_t* crc_in, uint32_t* crc_out,
                                 const uint32_t* valid) {
  const bool ragged = valid != nullptr;
  const size_t n = static_cast<size_t>(c->n);
  const size_t len = g.len, ncrc = nstripes * static_cast<size_t>(max_erased);
  const size_t span = batch_span(nstripes, g.stripe_stride, c->n, g.row_stride, len);
  const size_t out_span = batch_span(nstripes, g.out_stripe_stride, max_erased, g.out_row_stride, len);
  auto job = [&](HostCrcs& crcs) -> hrs_status {
    if (ps.max_nout == 0) {  // nothing lost anywhere: every CRC continues over no bytes
      if (crc_out && crc_in) std::memmove(crc_out, crc_in, ncrc * sizeof(uint32_t));
      else if (crc_out) std::memset(crc_out, 0, ncrc * sizeof(uint32_t));
      return HRS_OK;
    }
    hrs_status st = crcs.on_device();
    if (st != HRS_OK) return st;
    // stripes [s0, s0 + ns) at `at` on hs, with their CRCs when asked
    auto repair = [&](const BatchGeom& at, size_t s0, size_t ns, hipStream_t hs) {
      const BatchCrcs bc{max_erased, crcs.in(s0 * max_erased), crcs.out(s0 * max_erased)};
      return run_batch(c, ps, at, s0, ns, crcs ? &bc : nullptr, hs, ragged);
    };
    uint8_t *zs = nullptr, *zo = nullptr;
    if (zero_copy_on() && host_device_ptr(g.stripes, span, &zs) && host_device_ptr(g.out, out_span, &zo))
      return zero_copy_call(c, [&](hipStream_t hs) {
        if ((ps.fused || crcs) && (st = upload_plans(c, ps, hs)) != HRS_OK) return st;
        st = repair({zs, g.row_stride, g.stripe_stride, zo, g.out_row_stride, g.out_stripe_stride, len}, 0, nstripes,
                    hs);
        if (ps.slot) slot_used(ps.slot, hs);
        return st;
      });
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
    if ((st = hbatch_slot(c, 0, 0, 0)) != HRS_OK) return st;
    const hipStream_t first = c->hbatch[0].stream;
    if (ps.fused || crcs) {
      if ((st = upload_plans(c, ps, first)) != HRS_OK) return st;
      slot_used(ps.slot, first);
      for (int i = 1; i < hrs::kHostBatchSlots; ++i) {
        if ((st = hbatch_slot(c, i, 0, 0)) != HRS_OK) return st;
        const hipError_t e = hipStreamWaitEvent(c->hbatch[i].stream, ps.slot->done, 0);
        if (e != hipSuccess) return hip_fail(c, e, "hipStreamWaitEvent");
      }
    }
    // the slots share the handle's raw-CRC scratch: run_batch chains its
    // uses by an event, so the slots' CRC kernels run one after another
    // (each fills the chip); their copies still overlap them
    HostJob hj{g.stripes, g.row_stride, g.stripe_stride, c->n, g.out, g.out_row_stride, g.out_stripe_stride,
               ps.max_nout, len, nstripes};
    hj.reads = [&](size_t s) -> const std::vector<RowRun>& { return pruns[ps.pat[s]]; };
    hj.writes = [&](size_t s) { return ps.plans[ps.pat[s]].nout; };
    if (ragged) {
      hj.in_bytes = [&](size_t s, int l) { return static_cast<size_t>(valid[s * n + l]); };
      hj.out_bytes = [&](size_t s, int t) { return static_cast<size_t>(valid[s * n + erased[s * max_erased + t]]); };
    }
    hj.compute = [&](const Chunk& k) {
      return repair({k.img, k.pitch, k.img_stripe, k.out, k.pitch, k.out_stripe, len}, k.s0, k.ns, k.hs);
    };
    st = host_batch(c, hj);
    if (ps.slot) slot_used(ps.slot, first);  // the plan slot is reused only after this job's kernels
    return st;
  };
  return host_batch_call(c, g.stripes, span, g.out, out_span, HostCrcs{c, ncrc, crc_in, crc_out},
                         ps.max_nout > 0 || with_crc, job);
}

hrs_status decode_batch_host_entry(hrs_codec* c, const BatchGeom& g, const int* erased, int max_erased,
                                   size_t nstripes, bool with_crc, const uint32_t* crc_in, uint32_t* crc_out) {
  bool empty = false;
  hrs_status st =
      decode_batch_args_ok(c, g, erased, max_erased, nstripes, with_crc ? kBatchWithCrc : 0u, crc_in, crc_out, &empty);
  if (st != HRS_OK || empty) return st;
  BatchPlanSet ps;
  st = build_batch_plans(c, erased, max_erased, nstripes, ps);
  if (st != HRS_OK) return st;
  return decode_batch_host_run(c, g, erased, max_erased, nstripes, ps, with_crc, crc_in, crc_out, nullptr);
}

// hrs_decode_batch_ragged_host and hrs_decode_batch_ragged_host_crc (with_crc;
// HOST arrays of nstripes * max_erased words, each CRC over exactly its cell's
// length): the rules of ragged_batch_args_ok, then the sibling's job with the
// lengths; an all-full batch in kernel modes 0 and 1 is the sibling's job.
hrs_status decode_batch_ragged_host_entry(hrs_codec* c, const BatchGeom& g, const int* erased, int max_erased,
                                          size_t nstripes, const uint32_t* valid, bool with_crc = false,
                                          const uint32_t* crc_in = nullptr, uint32_t* crc_out = nullptr) {
  if (!c) return HRS_EINVAL;
  BatchPlanSet ps;
  bool empty = false, all_full = false;
  const hrs_status st = ragged_batch_args_ok(c, g, erased, max_erased, nstripes, valid, ps, &empty, &all_full,
                                             with_crc ? kBatchWithCrc : 0u, crc_in, crc_out);
  if (st != HRS_OK || empty) return st;
  const bool ragged = ps.max_nout > 0 && !ragged_batch_takes_plain(c, all_full);
  if (ragged) plan_order_lengths(c, erased, max_erased, nstripes, valid, ps);
  return decode_batch_host_run(c, g, erased, max_erased, nstripes, ps, with_crc, crc_in, crc_out,
                               ragged ? valid : nullptr);
}

// The argument rules of the encode batches, in this order: the handle (NULL:
// HRS_EINVAL, no message), stripes, the empty batch (*empty = true: return
// HRS_OK and touch nothing), then with_crc: crc_args_ok over nstripes * n words.
hrs_status encode_batch_args_ok(hrs_codec* c, const uint8_t* stripes, size_t len, size_t nstripes, bool with_crc,
                                const uint32_t* crc_in, const uint32_t* crc_out, bool* empty) {
  *empty = false;
  if (!c) return HRS_EINVAL;
  if (!stripes) return fail(c, HRS_EINVAL, "stripes is NULL");
  if (nstripes == 0 || len == 0) {
    *empty = true;
    return HRS_OK;
  }
  return with_crc ? crc_args_ok(c, crc_in, crc_out, nstripes * static_cast<size_t>(c->n)) : HRS_OK;
}

// hrs_encode_batch_host and hrs_encode_batch_host_crc (with_crc; HOST arrays
// of nstripes * n words: encode_crc_impl instead of run_apply). The parity
// rows 0..p-1 of each stripe are written in place.
hrs_status encode_batch_host_entry(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride, size_t len,
                                   size_t nstripes, bool with_crc, const uint32_t* crc_in, uint32_t* crc_out) {
  bool empty = false;
  const hrs_status ok = encode_batch_args_ok(c, stripes, len, nstripes, with_crc, crc_in, crc_out, &empty);
  if (ok != HRS_OK || empty) return ok;
  const int k = c->k, p = c->p;
  const size_t n = static_cast<size_t>(c->n);
  const size_t span = batch_span(nstripes, stripe_stride, c->n, row_stride, len);
  auto job = [&](HostCrcs& crcs) -> hrs_status {
    hrs_status st = crcs.on_device();
    if (st != HRS_OK) return st;
    std::vector<const uint8_t*> in(k);
    std::vector<uint8_t*> outp(p);
    // stripes [s0, s0 + ns) on hs: the data rows p.. of `img` (rows `row`
    // apart) into the parity rows 0.. at `par`; with CRCs the raw scratch is
    // chained across the slot streams
    auto encode = [&](hipStream_t hs, size_t s0, size_t ns, const uint8_t* img, size_t row, size_t img_stride,
                      uint8_t* par, size_t par_stride) -> hrs_status {
      for (int i = 0; i < k; ++i) in[i] = img + static_cast<size_t>(p + i) * row;
      for (int r = 0; r < p; ++r) outp[r] = par + static_cast<size_t>(r) * row;
      if (!crcs)
        return run_apply(c, c->g.data(), p, k, in.data(), img_stride, outp.data(), par_stride, len, ns, hs,
                         static_encode_family(c));
      return with_crc_scratch(c, crc_raw_bytes_for(len, ns, c->n), hs, [&] {
        return encode_crc_impl(c, in.data(), img_stride, outp.data(), par_stride, len, ns, crcs.in(s0 * n),
                               crcs.out(s0 * n), hs, c->crc_raw);
      });
    };
    uint8_t* zs = nullptr;
    if (zero_copy_on() && host_device_ptr(stripes, span, &zs))  // the kernel works on the caller's stripes in place
      return zero_copy_call(
          c, [&](hipStream_t hs) { return encode(hs, 0, nstripes, zs, row_stride, stripe_stride, zs, stripe_stride); });
    const std::vector<RowRun> data_rows{{p, k}};  // hops locations p..n-1: one run
    HostJob hj{stripes, row_stride, stripe_stride, c->n, stripes, row_stride, stripe_stride, p, len, nstripes};
    hj.reads = [&](size_t) -> const std::vector<RowRun>& { return data_rows; };
    hj.writes = [&](size_t) { return p; };
    hj.compute = [&](const Chunk& q) {
      return encode(q.hs, q.s0, q.ns, q.img, q.pitch, q.img_stripe, q.out, q.out_stripe);
    };
    return host_batch(c, hj);
  };
  return host_batch_call(c, stripes, span, nullptr, 0, HostCrcs{c, nstripes * n, crc_in, crc_out}, true, job);
}

// hrs_encode_ragged_batch_host and hrs_encode_ragged_batch_host_crc (with_crc;
// HOST arrays of nstripes * n words: encode_ragged_crc_impl instead of
// run_ragged): hrs_encode_batch_host over data cells of which only the leading
// valid[s * k + j] bytes hold data (HOST words; include/hrs.h "ragged
// encode"). The words go up once through a batch slot, on the one launch's
// stream (pinned) or on slot 0's with the other slot streams waiting for it
// (staged); a staged chunk copies in only those bytes of each cell, and what
// the slot image keeps behind them reaches neither parity nor CRC.
hrs_status encode_ragged_batch_host_entry(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                          size_t len, size_t nstripes, const uint32_t* valid, bool with_crc,
                                          const uint32_t* crc_in, uint32_t* crc_out) {
  if (!c) return HRS_EINVAL;
  if (!stripes || !valid) return fail(c, HRS_EINVAL, "stripes or valid is NULL");
  if (with_crc && !crc_out) return fail(c, HRS_EINVAL, "crc_out is NULL");
  if (nstripes == 0 || len == 0) return HRS_OK;
  bool all_full = false;
  hrs_status ok = ragged_valid_ok(c, valid, len, nstripes, &all_full);
  if (ok != HRS_OK) return ok;
  const size_t n = static_cast<size_t>(c->n);
  if (with_crc && (ok = crc_args_ok(c, crc_in, crc_out, nstripes * n)) != HRS_OK) return ok;
  if (with_crc ? ragged_crc_takes_plain(c, all_full) : ragged_takes_plain(c, all_full))
    return encode_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, with_crc, crc_in, crc_out);
  const int k = c->k, p = c->p;
  const size_t span = batch_span(nstripes, stripe_stride, c->n, row_stride, len);
  const size_t valid_bytes = nstripes * static_cast<size_t>(k) * sizeof(uint32_t);
  auto job = [&](HostCrcs& crcs) -> hrs_status {
    hrs_status st = crcs.on_device();
    if (st != HRS_OK) return st;
    std::vector<const uint8_t*> in(k);
    std::vector<uint8_t*> outp(p);
    hrs_codec::BatchSlot* slot = nullptr;
    // stripes [s0, s0 + ns) on hs, laid out as for encode_batch_host_entry's
    // encode, with the chunk's slice of the valid words and of the CRC arrays
    auto encode = [&](hipStream_t hs, size_t s0, size_t ns, const uint8_t* img, size_t row, size_t img_stride,
                      uint8_t* par, size_t par_stride) -> hrs_status {
      for (int i = 0; i < k; ++i) in[i] = img + static_cast<size_t>(p + i) * row;
      for (int r = 0; r < p; ++r) outp[r] = par + static_cast<size_t>(r) * row;
      const uint32_t* dvalid = reinterpret_cast<const uint32_t*>(slot->dev) + s0 * static_cast<size_t>(k);
      if (!crcs) return run_ragged(c, in.data(), img_stride, outp.data(), par_stride, len, ns, dvalid, hs);
      return with_crc_scratch(c, crc_raw_bytes_for(len, ns, c->n), hs, [&] {
        return encode_ragged_crc_impl(c, in.data(), img_stride, outp.data(), par_stride, len, ns, dvalid,
                                      crcs.in(s0 * n), crcs.out(s0 * n), hs, c->crc_raw);
      });
    };
    uint8_t* zs = nullptr;
    if (zero_copy_on() && host_device_ptr(stripes, span, &zs))  // in place, dead windows never cross the link
      return zero_copy_call(c, [&](hipStream_t hs) {
        hrs_status st = upload(c, valid, valid_bytes, valid, 0, hs, &slot);
        if (st != HRS_OK) return st;
        st = encode(hs, 0, nstripes, zs, row_stride, stripe_stride, zs, stripe_stride);
        slot_used(slot, hs);
        return st;
      });
    if ((st = hbatch_slot(c, 0, 0, 0)) != HRS_OK) return st;
    const hipStream_t first = c->hbatch[0].stream;
    if ((st = upload(c, valid, valid_bytes, valid, 0, first, &slot)) != HRS_OK) return st;
    slot_used(slot, first);
    for (int i = 1; i < hrs::kHostBatchSlots; ++i) {
      if ((st = hbatch_slot(c, i, 0, 0)) != HRS_OK) return st;
      const hipError_t e = hipStreamWaitEvent(c->hbatch[i].stream, slot->done, 0);
      if (e != hipSuccess) return hip_fail(c, e, "hipStreamWaitEvent");
    }
    const std::vector<RowRun> data_rows{{p, k}};
    HostJob hj{stripes, row_stride, stripe_stride, c->n, stripes, row_stride, stripe_stride, p, len, nstripes};
    hj.reads = [&](size_t) -> const std::vector<RowRun>& { return data_rows; };
    hj.writes = [&](size_t) { return p; };
    hj.in_bytes = [&](size_t s, int l) { return static_cast<size_t>(valid[s * static_cast<size_t>(k) + (l - p)]); };
    hj.compute = [&](const Chunk& q) {
      return encode(q.hs, q.s0, q.ns, q.img, q.pitch, q.img_stripe, q.out, q.out_stripe);
    };
    st = host_batch(c, hj);
    slot_used(slot, first);  // the table's slot is reused only after this job's kernels
    return st;
  };
  const HostCrcs crcs{c, nstripes * n, crc_in, with_crc ? crc_out : nullptr};
  return host_batch_call(c, stripes, span, nullptr, 0, crcs, true, job);
}

// hrs_scrub_batch_host: every stripe's n rows are its reads, there are no
// output rows; the reports accumulate in the handle's device buffer (dense,
// 4 + n words per stripe) and come back in one copy.
// heal (hrs_heal_batch_host): the heal kernels, which patch the image they
// read. Pinned stripes are patched in place across the link; a staged chunk's
// reports are fetched when its kernels have finished and the cells with a
// nonzero count in word 4 + l go back to the caller (host_batch's dirty hook).
// crcs (hrs_scrub_batch_host_crc, hrs_heal_batch_host_crc; nstripes * n words,
// hops order): run_scrub_crc instead of run_scrub. A pinned cell crosses the
// link once when the shape takes the one-pass kernel (the heal's dirty windows
// twice).
// es != NULL (hrs_heal_erased_batch_host[_crc]; heal is set): run_heal_erased
// / run_heal_erased_crc with each chunk's slice of pattern indices, uploaded
// with the table through a batch slot on the chunk's stream (two slots:
// acquiring one waits for the chunk that used it two chunks earlier). A
// stripe's erased cells are never read, so a staged chunk copies in only the
// survivor rows (the slot image keeps stale bytes at erased rows; the kernels
// write every byte of them) and copies back the erased cells plus the cells
// with a nonzero count in word 4 + l.
// valid != NULL (hrs_scrub_ragged_batch_host, hrs_heal_ragged_batch_host; no
// CRCs, no erasures): cell l of stripe s holds valid[s * n + l] leading bytes.
// The length table goes up once through a batch slot, on the one launch's
// stream (pinned) or on slot 0's with the other slot streams waiting for it
// (staged); run_scrub_ragged takes each chunk's slice of it. A staged chunk
// copies in only those bytes of each cell and copies back only those of a
// dirty one; what the slot image keeps behind them the ragged kernels mask.
hrs_status scrub_batch_host_job(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                size_t len, size_t nstripes, uint32_t* reports, size_t report_stride, bool heal,
                                HostCrcs& crcs, const ErasedSets* es, const uint32_t* valid = nullptr) {
  const int n = c->n;
  const size_t lwords = hrs::scrub_ragged_words(n);
  hrs_codec::BatchSlot* lslot = nullptr;
  const uint32_t* dlens = nullptr;
  hrs_status st = crcs.on_device();
  if (st != HRS_OK) return st;
  const size_t nwords = static_cast<size_t>(hrs::kScrubHead + n);
  const size_t bytes = nstripes * nwords * sizeof(uint32_t);
  if ((st = grow_words(c, &c->scrub_reports, &c->scrub_reports_bytes, bytes)) != HRS_OK) return st;
  uint32_t* drep = c->scrub_reports;
  std::vector<const uint8_t*> rows(n);
  // the scrub or heal of stripes [s0, s0 + ns) on hs, rows `pitch` apart from img, with their CRCs when asked
  auto scrub = [&](hipStream_t hs, size_t s0, size_t ns, const uint8_t* img, size_t pitch, size_t stride) {
    for (int l = 0; l < n; ++l) rows[l] = img + static_cast<size_t>(l) * pitch;
    const uint8_t* const* r = rows.data();
    uint32_t* rep = drep + s0 * nwords;
    if (valid) return run_scrub_ragged(c, r, stride, len, ns, dlens + s0 * lwords, rep, nwords, hs, heal);
    if (es) {
      uint8_t* const* w = reinterpret_cast<uint8_t* const*>(const_cast<uint8_t**>(r));
      if (!crcs) return run_heal_erased(c, w, stride, len, ns, es->pats, es->pat.data() + s0, rep, nwords, hs);
      return run_heal_erased_crc(c, w, stride, len, ns, es->pats, es->pat.data() + s0, rep, nwords, crcs.in(s0 * n),
                                 crcs.out(s0 * n), hs, on_host(r[0]));
    }
    if (!crcs) return run_scrub(c, r, stride, len, ns, rep, nwords, hs, heal);
    return run_scrub_crc(c, r, stride, len, ns, rep, nwords, crcs.in(s0 * n), crcs.out(s0 * n), hs, heal);
  };
  uint8_t* zs = nullptr;
  if (zero_copy_on() && host_device_ptr(stripes, batch_span(nstripes, stripe_stride, n, row_stride, len), &zs)) {
    // runtime-pinned: one launch reads the caller's stripes across the host link
    st = zero_copy_call(c, [&](hipStream_t hs) {
      if (valid && (st = scrub_ragged_table(c, valid, nstripes, hs, &lslot, &dlens)) != HRS_OK) return st;
      st = scrub(hs, 0, nstripes, zs, row_stride, stripe_stride);
      if (lslot) slot_used(lslot, hs);
      return st;
    });
  } else {
    hipStream_t first = nullptr;
    if (valid) {
      if ((st = hbatch_slot(c, 0, 0, 0)) != HRS_OK) return st;
      first = c->hbatch[0].stream;
      if ((st = scrub_ragged_table(c, valid, nstripes, first, &lslot, &dlens)) != HRS_OK) return st;
      slot_used(lslot, first);
      for (int i = 1; i < hrs::kHostBatchSlots; ++i) {
        if ((st = hbatch_slot(c, i, 0, 0)) != HRS_OK) return st;
        const hipError_t e = hipStreamWaitEvent(c->hbatch[i].stream, lslot->done, 0);
        if (e != hipSuccess) return hip_fail(c, e, "hipStreamWaitEvent");
      }
    }
    const std::vector<RowRun> all_rows{{0, n}};
    std::vector<std::vector<RowRun>> survivor_runs(es ? es->keys.size() : 0);  // per pattern
    for (size_t id = 0; id < survivor_runs.size(); ++id) {
      std::vector<int> live;
      for (int l = 0; l < n; ++l)
        if (!std::binary_search(es->keys[id].begin(), es->keys[id].end(), l)) live.push_back(l);
      survivor_runs[id] = runs_of(live.data(), static_cast<int>(live.size()));
    }
    HostJob hj{stripes, row_stride, stripe_stride, n, const_cast<uint8_t*>(stripes), row_stride, stripe_stride, 0, len,
               nstripes};
    hj.reads = [&](size_t s) -> const std::vector<RowRun>& { return es ? survivor_runs[es->pat[s]] : all_rows; };
    hj.writes = [](size_t) { return 0; };
    hj.compute = [&](const Chunk& k) { return scrub(k.hs, k.s0, k.ns, k.img, k.pitch, k.img_stripe); };
    if (valid) hj.in_bytes = [&](size_t s, int l) { return static_cast<size_t>(valid[s * static_cast<size_t>(n) + l]); };
    std::vector<uint32_t> chunk_rep;
    if (heal)
      hj.dirty = [&](size_t s0, size_t ns, std::vector<DirtyCell>& cells) -> hrs_status {
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
    st = host_batch(c, hj);
    if (lslot) slot_used(lslot, first);  // the table's slot is reused only after this job's kernels
  }
  if (st != HRS_OK) return st;
  std::vector<uint32_t> host(nstripes * nwords);
  const hipError_t e = hipMemcpy(host.data(), drep, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(c, e, "hipMemcpy reports");
  for (size_t s = 0; s < nstripes; ++s)
    std::memcpy(reports + s * report_stride, host.data() + s * nwords, nwords * sizeof(uint32_t));
  return HRS_OK;
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
  // with no error: the cells must not overlap.
  if ((st = scrub_cells_apart_ok(c, row_stride, stripe_stride, len, nstripes)) != HRS_OK) return st;
  const size_t ncrc = nstripes * static_cast<size_t>(c->n);
  if (with_crc && (st = crc_args_ok(c, crc_in, crc_out, ncrc)) != HRS_OK) return st;
  // max_erased == 0: nothing can be erased, the heal itself
  const ErasedSets* sets = with_erased && max_erased > 0 ? &es : nullptr;
  return host_batch_call(c, stripes, batch_span(nstripes, stripe_stride, c->n, row_stride, len), nullptr, 0,
                         HostCrcs{c, ncrc, crc_in, with_crc ? crc_out : nullptr}, true, [&](HostCrcs& crcs) {
                           return scrub_batch_host_job(c, stripes, row_stride, stripe_stride, len, nstripes, reports,
                                                       report_stride, heal, crcs, sets);
                         });
}

// hrs_scrub_ragged_batch_host and hrs_heal_ragged_batch_host: the rules of
// scrub_ragged_args_ok (the sibling's gate and cell-overlap rule, then valid),
// then the sibling's job with the lengths; an all-full batch in kernel modes 0
// and 1 is the sibling's job.
hrs_status scrub_ragged_batch_host_entry(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                         size_t len, size_t nstripes, const uint32_t* valid, uint32_t* reports,
                                         size_t report_stride, bool heal) {
  bool empty = false, all_full = false;
  const hrs_status st = scrub_ragged_args_ok(c, stripes, reports, report_stride, len, nstripes,
                                             kScrubWithReports | kScrubImage, row_stride, stripe_stride, valid, &empty,
                                             &all_full);
  if (st != HRS_OK || empty) return st;
  const uint32_t* lengths = scrub_ragged_takes_plain(c, all_full) ? nullptr : valid;
  return host_batch_call(c, stripes, batch_span(nstripes, stripe_stride, c->n, row_stride, len), nullptr, 0,
                         HostCrcs{c, 0, nullptr, nullptr}, true, [&](HostCrcs& crcs) {
                           return scrub_batch_host_job(c, stripes, row_stride, stripe_stride, len, nstripes, reports,
                                                       report_stride, heal, crcs, nullptr, lengths);
                         });
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

hrs_status hrs_scrub_ragged_batch_host(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                       size_t len, size_t nstripes, const uint32_t* valid, uint32_t* reports,
                                       size_t report_stride) {
  return scrub_ragged_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, valid, reports,
                                       report_stride, false);
}

hrs_status hrs_heal_ragged_batch_host(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                      size_t len, size_t nstripes, const uint32_t* valid, uint32_t* reports,
                                      size_t report_stride) {
  return scrub_ragged_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, valid, reports,
                                       report_stride, true);
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

hrs_status hrs_decode_batch_host(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                 const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                 size_t out_stripe_stride, size_t len, size_t nstripes) {
  return decode_batch_host_entry(c, {stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride, len},
                                 erased, max_erased, nstripes, false, nullptr, nullptr);
}

hrs_status hrs_decode_batch_host_crc(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                     const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                     size_t out_stripe_stride, size_t len, size_t nstripes, const uint32_t* crc_in,
                                     uint32_t* crc_out) {
  return decode_batch_host_entry(c, {stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride, len},
                                 erased, max_erased, nstripes, true, crc_in, crc_out);
}

hrs_status hrs_decode_batch_ragged_host(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                        const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                        size_t out_stripe_stride, size_t len, size_t nstripes, const uint32_t* valid) {
  return decode_batch_ragged_host_entry(
      c, {stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride, len}, erased, max_erased,
      nstripes, valid);
}

hrs_status hrs_decode_batch_ragged_host_crc(hrs_codec* c, const uint8_t* stripes, size_t row_stride,
                                            size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                            size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                            size_t nstripes, const uint32_t* valid, const uint32_t* crc_in,
                                            uint32_t* crc_out) {
  return decode_batch_ragged_host_entry(
      c, {stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride, len}, erased, max_erased,
      nstripes, valid, true, crc_in, crc_out);
}

hrs_status hrs_encode_batch_host(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride, size_t len,
                                 size_t nstripes) {
  return encode_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, false, nullptr, nullptr);
}

hrs_status hrs_encode_ragged_batch_host(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                        size_t len, size_t nstripes, const uint32_t* valid) {
  return encode_ragged_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, valid, false, nullptr,
                                        nullptr);
}

hrs_status hrs_encode_ragged_batch_host_crc(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                            size_t len, size_t nstripes, const uint32_t* valid,
                                            const uint32_t* crc_in, uint32_t* crc_out) {
  return encode_ragged_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, valid, true, crc_in,
                                        crc_out);
}

hrs_status hrs_encode_batch_host_crc(hrs_codec* c, uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                     size_t len, size_t nstripes, const uint32_t* crc_in, uint32_t* crc_out) {
  return encode_batch_host_entry(c, stripes, row_stride, stripe_stride, len, nstripes, true, crc_in, crc_out);
}

hrs_status hrs_decode_batch_host_multi(hrs_codec* const* codecs, int ncodecs, const uint8_t* stripes,
                                       size_t row_stride, size_t stripe_stride, const int* erased, int max_erased,
                                       uint8_t* out, size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                       size_t nstripes) {
  hrs_status st = check_device_set(codecs, ncodecs);
  if (st != HRS_OK) return st;
  bool empty = false;
  st = decode_batch_args_ok(codecs[0], {stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride, len},
                            erased, max_erased, nstripes, kBatchDeviceSet, nullptr, nullptr, &empty);
  if (st != HRS_OK || empty) return st;
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
  bool empty = false;
  st = encode_batch_args_ok(codecs[0], stripes, len, nstripes, false, nullptr, nullptr, &empty);
  if (st != HRS_OK || empty) return st;
  return run_device_set(codecs, ncodecs, nstripes, [&](hrs_codec* c, size_t s0, size_t ns) {
    return hrs_encode_batch_host(c, stripes + s0 * stripe_stride, row_stride, stripe_stride, len, ns);
  });
}

}  // extern "C"
