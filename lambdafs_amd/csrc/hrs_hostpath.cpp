// Host-buffer calls, the JNI path: synchronous encodeBulk / decodeBulk over
// caller rows (in place when they are pinned, else in column chunks through a
// ring of staging slots, with optional block CRC-32s chained on the host), and
// the asynchronous submit / wait / collect rounds over a ring of operation
// slots. Both go through one chunk body (stage_chunk) on a StageSlot, with one
// rule each for the live inputs, the slot layout, zero copy, the kernel choice
// and the CRC chaining; the extern "C" entry points at the end only check
// their arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/hrs.h"
#include "hrs_codec.hpp"
#include "crc32.hpp"
#include "hrs_host.hpp"
#include "hrs_internal.hpp"
#include "hrs_launch.hpp"

namespace hrs::api {

using StageSlot = hrs_codec::StageSlot;
using AsyncSlot = hrs_codec::AsyncSlot;

// ---- shared with the other host units (hrs_codec.hpp)

void free_stage_slot(StageSlot& h) {
  if (h.stream) {
    (void)hipStreamSynchronize(h.stream);
    (void)hipStreamDestroy(h.stream);
  }
  if (h.done) (void)hipEventDestroy(h.done);
  if (h.dev) (void)hipFree(h.dev);
  if (h.pin) (void)hipHostFree(h.pin);
}

// Stores of the copy-ins into the pinned staging (HRS_HOST_NT, read per
// call). The GPU reads the staging next, across the link, and the staging
// lives on the GPU's NUMA node: lines a CPU of the other socket left dirty in
// its caches make every such read a cross-socket snoop. Default ("1"):
// nontemporal stores, so the lines are in memory (RS(10,4) 1 MiB staged
// encode from the other socket 0.33-0.36 ms with cached stores, 0.28 with
// nontemporal; from the GPU's node 0.255-0.262 vs 0.264-0.269: never worse;
// profiles/r06/NOTES.md §4, r06x / r06y). "auto": nontemporal only from CPUs
// off the GPU's node; "0": cached.
uint8_t host_store_mode() {
  const char* e = getenv("HRS_HOST_NT");
  if (!e) return hrs::kStoreStream;
  if (strcmp(e, "auto") == 0) return hrs::kStoreRemote;
  return e[0] == '0' ? hrs::kStorePlain : hrs::kStoreStream;
}

// NUMA node of the handle's device: its PCI function's, from sysfs (cached).
static int device_numa_node(hrs_codec* c) {
  if (c->numa_node != -2) return c->numa_node;
  int node = -1;
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof bus, c->device) == hipSuccess) {
    for (char* q = bus; *q; ++q) *q = static_cast<char>(tolower(*q));
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    if (FILE* f = fopen(path, "r")) {
      if (fscanf(f, "%d", &node) != 1) node = -1;
      fclose(f);
    }
  } else {
    (void)hipGetLastError();
  }
  c->numa_node = node;
  return node;
}

hrs::CopyPool& copy_pool(hrs_codec* c) {
  hrs::CopyPool::set_home_node(device_numa_node(c), c->device);
  return hrs::CopyPool::instance();
}

namespace {

size_t round256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

// Sizes a staging slot: its stream and event on first use, then `bytes` of
// device rows and of pinned staging (never shrunk).
hrs_status stage_slot(hrs_codec* c, StageSlot& h, size_t bytes) {
  if (!h.stream) {
    hipError_t e = hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail(c, e, "hipStreamCreate");
    e = hipEventCreateWithFlags(&h.done, hipEventDisableTiming);
    if (e != hipSuccess) return hip_fail(c, e, "hipEventCreate");
  }
  if (h.bytes >= bytes) return HRS_OK;
  (void)hipStreamSynchronize(h.stream);
  if (h.dev) (void)hipFree(h.dev);
  if (h.pin) (void)hipHostFree(h.pin);
  h.dev = nullptr;
  h.pin = nullptr;
  h.pin_dev = nullptr;
  h.bytes = 0;
  hipError_t e = hipMalloc(&h.dev, bytes);
  if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
  e = hipHostMalloc(&h.pin, bytes, hipHostMallocDefault);
  if (e != hipSuccess) return fail(c, HRS_ENOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
  if (!host_device_ptr(h.pin, bytes, &h.pin_dev)) h.pin_dev = nullptr;  // then the calls take the copy engine
  h.bytes = bytes;
  return HRS_OK;
}

// Block checksums carried through a host-buffer call (Encoder.java:408-450,
// Decoder.java:222-229 / :645-655): kCrcEncode = CRC-32 of the k inputs then
// the p outputs (the encode matrix is c->g), kCrcOutputs = of the nout outputs.
// Each chunk's CRCs come back with its outputs and are chained on the host,
// crc = Z_len(crc) ^ crc_chunk (zlib crc32_combine), starting from `in`
// (NULL = fresh CRC32 objects).
enum HostCrcMode { kCrcNone = 0, kCrcEncode = 1, kCrcOutputs = 2 };
struct HostCrc {
  int mode = kCrcNone;
  const uint32_t* in = nullptr;
  uint32_t* out = nullptr;
};

int ncrc_for(int mode, int nin, int nout) { return mode == kCrcEncode ? nin + nout : mode == kCrcOutputs ? nout : 0; }

// One operation over rows: out = m (nout x nin) * in, checksummed as `mode` says.
struct RowOp {
  const uint8_t* m;
  int nout, nin;
  bool static_kp;
  int mode;
  int ncrc() const { return ncrc_for(mode, nin, nout); }
};

// The inputs an operation reads (those some output takes, and every one of a
// checksummed encode): slot_of[i] is input i's row in the staging (-1: not
// read), nlive their number. din / dout are the row pointers of the job in
// hand, set by whoever runs it.
struct LiveRows {
  std::vector<int> slot_of;
  int nlive = 0;
  std::vector<const uint8_t*> din;
  std::vector<uint8_t*> dout;
};

hrs_status live_inputs(hrs_codec* c, const RowOp& op, const uint8_t* const* in_rows, LiveRows& live) {
  live.slot_of.assign(op.nin, -1);
  live.nlive = 0;
  for (int i = 0; i < op.nin; ++i) {
    bool any = op.mode == kCrcEncode;  // every source is checksummed
    for (int o = 0; o < op.nout; ++o) any |= op.m[o * op.nin + i] != 0;
    if (!any) continue;
    if (!in_rows[i]) return fail(c, HRS_EINVAL, "input row %d is NULL", i);
    live.slot_of[i] = live.nlive++;
  }
  live.din.resize(op.nin);
  live.dout.resize(op.nout);
  return HRS_OK;
}

// A staging slot's layout for cells of up to `cell` bytes: nlive + nout rows
// of `pitch`, then (CRC only) the ncrc CRC words of the cell, then the raw
// window-CRC scratch.
struct StageLayout {
  size_t pitch, crc_off, raw_off, need;
  StageLayout(size_t cell, int nlive, int nout, int ncrc)
      : pitch(round256(cell)),
        crc_off(pitch * static_cast<size_t>(nlive + nout)),
        raw_off(crc_off + round256(ncrc * sizeof(uint32_t))),
        need(ncrc ? raw_off + crc_raw_bytes_for(cell, 1, ncrc) : crc_off) {}
};

// Zero copy: the kernel reads its rows from pinned host memory and writes its
// outputs (and the cell CRCs) there, across the host link — no H2D / D2H.
// Taken when it is on, the memory has a device alias, and a checksummed cell's
// kernel is one-pass (a two-pass CRC would read the cells across the link a
// second time); everything else takes the copy engine.
bool zero_copy_ok(const hrs_codec* c, const RowOp& op, int nlive, size_t len, bool have_alias) {
  if (!have_alias || !zero_copy_on()) return false;
  if (op.mode == kCrcEncode) return encode_crc_one_pass(c, len, 1);
  if (op.mode == kCrcOutputs) return apply_crc_one_pass(c, op.nout, nlive, len);
  return true;
}

// The kernels of one cell: encode + CRC, repair + CRC of the repaired cells
// (fused where the shape allows), or the plain apply.
hrs_status run_rows(hrs_codec* c, const RowOp& op, const uint8_t* const* din, uint8_t* const* dout, size_t len,
                    uint32_t* dcrc, hipStream_t s, uint32_t* raw, uint64_t* fold_win) {
  if (op.mode == kCrcEncode) return encode_crc_impl(c, din, 0, dout, 0, len, 1, nullptr, dcrc, s, raw, fold_win);
  if (op.mode == kCrcOutputs)
    return apply_crc_impl(c, op.m, op.nout, op.nin, din, 0, dout, 0, len, 1, nullptr, dcrc, s, raw, fold_win);
  return run_apply(c, op.m, op.nout, op.nin, din, 0, dout, 0, len, 1, s, op.static_kp);
}

// One cell of `len` bytes per row, already in the slot's pinned staging, on
// the slot's stream: zero copy (zc) runs the kernels on the staging; else H2D
// of the live rows -> kernels -> D2H of the outputs and the CRC words right
// behind them. fold_win != NULL (zero-copy cells only): the raw window CRCs
// go to the pinned staging and the caller folds them on the host (no fold
// launch; *fold_win as encode_crc_impl sets it); NULL: they stay in device
// memory and a fold kernel writes the CRC words.
hrs_status stage_chunk(hrs_codec* c, const RowOp& op, StageSlot& h, const StageLayout& lay, LiveRows& live, size_t len,
                       bool zc, uint64_t* fold_win) {
  // only zero-copy cells cap their grid (the link bounds them); one sent to
  // the copy engine runs on device memory with the full grid
  hrs::GridCap cap(zc ? zero_copy_blocks() : 0u);
  const int nlive = live.nlive, ncrc = op.ncrc();
  if (nlive > 0 && !zc) {
    hipError_t e = hipMemcpyAsync(h.dev, h.pin, lay.pitch * (nlive - 1) + len, hipMemcpyHostToDevice, h.stream);
    if (e != hipSuccess) return hip_fail(c, e, "hipMemcpyAsync H2D");
  }
  uint8_t* img = zc ? h.pin_dev : h.dev;
  for (int i = 0; i < op.nin; ++i) live.din[i] = live.slot_of[i] >= 0 ? img + lay.pitch * live.slot_of[i] : nullptr;
  for (int o = 0; o < op.nout; ++o) live.dout[o] = img + lay.pitch * (nlive + o);
  uint32_t* dcrc = reinterpret_cast<uint32_t*>(img + lay.crc_off);
  uint32_t* raw = reinterpret_cast<uint32_t*>((fold_win ? h.pin_dev : h.dev) + lay.raw_off);
  hrs_status st = run_rows(c, op, live.din.data(), live.dout.data(), len, dcrc, h.stream, raw, fold_win);
  if (st != HRS_OK) return st;
  if (!zc) {
    const size_t back = ncrc ? lay.crc_off + ncrc * sizeof(uint32_t) - lay.pitch * nlive
                             : lay.pitch * (op.nout - 1) + len;
    hipError_t e = hipMemcpyAsync(h.pin + lay.pitch * nlive, h.dev + lay.pitch * nlive, back, hipMemcpyDeviceToHost,
                                  h.stream);
    if (e != hipSuccess) return hip_fail(c, e, "hipMemcpyAsync D2H");
  }
  return HRS_OK;
}

const hrs::crc::Mat& crc_zmat(hrs_codec* c, uint64_t len) {
  auto it = c->crc_zmats.find(len);
  if (it == c->crc_zmats.end()) it = c->crc_zmats.emplace(len, hrs::crc::zeros(len)).first;
  return it->second;
}

// CRC32.update chaining: the n running values in `crc` continue over a cell
// of `len` bytes per row whose own CRCs are `part`.
void chain_crcs(hrs_codec* c, size_t len, uint32_t* crc, const uint32_t* part, int n) {
  if (n <= 0) return;
  const hrs::crc::Mat& z = crc_zmat(c, len);
  for (int r = 0; r < n; ++r) crc[r] = hrs::crc::apply(z, crc[r]) ^ part[r];
}

// Z_len as 4 byte-indexed tables (crc32.hpp to_tables), for host folds.
const uint32_t* crc_ztab(hrs_codec* c, uint64_t len) {
  auto it = c->crc_ztabs.find(len);
  if (it == c->crc_ztabs.end()) {
    std::vector<uint32_t> t(4 * 256);
    hrs::crc::to_tables(crc_zmat(c, len), t.data());
    it = c->crc_ztabs.emplace(len, std::move(t)).first;
  }
  return it->second.data();
}

inline uint32_t ztab_apply(const uint32_t* t, uint32_t v) {
  return t[v & 0xFFu] ^ t[256 + ((v >> 8) & 0xFFu)] ^ t[512 + ((v >> 16) & 0xFFu)] ^ t[768 + (v >> 24)];
}

// Checksummed staged chunks fold their raw window CRCs on the host
// (HRS_HOST_FOLD=0: a fold kernel per chunk, the round-5 form; read per call).
bool host_fold_on() {
  const char* e = getenv("HRS_HOST_FOLD");
  return !(e && e[0] == '0');
}

// Rows the caller holds in memory the runtime allocated pinned (hipHostMalloc,
// torch pin_memory) are visible to the GPU at their own addresses and never
// move: the zero-copy kernel runs over them in place, one launch, no staging
// copies ("pinned"). Taken when zero_copy_ok says so and every live input
// (live.din) and output row lies wholly inside such an allocation and is
// 16-byte aligned; otherwise false and nothing done.
// Pageable memory the caller registered with hipHostRegister is NOT taken
// here: registration maps the pages for the GPU without pinning them, and in
// round 5 GPU writes into registered pages were lost when a page moved during
// a kernel ("Platform constraint"). Such rows are staged.
bool host_apply_pinned(hrs_codec* c, const RowOp& op, const LiveRows& live, uint8_t* const* out_rows, size_t len,
                       uint32_t* crc, hrs_status* st) {
  if (!zero_copy_ok(c, op, live.nlive, len, true)) return false;
  auto in_place = [len](const uint8_t* p) {
    uint8_t* d = nullptr;
    return aligned16(p) && host_device_ptr(p, len, &d) && d == p;
  };
  for (int i = 0; i < op.nin; ++i)
    if (live.din[i] && !in_place(live.din[i])) return false;
  for (int o = 0; o < op.nout; ++o)
    if (!in_place(out_rows[o])) return false;
  // the cell CRC words in slot 0's pinned staging, the raw window CRCs in its device buffer
  const int ncrc = op.ncrc();
  const size_t words = static_cast<size_t>(std::max(ncrc, 1)) * sizeof(uint32_t);
  const size_t raw_off = round256(words);
  StageSlot& h = c->host[0];
  *st = stage_slot(c, h, ncrc > 0 ? raw_off + crc_raw_bytes_for(len, 1, ncrc) : words);
  if (*st != HRS_OK) return true;
  if (!h.pin_dev) return false;
  c->last_host_path = "pinned";
  {
    hrs::GridCap cap(zero_copy_blocks());
    *st = run_rows(c, op, live.din.data(), out_rows, len, reinterpret_cast<uint32_t*>(h.pin_dev), h.stream,
                   reinterpret_cast<uint32_t*>(h.dev + raw_off), nullptr);
  }
  const hipError_t e = hipStreamSynchronize(h.stream);
  if (*st == HRS_OK && e != hipSuccess) *st = hip_fail(c, e, "hipStreamSynchronize");
  if (*st == HRS_OK) chain_crcs(c, len, crc, reinterpret_cast<const uint32_t*>(h.pin), ncrc);
  return true;
}

// ---- the staged pipeline (pageable rows) ----
// The caller's rows are cut into column chunks (the first HRS_HOST_FIRST
// bytes, then HRS_HOST_CHUNK each) that rotate through a ring of S slots
// (HRS_HOST_SLOTS), each a StageSlot. Per chunk: the copy pool moves its live
// input columns into the slot's staging, stage_chunk runs it there (zero
// copy, or H2D -> kernel -> D2H with HRS_ZEROCOPY=0 and for chunks no
// one-pass kernel takes), its completion is the slot's event, and the pool
// moves its output columns out. Chunks are copied out in order as soon as
// they are done (not only when their slot is needed again), so only the last
// chunk's copy-out follows the link time; each chunk's CRC words are kept and
// chained in order at the end. (Queueing the kernels ahead of the copy-ins
// behind gate kernels was measured slower and is gone: profiles/r06/NOTES.md.)
size_t env_window_bytes(const char* name, size_t dflt) {
  const char* e = getenv(name);
  const long x = e ? atol(e) : 0;
  if (x < static_cast<long>(hrs::kWindowBytes)) return dflt;
  return static_cast<size_t>(x) / hrs::kWindowBytes * hrs::kWindowBytes;
}

// Defaults measured with tools/host_pipeline_sweep (profiles/r06/NOTES.md):
// 128 KiB x 8 slots, once the copy pool's batches stopped ending in a
// condition-variable sleep (r06q / r06r, same box, 3 copy workers; RS(10,4)
// 1 MiB calls, encode / decode / encode + CRC / decode + CRC): 0.267 / 0.245 /
// 0.283 / 0.244 ms against 0.281 / 0.248 / 0.293 / 0.255 at 256 KiB x 4 (the
// round-6 default before) and 0.314 / 0.271 / 0.348 / 0.271 at 512 KiB x 2
// (round 5); in-place floor on pinned rows 0.224 / 0.213 / 0.238 / 0.221.
size_t host_chunk_bytes() { return env_window_bytes("HRS_HOST_CHUNK", 128 << 10); }
size_t host_first_bytes(size_t chunk) { return std::min(chunk, env_window_bytes("HRS_HOST_FIRST", chunk)); }

int host_slots() {
  const char* e = getenv("HRS_HOST_SLOTS");
  const int x = e ? atoi(e) : 0;
  return (x >= 2 && x <= hrs::kHostSlots) ? x : 8;
}

hrs_status staged_run(hrs_codec* c, const RowOp& op, const uint8_t* const* in_rows, uint8_t* const* out_rows,
                      size_t len, uint32_t* crc, LiveRows& live) {
  struct Span {
    size_t off, len;
  };
  const int nin = op.nin, nout = op.nout, nlive = live.nlive, ncrc = op.ncrc();
  const size_t chunk = std::min(len, host_chunk_bytes());
  const size_t first = host_first_bytes(chunk);
  std::vector<Span> ch;
  for (size_t off = 0; off < len;) {
    const size_t l = std::min(ch.empty() ? first : chunk, len - off);
    ch.push_back({off, l});
    off += l;
  }
  const size_t C = ch.size();
  const int S = static_cast<int>(std::min<size_t>(host_slots(), C));
  const StageLayout lay(chunk, nlive, nout, ncrc);
  bool alias = true;
  for (int i = 0; i < S; ++i) {
    hrs_status st = stage_slot(c, c->host[i], lay.need);
    if (st != HRS_OK) return st;
    alias &= c->host[i].pin_dev != nullptr;
  }
  // asked once per chunk length (at most three): this runs before the first
  // copy-in, where nothing hides it
  std::vector<char> zc(C);
  bool all_zc = true;
  for (size_t j = 0; j < C; ++j) {
    zc[j] = j && ch[j].len == ch[j - 1].len ? zc[j - 1] : zero_copy_ok(c, op, nlive, ch[j].len, alias);
    all_zc &= zc[j] != 0;
  }
  c->last_host_path = all_zc ? "staged" : "copy_engine";
  hrs::CopyPool& pool = copy_pool(c);
  std::vector<hrs::CopyJob> jobs;
  std::vector<uint32_t> parts(static_cast<size_t>(ncrc) * C);
  hrs::CopyPool::Hold hold;  // the pool's workers stay awake for this call
  // Copies go to the pool as one batch per step: the outputs of every chunk
  // that is done (copy_out) and the next chunk's inputs (copy_in). A chunk's
  // input rows and output rows are disjoint regions of its slot, so a chunk's
  // copy-out and its slot's next copy-in may share a batch.
  const uint8_t nt = host_store_mode();
  auto copy_in = [&](size_t j) {
    const StageSlot& h = c->host[j % S];
    for (int i = 0; i < nin; ++i)
      if (live.slot_of[i] >= 0)
        jobs.push_back({h.pin + lay.pitch * live.slot_of[i], in_rows[i] + ch[j].off, ch[j].len, nt});
  };
  // zero-copy chunks leave their raw window CRCs in the pinned staging and
  // the host folds them at copy-out (no fold launch per chunk)
  const bool host_fold = host_fold_on();
  std::vector<uint64_t> fold_win(C, 0);  // window of a chunk whose raw CRCs the host folds (0: GPU-folded)
  auto copy_out = [&](size_t j) {
    const StageSlot& h = c->host[j % S];
    for (int o = 0; o < nout; ++o)
      jobs.push_back({out_rows[o] + ch[j].off, h.pin + lay.pitch * (nlive + o), ch[j].len});
    if (!ncrc) return;
    if (!fold_win[j]) {
      std::memcpy(&parts[j * ncrc], h.pin + lay.crc_off, ncrc * sizeof(uint32_t));
      return;
    }
    // CRC-32 of the chunk's cell of row r from its raw window CRCs
    // (crc32.hpp: raw(A || B) = Z_|B|(raw(A)) ^ raw(B); crc = Z_len(~0) ^ raw ^ ~0)
    const size_t nw = ch[j].len / fold_win[j];
    const uint32_t* zw = crc_ztab(c, fold_win[j]);
    const uint32_t* zl = crc_ztab(c, ch[j].len);
    const uint32_t* raw = reinterpret_cast<const uint32_t*>(h.pin + lay.raw_off);
    // up to 16 rows' chains advance in lockstep, so their table lookups
    // overlap (a 14-row chunk of 64 windows: 1.4-1.7 us instead of 3.7-3.9
    // row by row, on the build host)
    const uint32_t zinit = ztab_apply(zl, ~0u);
    for (int r0 = 0; r0 < ncrc; r0 += 16) {
      const int m = std::min(16, ncrc - r0);
      uint32_t x[16] = {0};
      for (size_t w = 0; w < nw; ++w)
        for (int r = 0; r < m; ++r) x[r] = ztab_apply(zw, x[r]) ^ raw[(r0 + r) * nw + w];
      for (int r = 0; r < m; ++r) parts[j * ncrc + r0 + r] = zinit ^ x[r] ^ ~0u;
    }
  };
  auto flush = [&] {
    if (!jobs.empty()) pool.run(jobs);
    jobs.clear();
  };
  auto ev = [&](size_t j) { return c->host[j % S].done; };
  size_t out_next = 0;  // chunks [0, out_next) are copied out
  for (size_t j = 0; j < C; ++j) {
    while (out_next + S <= j) {  // the slot's previous chunk must be out
      hipError_t e = hipEventSynchronize(ev(out_next));
      if (e != hipSuccess) return hip_fail(c, e, "hipEventSynchronize");
      copy_out(out_next++);
    }
    while (out_next < j && hipEventQuery(ev(out_next)) == hipSuccess) copy_out(out_next++);
    copy_in(j);
    flush();
    StageSlot& h = c->host[j % S];
    hrs_status st = stage_chunk(c, op, h, lay, live, ch[j].len, zc[j], zc[j] && host_fold ? &fold_win[j] : nullptr);
    if (st != HRS_OK) return st;
    hipError_t e = hipEventRecord(h.done, h.stream);
    if (e != hipSuccess) return hip_fail(c, e, "hipEventRecord");
  }
  while (out_next < C) {
    hipError_t e = hipEventSynchronize(ev(out_next));
    if (e != hipSuccess) return hip_fail(c, e, "hipEventSynchronize");
    copy_out(out_next++);
    while (out_next < C && hipEventQuery(ev(out_next)) == hipSuccess) copy_out(out_next++);
    flush();
  }
  for (size_t j = 0; j < C && ncrc; ++j) chain_crcs(c, ch[j].len, crc, &parts[j * ncrc], ncrc);  // in column order
  return HRS_OK;
}

hrs_status host_apply_impl(hrs_codec* c, const RowOp& op, const uint8_t* const* in_rows, uint8_t* const* out_rows,
                           size_t len, const HostCrc& crc) {
  const int ncrc = op.ncrc();
  for (int r = 0; r < ncrc; ++r) crc.out[r] = crc.in ? crc.in[r] : 0u;  // the running values; an empty call leaves them
  if (len == 0 || op.nout == 0) return HRS_OK;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  LiveRows live;
  hrs_status st = live_inputs(c, op, in_rows, live);
  if (st != HRS_OK) return st;
  for (int o = 0; o < op.nout; ++o)
    if (!out_rows[o]) return fail(c, HRS_EINVAL, "output row %d is NULL", o);
  for (int i = 0; i < op.nin; ++i) live.din[i] = live.slot_of[i] >= 0 ? in_rows[i] : nullptr;
  if (host_apply_pinned(c, op, live, out_rows, len, crc.out, &st)) return st;
  return staged_run(c, op, in_rows, out_rows, len, crc.out, live);
}

// A call that fails part-way may leave a slot's H2D / kernel / D2H in
// flight; the next call would then memcpy into staging the DMA engine is
// still reading or writing. So a failed call drains every slot stream before
// it returns (a successful one has already waited for every slot it used).
hrs_status host_apply(hrs_codec* c, const uint8_t* m, int nout, int nin, const uint8_t* const* in_rows,
                      uint8_t* const* out_rows, size_t len, bool static_kp, const HostCrc& crc = HostCrc()) {
  const hrs_status st = host_apply_impl(c, RowOp{m, nout, nin, static_kp, crc.mode}, in_rows, out_rows, len, crc);
  if (st != HRS_OK)
    for (auto& h : c->host)
      if (h.stream) (void)hipStreamSynchronize(h.stream);
  return st;
}

// ---------------------------------------- asynchronous host-buffer calls
// An Encoder / Decoder round split in two: submit copies the caller's rows
// into a free slot's pinned staging (the rows may be reused as soon as it
// returns: Java heap arrays are pinned only for the call) and queues the
// whole cell as one stage_chunk on the slot's stream (its raw window CRCs
// stay in device memory: no host fold here); collect waits for that operation
// and copies its output rows (and chained CRCs) out. While round r runs on
// the GPU the caller reads round r + 1 and submits it, so successive rounds
// overlap (Encoder.java:421-453 runs them back to back).

hrs_status async_submit_impl(hrs_codec* c, AsyncSlot& a, const RowOp& op, const uint8_t* const* in_rows, size_t len) {
  LiveRows live;
  hrs_status st = live_inputs(c, op, in_rows, live);
  if (st != HRS_OK) return st;
  const StageLayout lay(len, live.nlive, op.nout, op.ncrc());
  st = stage_slot(c, a, lay.need);
  if (st != HRS_OK) return st;
  std::vector<hrs::CopyJob> jobs;
  for (int i = 0; i < op.nin; ++i)
    if (live.slot_of[i] >= 0) jobs.push_back({a.pin + lay.pitch * live.slot_of[i], in_rows[i], len, host_store_mode()});
  copy_pool(c).run(jobs);
  const bool zc = zero_copy_ok(c, op, live.nlive, len, a.pin_dev != nullptr);
  a.timed = false;
  if (c->timing) {
    for (hipEvent_t* ev : {&a.t_start, &a.t_end})
      if (!*ev) {
        hipError_t e = hipEventCreate(ev);
        if (e != hipSuccess) return hip_fail(c, e, "hipEventCreate");
      }
    hipError_t e = hipEventRecord(a.t_start, a.stream);
    if (e != hipSuccess) return hip_fail(c, e, "hipEventRecord");
    a.timed = true;
  }
  st = stage_chunk(c, op, a, lay, live, len, zc, nullptr);
  if (st != HRS_OK) return st;
  hipError_t e = hipSuccess;
  if (a.timed && (e = hipEventRecord(a.t_end, a.stream)) != hipSuccess) return hip_fail(c, e, "hipEventRecord");
  e = hipEventRecord(a.done, a.stream);
  if (e != hipSuccess) return hip_fail(c, e, "hipEventRecord");
  a.nlive = live.nlive;
  a.pitch = lay.pitch;
  a.crc_off = lay.crc_off;
  a.queued = true;
  return HRS_OK;
}

hrs_status async_submit(hrs_codec* c, const uint8_t* m, int nout, int nin, const uint8_t* const* in_rows, size_t len,
                        bool static_kp, int crc_mode, uint64_t* ticket) {
  if (!ticket) return fail(c, HRS_EINVAL, "ticket is NULL");
  *ticket = 0;
  int free_slot = -1;
  for (int i = 0; i < hrs::kAsyncSlots && free_slot < 0; ++i)
    if (!c->async[i].busy) free_slot = i;
  if (free_slot < 0)
    return fail(c, HRS_EINVAL, "all %d asynchronous slots hold uncollected operations: collect one first",
                hrs::kAsyncSlots);
  AsyncSlot& a = c->async[free_slot];
  a.queued = false;
  a.timed = false;
  a.nout = nout;
  a.ncrc = ncrc_for(crc_mode, nin, nout);
  a.len = len;
  if (len > 0 && nout > 0) {
    DeviceGuard g(c->device);
    if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
    const hrs_status st = async_submit_impl(c, a, RowOp{m, nout, nin, static_kp, crc_mode}, in_rows, len);
    if (st != HRS_OK) {  // leave nothing in flight in a slot marked free
      if (a.stream) (void)hipStreamSynchronize(a.stream);
      a.queued = false;
      return st;
    }
  }
  a.busy = true;
  a.ticket = ++c->async_tickets;
  *ticket = a.ticket;
  return HRS_OK;
}

// The busy slot that holds `ticket`, or NULL.
AsyncSlot* find_ticket(hrs_codec* c, uint64_t ticket) {
  for (auto& s : c->async)
    if (s.busy && s.ticket == ticket) return &s;
  return nullptr;
}

hrs_status no_ticket(hrs_codec* c, uint64_t ticket) {
  return fail(c, HRS_EINVAL, "no uncollected operation with ticket %llu", static_cast<unsigned long long>(ticket));
}

// The argument block of the 5-argument decodes, then their locations.
// outs_ok: what this call writes when ne > 0 (write_bufs, crc_out) is there.
hrs_status decode_args_ok(hrs_codec* c, const void* read_bufs, bool outs_ok, const int* erased, int ne,
                          const int* to_read, int nr, const int* ntr, int nn) {
  if (!read_bufs || (ne > 0 && (!outs_ok || !erased)) || ne < 0 || nn < 0 || nr < 0 || (nn > 0 && !ntr))
    return fail(c, HRS_EINVAL, "bad decode arguments");
  if (!decode_locations_ok(c, erased, ne, to_read, nr, ntr, nn))
    return fail(c, HRS_EINVAL, "location out of range [0,%d)", c->n);
  return HRS_OK;
}

}  // namespace
}  // namespace hrs::api

using namespace hrs::api;

extern "C" {

hrs_status hrs_encode(hrs_codec* c, const uint8_t* const* inputs, uint8_t* const* outputs, size_t len) {
  if (!c) return HRS_EINVAL;
  if (!inputs || !outputs) return fail(c, HRS_EINVAL, "inputs/outputs is NULL");
  return host_apply(c, c->g.data(), c->p, c->k, inputs, outputs, len, static_encode_family(c));
}

hrs_status hrs_encode_crc(hrs_codec* c, const uint8_t* const* inputs, uint8_t* const* outputs, size_t len,
                          const uint32_t* crc_in, uint32_t* crc_out) {
  if (!c) return HRS_EINVAL;
  if (!inputs || !outputs || !crc_out) return fail(c, HRS_EINVAL, "inputs/outputs/crc_out is NULL");
  return host_apply(c, c->g.data(), c->p, c->k, inputs, outputs, len, static_encode_family(c),
                    HostCrc{kCrcEncode, crc_in, crc_out});
}

hrs_status hrs_decode_crc(hrs_codec* c, const uint8_t* const* read_bufs, uint8_t* const* write_bufs,
                          const int* erased, int ne, const int* to_read, int nr, const int* ntr, int nn, size_t len,
                          const uint32_t* crc_in, uint32_t* crc_out) {
  if (!c) return HRS_EINVAL;
  hrs_status st = decode_args_ok(c, read_bufs, write_bufs && crc_out, erased, ne, to_read, nr, ntr, nn);
  if (st != HRS_OK || ne == 0) return st;
  std::vector<uint8_t> tmp;
  const uint8_t* d = nullptr;
  st = decode5_matrix(c, erased, ne, ntr, nn, read_bufs, tmp, &d, to_read, to_read ? nr : -1);
  if (st != HRS_OK) return st;
  return host_apply(c, d, ne, c->n, read_bufs, write_bufs, len, false, HostCrc{kCrcOutputs, crc_in, crc_out});
}

hrs_status hrs_decode(hrs_codec* c, const uint8_t* const* read_bufs, uint8_t* const* write_bufs, const int* erased,
                      int ne, const int* to_read, int nr, const int* ntr, int nn, size_t len) {
  if (!c) return HRS_EINVAL;
  hrs_status st = decode_args_ok(c, read_bufs, write_bufs != nullptr, erased, ne, to_read, nr, ntr, nn);
  if (st != HRS_OK || (ne == 0 && c->kind == HRS_CODE_RS)) return st;
  std::vector<uint8_t> tmp;
  const uint8_t* d = nullptr;
  st = decode5_matrix(c, erased, ne, ntr, nn, read_bufs, tmp, &d, to_read, to_read ? nr : -1);
  if (st != HRS_OK) return st;
  return host_apply(c, d, ne, c->n, read_bufs, write_bufs, len, false);
}

hrs_status hrs_decode3(hrs_codec* c, const uint8_t* const* read_bufs, uint8_t* const* write_bufs, const int* erased,
                       int ne, size_t len) {
  if (!c) return HRS_EINVAL;
  if (ne < 0 || (ne > 0 && (!read_bufs || !write_bufs || !erased))) return fail(c, HRS_EINVAL, "bad decode3 arguments");
  if (c->kind == HRS_CODE_XOR) {  // XORCode.decodeBulk 3-arg == 5-arg (XORCode.java:140-145)
    std::vector<uint8_t> tmp;
    const uint8_t* d = nullptr;
    hrs_status st = decode5_matrix(c, erased, ne, nullptr, 0, read_bufs, tmp, &d);
    if (st != HRS_OK) return st;
    return host_apply(c, d, ne, c->n, read_bufs, write_bufs, len, false);
  }
  if (c->kind == HRS_CODE_NRS || c->kind == HRS_CODE_SRC)  // only ReedSolomonCode / XORCode have it
    return fail(c, HRS_EINVAL, "decodeBulk(readBufs, writeBufs, erasedLocations) is not supported by this code");
  if (ne == 0) return HRS_OK;  // ReedSolomonCode.java:170-172
  if (ne > c->p) return fail(c, HRS_EINVAL, "%d erasures > parity size %d", ne, c->p);  // errSignature[p]
  hrs_status st;
  const std::vector<uint8_t>* d = cached_decode_matrix(c, erased, ne, erased, ne, 0, &st);
  if (!d) return st;
  return host_apply(c, d->data(), ne, c->n, read_bufs, write_bufs, len, false);
}

hrs_status hrs_encode_submit(hrs_codec* c, const uint8_t* const* inputs, size_t len, int checksums, uint64_t* ticket) {
  if (!c) return HRS_EINVAL;
  if (!inputs) return fail(c, HRS_EINVAL, "inputs is NULL");
  return async_submit(c, c->g.data(), c->p, c->k, inputs, len, static_encode_family(c),
                      checksums ? kCrcEncode : kCrcNone, ticket);
}

hrs_status hrs_decode_submit(hrs_codec* c, const uint8_t* const* read_bufs, const int* erased, int ne,
                             const int* to_read, int nr, const int* ntr, int nn, size_t len, int checksums,
                             uint64_t* ticket) {
  if (!c) return HRS_EINVAL;
  hrs_status st = decode_args_ok(c, read_bufs, true, erased, ne, to_read, nr, ntr, nn);
  if (st != HRS_OK) return st;
  std::vector<uint8_t> tmp;
  const uint8_t* d = nullptr;
  if (ne > 0) {
    st = decode5_matrix(c, erased, ne, ntr, nn, read_bufs, tmp, &d, to_read, to_read ? nr : -1);
    if (st != HRS_OK) return st;
  }
  return async_submit(c, d, ne, c->n, read_bufs, ne > 0 ? len : 0, false, checksums ? kCrcOutputs : kCrcNone, ticket);
}

hrs_status hrs_collect(hrs_codec* c, uint64_t ticket, uint8_t* const* outputs, uint32_t* crc_io) {
  if (!c) return HRS_EINVAL;
  AsyncSlot* a = find_ticket(c, ticket);
  if (!a) return no_ticket(c, ticket);
  if (a->nout > 0 && a->len > 0 && !outputs) return fail(c, HRS_EINVAL, "outputs is NULL");
  if (a->ncrc > 0 && !crc_io) return fail(c, HRS_EINVAL, "crc_io is NULL for a checksummed operation");
  for (int o = 0; o < a->nout && a->len > 0; ++o)
    if (!outputs[o]) return fail(c, HRS_EINVAL, "output row %d is NULL", o);
  hrs_status st = HRS_OK;
  if (a->queued) {
    hipError_t e = hipEventSynchronize(a->done);
    if (e != hipSuccess) {
      // the slot's H2D / kernel / D2H may still be in flight: drain its stream
      // before the slot is marked free, so the next submit cannot refill
      // staging the DMA engine is still using
      st = hip_fail(c, e, "hipEventSynchronize");
      DeviceGuard g(c->device);
      (void)hipStreamSynchronize(a->stream);
    }
  }
  if (st == HRS_OK && a->queued) {
    std::vector<hrs::CopyJob> jobs;
    for (int o = 0; o < a->nout; ++o) jobs.push_back({outputs[o], a->pin + a->pitch * (a->nlive + o), a->len});
    copy_pool(c).run(jobs);
    chain_crcs(c, a->len, crc_io, reinterpret_cast<const uint32_t*>(a->pin + a->crc_off), a->ncrc);
  }
  a->busy = false;
  a->queued = false;
  return st;
}

hrs_status hrs_wait(hrs_codec* c, uint64_t ticket) {
  if (!c) return HRS_EINVAL;
  const AsyncSlot* a = find_ticket(c, ticket);
  if (!a) return no_ticket(c, ticket);
  if (!a->queued) return HRS_OK;
  hipError_t e = hipEventSynchronize(a->done);
  return e == hipSuccess ? HRS_OK : hip_fail(c, e, "hipEventSynchronize");
}

hrs_status hrs_release(hrs_codec* c, uint64_t ticket) {
  if (!c) return HRS_EINVAL;
  AsyncSlot* a = find_ticket(c, ticket);
  if (!a) return no_ticket(c, ticket);
  hrs_status st = HRS_OK;
  if (a->queued) {  // nothing of this round may still read or write the slot's staging
    DeviceGuard g(c->device);
    const hipError_t e = hipStreamSynchronize(a->stream);
    if (e != hipSuccess) st = hip_fail(c, e, "hipStreamSynchronize");
  }
  a->busy = false;
  a->queued = false;
  return st;
}

hrs_status hrs_ticket_shape(const hrs_codec* c, uint64_t ticket, int* num_outputs, size_t* len, int* num_crcs) {
  if (!c) return HRS_EINVAL;
  const AsyncSlot* a = find_ticket(const_cast<hrs_codec*>(c), ticket);
  if (!a) return HRS_EINVAL;  // a query: the handle's message stays
  if (num_outputs) *num_outputs = a->nout;
  if (len) *len = a->len;
  if (num_crcs) *num_crcs = a->ncrc;
  return HRS_OK;
}

hrs_status hrs_set_timing(hrs_codec* c, int on) {
  if (!c) return HRS_EINVAL;
  c->timing = on != 0;
  return HRS_OK;
}

hrs_status hrs_ticket_gpu_ms(const hrs_codec* cc, uint64_t ticket, float* ms) {
  auto* c = const_cast<hrs_codec*>(cc);
  if (!c || !ms) return HRS_EINVAL;
  const AsyncSlot* a = find_ticket(c, ticket);
  if (!a) return no_ticket(c, ticket);
  if (!a->queued || !a->timed)
    return fail(c, HRS_EINVAL, "operation %llu was submitted without timing", static_cast<unsigned long long>(ticket));
  DeviceGuard g(c->device);
  const hipError_t e = hipEventElapsedTime(ms, a->t_start, a->t_end);
  return e == hipSuccess ? HRS_OK : hip_fail(c, e, "hipEventElapsedTime");
}

int hrs_pending(const hrs_codec* c) {
  if (!c) return -1;
  int n = 0;
  for (const auto& s : c->async) n += s.busy;
  return n;
}

}  // extern "C"
