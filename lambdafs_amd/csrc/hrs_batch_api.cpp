// Device-resident repair batches: heterogeneous batches (one erasure pattern
// per stripe, plans uploaded through pinned slots, one batch launch) with
// their block-CRC-32 form (hrs_decode_batch_dev, hrs_decode_batch_crc_dev)
// and their ragged forms (hrs_decode_batch_ragged_dev: per-cell lengths;
// hrs_decode_batch_ragged_crc_dev: with each rebuilt cell's CRC-32 over its length),
// and the per-call table slots every unit uploads through. The host-memory
// batches that run their chunks through run_batch are in hrs_hostbatch_api.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/hrs.h"
#include "hrs_batch_ragged.hpp"
#include "hrs_codec.hpp"
#include "hrs_crc.hpp"
#include "hrs_internal.hpp"
#include "hrs_launch.hpp"
#include "hrs_ragged.hpp"

namespace hrs::api {

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

namespace {

// The next batch slot, idle and at least `need` bytes on both sides (a slot is
// reused once the event recorded after its last launch has completed).
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

// Whether the vector kernels may take the batch: bases and strides 16-byte aligned.
bool vector_aligned(const BatchGeom& g) {
  return aligned16(g.stripes) && aligned16(g.out) && g.row_stride % 16 == 0 && g.stripe_stride % 16 == 0 &&
         g.out_row_stride % 16 == 0 && g.out_stripe_stride % 16 == 0;
}

// The kernel arguments every launch over stripes [s0, ...) of the batch shares.
hrs::BatchArgs batch_args(const BatchPlanSet& ps, const BatchGeom& g, size_t s0) {
  hrs::BatchArgs a{};
  a.base = g.stripes;
  a.out = g.out;
  a.row_stride = g.row_stride;
  a.stripe_stride = g.stripe_stride;
  a.out_row_stride = g.out_row_stride;
  a.out_stripe_stride = g.out_stripe_stride;
  a.len = g.len;
  a.plans = ps.dplans;
  a.pat = ps.dpat + s0;
  return a;
}

// The ragged launches of stripes [s0, s0 + ns): batch_ragged_kernel over the
// whole 2 KiB windows of an aligned batch of its shapes, the byte-granular
// kernel over the row tail, every other shape or layout and kernel mode 2.
hrs::BatchRaggedArgs batch_ragged_args(const BatchPlanSet& ps, const BatchGeom& g, size_t s0) {
  hrs::BatchRaggedArgs a{};
  a.b = batch_args(ps, g, s0);
  a.lens = ps.dlens + s0 * static_cast<size_t>(ps.len_words);
  a.words = ps.len_words;
  a.nin_words = ps.max_nin;
  return a;
}

hrs_status launch_batch_ragged(hrs_codec* c, const BatchPlanSet& ps, const BatchGeom& g, size_t s0, size_t ns,
                               hipStream_t hs) {
  hrs::BatchRaggedArgs a = batch_ragged_args(ps, g, s0);
  const bool vec = c->kernel_mode != 2 && vector_aligned(g) && hrs::batch_ragged_vector_shape(ps.max_nout, ps.max_nin);
  a.b.nwin = vec ? g.len / hrs::kWindowBytes : 0;
  if (a.b.nwin > 0) {
    a.b.ntasks = a.b.nwin * ns;
    hipError_t e = hrs::launch_batch_ragged(a, ps.max_nout, ps.max_nin, hs);
    if (e != hipSuccess) return hip_fail(c, e, "ragged batch launch");
    c->last_kernel = hrs::last_kernel();
  }
  a.b.col0 = a.b.nwin * hrs::kWindowBytes;
  if (a.b.col0 < g.len) {
    a.b.ntasks = (g.len - a.b.col0) * ns;
    hipError_t e = hrs::launch_batch_ragged_bytewise(a, hs);
    if (e != hipSuccess) return hip_fail(c, e, "ragged batch bytewise launch");
    if (a.b.nwin == 0) c->last_kernel = hrs::last_kernel();  // the call's only kernel
  }
  return HRS_OK;
}

hrs_status launch_batch(hrs_codec* c, const BatchPlanSet& ps, const BatchGeom& g, size_t s0, size_t ns,
                        hipStream_t hs, bool ragged = false) {
  if (ragged) return launch_batch_ragged(c, ps, g, s0, ns, hs);
  if (!ps.fused) {  // shapes beyond the batch kernel (wide codes): one launch per stripe
    std::vector<const uint8_t*> rows(c->n);
    std::vector<uint8_t*> outs(hrs::kMaxOut);
    for (size_t i = 0; i < ns; ++i) {
      const int id = ps.pat[s0 + i];
      const hrs::BatchPlan& pl = ps.plans[id];
      if (pl.nout == 0) continue;
      for (int l = 0; l < c->n; ++l) rows[l] = g.stripes + i * g.stripe_stride + l * g.row_stride;
      for (int o = 0; o < pl.nout; ++o) outs[o] = g.out + i * g.out_stripe_stride + o * g.out_row_stride;
      hrs_status st =
          run_apply(c, ps.mats[id].data(), pl.nout, c->n, rows.data(), 0, outs.data(), 0, g.len, 1, hs, false);
      if (st != HRS_OK) return st;
    }
    return HRS_OK;
  }
  hrs::BatchArgs a = batch_args(ps, g, s0);
  a.nwin = c->kernel_mode != 2 && vector_aligned(g) ? g.len / hrs::kWindowBytes : 0;
  if (a.nwin > 0) {
    a.ntasks = a.nwin * ns;
    hipError_t e = hrs::launch_batch_bitsliced(a, ps.max_nout, ps.max_nin, hs);
    if (e != hipSuccess) return hip_fail(c, e, "batch launch");
    c->last_kernel = hrs::last_kernel();
  }
  a.col0 = a.nwin * hrs::kWindowBytes;
  if (a.col0 < g.len) {
    a.ntasks = (g.len - a.col0) * ns;
    hipError_t e = hrs::launch_batch_bytewise(a, hs);
    if (e != hipSuccess) return hip_fail(c, e, "batch bytewise launch");
    if (a.nwin == 0) c->last_kernel = hrs::last_kernel();  // the call's only kernel
  }
  return HRS_OK;
}

// launch_batch + the CRC-32 of every repaired cell (BatchCrcs). The fold reads
// every stripe's loss count from the uploaded plans, the per-stripe fallback's
// too. raw: crc_raw_bytes_for(len, ns, max_erased) bytes of scratch.
// One pass (batch_decode_crc_kernel) for aligned whole-window batches of the
// one-pattern fused kernel's shapes; else launch_batch, the CRC window pass
// over the outputs (rows past a stripe's losses lie inside `out` and are read;
// the fold discards them) and the same fold.
hrs_status launch_batch_crc(hrs_codec* c, const BatchPlanSet& ps, const BatchGeom& g, size_t s0, size_t ns,
                            const BatchCrcs& crc, hipStream_t hs, uint32_t* raw) {
  const BatchCrcMask mask{ps.dplans, ps.dpat + s0, crc.max_erased};
  auto fold = [&](uint64_t win) {
    return crc_fold(c, g.len, ns * static_cast<uint64_t>(crc.max_erased), crc.in, crc.out, hs, raw, win, &mask);
  };
  if (ps.max_nout == 0)  // nothing lost anywhere: every CRC continues over no bytes
    return fold(hrs::kCrcWindow);
  // the one-pattern fused kernel's shapes at the batch's largest pattern
  if (ps.fused && apply_crc_one_pass(c, ps.max_nout, ps.max_nin, g.len) && vector_aligned(g)) {
    hrs_status st = crc_window_tables(c);
    if (st != HRS_OK) return st;
    hrs::BatchCrcArgs d{};
    d.b = batch_args(ps, g, s0);
    d.b.nwin = g.len / hrs::kWindowBytes;
    d.b.ntasks = d.b.nwin * ns;
    d.raw = raw;
    d.tables = c->crc_tables_a;
    d.rows_per_stripe = crc.max_erased;
    hipError_t e = hrs::launch_batch_decode_crc(d, ps.max_nout, ps.max_nin, hrs::device_cu_count(), hs);
    if (e != hipSuccess) return hip_fail(c, e, "batch decode+crc launch");
    c->last_kernel = hrs::last_kernel();
    return fold(hrs::kWindowBytes);
  }
  hrs_status st = launch_batch(c, ps, g, s0, ns, hs);
  if (st != HRS_OK) return st;
  const uint8_t* rows[hrs::kMaxOut];
  size_t strides[hrs::kMaxOut];
  for (int t = 0; t < ps.max_nout; ++t) {
    rows[t] = g.out + static_cast<size_t>(t) * g.out_row_stride;
    strides[t] = g.out_stripe_stride;
  }
  st = crc_windows(c, rows, strides, ps.max_nout, crc.max_erased, g.len, ns, hs, raw);
  if (st != HRS_OK) return st;
  return fold(hrs::kCrcWindow);
}

// launch_batch(ragged) + the CRC-32 of every repaired cell over exactly its
// length (include/hrs.h, "ragged repair + CRC-32"). The lengths the kernels and
// the fold read are the output words of the plan-order table (ps.dlens), which
// are 0 past a stripe's losses. One pass (batch_ragged_crc_kernel) for aligned
// whole-window batches of the fused shapes in kernel modes 0 and 3; else the
// ragged repair (its kernel names the call), the ragged CRC window pass over
// the max_nout output rows up to each cell's length (it reads back only bytes
// the repair just wrote) and the same fold with the row's padding.
hrs_status launch_batch_ragged_crc(hrs_codec* c, const BatchPlanSet& ps, const BatchGeom& g, size_t s0, size_t ns,
                                   const BatchCrcs& crc, hipStream_t hs, uint32_t* raw) {
  const hrs::BatchRaggedArgs ra = batch_ragged_args(ps, g, s0);
  auto fold = [&](uint64_t win) -> hrs_status {
    hrs_codec::FoldTables* ft = nullptr;
    hrs_status st = crc_fold_tables(c, g.len, win, &ft);
    if (st != HRS_OK) return st;
    hrs::BatchRaggedCrcFoldArgs b{};
    b.f.raw = raw;
    b.f.nwin = g.len / win;
    b.f.tail = g.len % win;
    b.f.nsr = ns * static_cast<uint64_t>(crc.max_erased);
    b.f.G = static_cast<int>((b.f.nwin + 63) / 64);
    b.f.tables = ft->dev;
    b.f.crc_in = crc.in;
    b.f.crc_out = crc.out;
    b.lens = ra.lens;
    b.words = ra.words;
    b.nin_words = ra.nin_words;
    b.max_nout = ps.max_nout;
    b.rows_per_stripe = crc.max_erased;
    b.len = static_cast<uint32_t>(g.len);
    b.fused = win == static_cast<uint64_t>(hrs::kWindowBytes);
    const hipError_t e = hrs::launch_batch_ragged_crc_fold(b, hrs::device_cu_count(), hs);
    if (e != hipSuccess) return hip_fail(c, e, "ragged crc fold launch");
    return fold_tables_used(c, ft, hs);
  };
  if (apply_crc_one_pass(c, ps.max_nout, ps.max_nin, g.len) && vector_aligned(g)) {
    hrs_status st = crc_window_tables(c);
    if (st != HRS_OK) return st;
    hrs::BatchRaggedCrcArgs d{};
    d.r = ra;
    d.r.b.nwin = g.len / hrs::kWindowBytes;
    d.r.b.ntasks = d.r.b.nwin * ns;
    d.raw = raw;
    d.tables = c->crc_tables_a;
    d.rows_per_stripe = crc.max_erased;
    const hipError_t e = hrs::launch_batch_ragged_crc(d, ps.max_nout, ps.max_nin, hrs::device_cu_count(), hs);
    if (e != hipSuccess) return hip_fail(c, e, "ragged batch decode+crc launch");
    c->last_kernel = hrs::last_kernel();
    return fold(hrs::kWindowBytes);
  }
  hrs_status st = launch_batch_ragged(c, ps, g, s0, ns, hs);
  if (st != HRS_OK) return st;
  if ((st = crc_window_tables(c)) != HRS_OK) return st;
  hrs::RaggedCrcWinArgs w{};
  w.w.nrows = ps.max_nout;
  bool aligned = aligned16(g.out) && g.out_row_stride % 16 == 0 && g.out_stripe_stride % 16 == 0;
  for (int t = 0; t < ps.max_nout; ++t) {
    w.w.rows[t] = g.out + static_cast<size_t>(t) * g.out_row_stride;
    w.w.stride[t] = g.out_stripe_stride;
  }
  w.w.row0 = 0;
  w.w.nrows_total = crc.max_erased;
  w.w.len = g.len;
  w.w.nwin = g.len / hrs::kCrcWindow;
  w.w.tail = g.len % hrs::kCrcWindow;
  w.w.nstripes = ns;
  w.w.raw = raw;
  w.w.tables = c->crc_tables_a;
  // row t of stripe i is cut at the table's output word t: lens[i * words + nin_words + t]
  w.valid = ra.lens + ra.nin_words;
  w.k = ra.words;
  const hipError_t e = hrs::launch_crc_ragged_windows(w, aligned, hrs::device_cu_count(), hs);
  if (e != hipSuccess) return hip_fail(c, e, "ragged crc window launch");
  return fold(hrs::kCrcWindow);  // the repair's kernel names the call
}

}  // namespace

hrs_status run_batch(hrs_codec* c, const BatchPlanSet& ps, const BatchGeom& g, size_t s0, size_t ns,
                     const BatchCrcs* crc, hipStream_t s, bool ragged) {
  if (!crc) return launch_batch(c, ps, g, s0, ns, s, ragged);
  return with_crc_scratch(c, crc_raw_bytes_for(g.len, ns, crc->max_erased), s, [&] {
    return ragged ? launch_batch_ragged_crc(c, ps, g, s0, ns, *crc, s, c->crc_raw)
                  : launch_batch_crc(c, ps, g, s0, ns, *crc, s, c->crc_raw);
  });
}

hrs_status upload(hrs_codec* c, const void* a, size_t a_bytes, const void* b, size_t b_bytes, hipStream_t s,
                  hrs_codec::BatchSlot** slot) {
  hrs_codec::BatchSlot* sl = nullptr;
  const hrs_status st = batch_slot_acquire(c, a_bytes + b_bytes, &sl);
  if (st != HRS_OK) return st;
  std::memcpy(sl->host, a, a_bytes);
  std::memcpy(sl->host + a_bytes, b, b_bytes);
  const hipError_t e = hipMemcpyAsync(sl->dev, sl->host, a_bytes + b_bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_fail(c, e, "hipMemcpyAsync table");
  *slot = sl;
  return HRS_OK;
}

void slot_used(hrs_codec::BatchSlot* sl, hipStream_t s) {
  if (hipEventRecord(sl->done, s) == hipSuccess) sl->pending = true;
  else (void)hipStreamSynchronize(s);
}

hrs_status upload_plans(hrs_codec* c, BatchPlanSet& ps, hipStream_t s) {
  const size_t plan_bytes = ps.plans.size() * sizeof(hrs::BatchPlan);
  if (!ps.lens.empty()) {  // a ragged batch: the length table behind the pattern indices, same upload
    const size_t pat_bytes = ps.pat.size() * sizeof(int32_t), len_bytes = ps.lens.size() * sizeof(uint32_t);
    const hrs_status st = batch_slot_acquire(c, plan_bytes + pat_bytes + len_bytes, &ps.slot);
    if (st != HRS_OK) return st;
    std::memcpy(ps.slot->host, ps.plans.data(), plan_bytes);
    std::memcpy(ps.slot->host + plan_bytes, ps.pat.data(), pat_bytes);
    std::memcpy(ps.slot->host + plan_bytes + pat_bytes, ps.lens.data(), len_bytes);
    const hipError_t e =
        hipMemcpyAsync(ps.slot->dev, ps.slot->host, plan_bytes + pat_bytes + len_bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(c, e, "hipMemcpyAsync table");
    ps.dplans = reinterpret_cast<const hrs::BatchPlan*>(ps.slot->dev);
    ps.dpat = reinterpret_cast<const int32_t*>(ps.slot->dev + plan_bytes);
    ps.dlens = reinterpret_cast<const uint32_t*>(ps.slot->dev + plan_bytes + pat_bytes);
    return HRS_OK;
  }
  const hrs_status st = upload(c, ps.plans.data(), plan_bytes, ps.pat.data(), ps.pat.size() * sizeof(int32_t), s,
                               &ps.slot);
  if (st != HRS_OK) return st;
  ps.dplans = reinterpret_cast<const hrs::BatchPlan*>(ps.slot->dev);
  ps.dpat = reinterpret_cast<const int32_t*>(ps.slot->dev + plan_bytes);
  return HRS_OK;
}

bool crc_arrays_apart(const uint32_t* crc_in, const uint32_t* crc_out, size_t n) {
  if (!crc_in || crc_in == crc_out) return true;
  const uintptr_t a = reinterpret_cast<uintptr_t>(crc_in), b = reinterpret_cast<uintptr_t>(crc_out);
  return a + n * 4 <= b || b + n * 4 <= a;
}

hrs_status crc_args_ok(hrs_codec* c, const uint32_t* crc_in, const uint32_t* crc_out, size_t n) {
  if (!crc_out) return fail(c, HRS_EINVAL, "crc_out is NULL");
  if (!crc_arrays_apart(crc_in, crc_out, n))
    return fail(c, HRS_EINVAL, "crc_in and crc_out overlap (crc_out may only be crc_in itself)");
  return HRS_OK;
}

hrs_status decode_batch_args_ok(hrs_codec* c, const BatchGeom& g, const int* erased, int max_erased, size_t nstripes,
                                unsigned flags, const uint32_t* crc_in, const uint32_t* crc_out, bool* empty) {
  *empty = false;
  if (!c) return HRS_EINVAL;
  if (!g.stripes || !g.out || max_erased < 0 || max_erased > hrs::kMaxOut || (max_erased > 0 && !erased))
    return fail(c, HRS_EINVAL, "bad batch decode arguments (max_erased must be in [0, %d])", hrs::kMaxOut);
  if (nstripes == 0 || g.len == 0 || max_erased == 0) {
    *empty = true;
    return HRS_OK;
  }
  if (!(flags & kBatchDeviceSet) && nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  if (flags & kBatchWithCrc) return crc_args_ok(c, crc_in, crc_out, nstripes * static_cast<size_t>(max_erased));
  return HRS_OK;
}

hrs_status ragged_batch_args_ok(hrs_codec* c, const BatchGeom& g, const int* erased, int max_erased, size_t nstripes,
                                const uint32_t* valid, BatchPlanSet& ps, bool* empty, bool* all_full, unsigned flags,
                                const uint32_t* crc_in, const uint32_t* crc_out) {
  *all_full = false;
  hrs_status st = decode_batch_args_ok(c, g, erased, max_erased, nstripes, flags, crc_in, crc_out, empty);
  if (st != HRS_OK) return st;
  if (!valid) return fail(c, HRS_EINVAL, "valid is NULL");
  if (*empty) return HRS_OK;
  if (g.len > UINT32_MAX) return fail(c, HRS_EINVAL, "ragged repair: len %zu exceeds 2^32 - 1", g.len);
  const size_t n = static_cast<size_t>(c->n);
  bool full = true;
  for (size_t s = 0; s < nstripes; ++s)
    for (size_t l = 0; l < n; ++l) {
      const uint32_t v = valid[s * n + l];
      if (v > g.len) return fail(c, HRS_EINVAL, "stripe %zu location %zu: valid %u exceeds len %zu", s, l, v, g.len);
      full &= v == g.len;
    }
  *all_full = full;
  if ((st = build_batch_plans(c, erased, max_erased, nstripes, ps)) != HRS_OK) return st;
  for (size_t s = 0; s < nstripes && !ps.fused; ++s)
    if (ps.plans[ps.pat[s]].nin > hrs::kBatchMaxIn)
      return fail(c, HRS_EINVAL, "stripe %zu: its pattern reads %d survivors, a ragged repair batch at most %d", s,
                  ps.plans[ps.pat[s]].nin, hrs::kBatchMaxIn);
  return HRS_OK;
}

void plan_order_lengths(const hrs_codec* c, const int* erased, int max_erased, size_t nstripes, const uint32_t* valid,
                        BatchPlanSet& ps) {
  const size_t n = static_cast<size_t>(c->n), words = static_cast<size_t>(ps.max_nin + ps.max_nout);
  ps.len_words = static_cast<int>(words);
  ps.lens.assign(nstripes * words, 0u);
  for (size_t s = 0; s < nstripes; ++s) {
    const hrs::BatchPlan& pl = ps.plans[ps.pat[s]];
    uint32_t* w = ps.lens.data() + s * words;
    for (int r = 0; r < pl.nin; ++r) w[r] = valid[s * n + pl.loc[r]];
    for (int t = 0; t < pl.nout; ++t) w[ps.max_nin + t] = valid[s * n + erased[s * max_erased + t]];
  }
}

}  // namespace hrs::api

using namespace hrs::api;

namespace {

// hrs_decode_batch_dev and hrs_decode_batch_crc_dev (with_crc; DEVICE arrays).
// The plain call is done when nothing is lost anywhere and uploads no plans
// for the per-stripe fallback; the CRC form always uploads them and runs the
// fold even then (every CRC continues over no bytes).
hrs_status decode_batch_dev_entry(hrs_codec* c, const BatchGeom& g, const int* erased, int max_erased,
                                  size_t nstripes, bool with_crc, const uint32_t* crc_in, uint32_t* crc_out,
                                  void* stream) {
  bool empty = false;
  hrs_status st =
      decode_batch_args_ok(c, g, erased, max_erased, nstripes, with_crc ? kBatchWithCrc : 0u, crc_in, crc_out, &empty);
  if (st != HRS_OK || empty) return st;
  BatchPlanSet ps;
  st = build_batch_plans(c, erased, max_erased, nstripes, ps);
  if (st != HRS_OK) return st;
  DeviceGuard guard(c->device);
  if (!guard.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  if (ps.max_nout == 0 && !with_crc) return HRS_OK;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if ((ps.fused || with_crc) && (st = upload_plans(c, ps, hs)) != HRS_OK) return st;
  const BatchCrcs crc{max_erased, crc_in, crc_out};
  st = run_batch(c, ps, g, 0, nstripes, with_crc ? &crc : nullptr, hs);
  if (ps.slot) slot_used(ps.slot, hs);
  return st;
}

// hrs_decode_batch_ragged_dev and hrs_decode_batch_ragged_crc_dev (with_crc;
// DEVICE arrays): the sibling's entry with a length per cell. valid is read on
// the host and leaves in plan order with the plans' upload, so the caller may
// reuse it when the call returns. With CRCs a batch that lost nothing anywhere
// still runs the plain batch's fold (every CRC continues over no bytes).
hrs_status decode_batch_ragged_dev_entry(hrs_codec* c, const BatchGeom& g, const int* erased, int max_erased,
                                         size_t nstripes, const uint32_t* valid, bool with_crc, const uint32_t* crc_in,
                                         uint32_t* crc_out, void* stream) {
  if (!c) return HRS_EINVAL;
  BatchPlanSet ps;
  bool empty = false, all_full = false;
  hrs_status st = ragged_batch_args_ok(c, g, erased, max_erased, nstripes, valid, ps, &empty, &all_full,
                                       with_crc ? kBatchWithCrc : 0u, crc_in, crc_out);
  if (st != HRS_OK || empty) return st;
  DeviceGuard guard(c->device);
  if (!guard.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  if (ps.max_nout == 0 && !with_crc) return HRS_OK;
  const bool ragged = ps.max_nout > 0 && !ragged_batch_takes_plain(c, all_full);
  if (ragged) plan_order_lengths(c, erased, max_erased, nstripes, valid, ps);
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if ((st = upload_plans(c, ps, hs)) != HRS_OK) return st;
  const BatchCrcs crc{max_erased, crc_in, crc_out};
  st = run_batch(c, ps, g, 0, nstripes, with_crc ? &crc : nullptr, hs, ragged);
  slot_used(ps.slot, hs);
  return st;
}

}  // namespace

extern "C" {

hrs_status hrs_decode_batch_ragged_dev(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                       const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                       size_t out_stripe_stride, size_t len, size_t nstripes, const uint32_t* valid,
                                       void* stream) {
  return decode_batch_ragged_dev_entry(
      c, {stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride, len}, erased, max_erased,
      nstripes, valid, false, nullptr, nullptr, stream);
}

hrs_status hrs_decode_batch_ragged_crc_dev(hrs_codec* c, const uint8_t* stripes, size_t row_stride,
                                           size_t stripe_stride, const int* erased, int max_erased, uint8_t* out,
                                           size_t out_row_stride, size_t out_stripe_stride, size_t len,
                                           size_t nstripes, const uint32_t* valid, const uint32_t* crc_in,
                                           uint32_t* crc_out, void* stream) {
  return decode_batch_ragged_dev_entry(
      c, {stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride, len}, erased, max_erased,
      nstripes, valid, true, crc_in, crc_out, stream);
}

hrs_status hrs_decode_batch_dev(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                size_t out_stripe_stride, size_t len, size_t nstripes, void* stream) {
  return decode_batch_dev_entry(c, {stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride, len},
                                erased, max_erased, nstripes, false, nullptr, nullptr, stream);
}

hrs_status hrs_decode_batch_crc_dev(hrs_codec* c, const uint8_t* stripes, size_t row_stride, size_t stripe_stride,
                                    const int* erased, int max_erased, uint8_t* out, size_t out_row_stride,
                                    size_t out_stripe_stride, size_t len, size_t nstripes, const uint32_t* crc_in,
                                    uint32_t* crc_out, void* stream) {
  return decode_batch_dev_entry(c, {stripes, row_stride, stripe_stride, out, out_row_stride, out_stripe_stride, len},
                                erased, max_erased, nstripes, true, crc_in, crc_out, stream);
}

}  // extern "C"
