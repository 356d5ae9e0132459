// Device-resident dispatch: the matrix-apply planner that picks a gfx950
// kernel per shape (static encode, XOR, resident / pipelined / streaming
// runtime kernels, byte-granular tails), the ragged encode's planner, and the
// hrs_encode_dev, hrs_encode_ragged_dev, hrs_decode_dev and hrs_apply_dev
// entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/hrs.h"
#include "hrs_codec.hpp"
#include "hrs_internal.hpp"
#include "hrs_ragged.hpp"

namespace hrs::api {

using hrs::RowArgs;

// out_o = XOR_i m[o][i] * in_i for every stripe. `static_kp` allows the
// compile-time encode kernels when m is this codec's G and inputs are the k
// data rows in order.
hrs_status run_apply(hrs_codec* c, const uint8_t* m, int nout, int nin, const uint8_t* const* in_rows,
                     size_t in_stride, uint8_t* const* out_rows, size_t out_stride, size_t len,
                     size_t nstripes, hipStream_t s, bool static_kp) {
  if (nout < 0 || nin < 0 || nout > 255 || nin > 255) return fail(c, HRS_EINVAL, "bad matrix shape %dx%d", nout, nin);
  if (nout == 0 || len == 0 || nstripes == 0) return HRS_OK;
  for (int o = 0; o < nout; ++o)
    if (!out_rows[o]) return fail(c, HRS_EINVAL, "output row %d is NULL", o);
  // Inputs whose coefficients are zero for every output contribute nothing:
  // skip them (saves their HBM reads; exact, since 0 * x = 0).
  std::vector<int> live;
  for (int i = 0; i < nin; ++i) {
    bool any = false;
    for (int o = 0; o < nout; ++o) any |= m[o * nin + i] != 0;
    if (any) {
      if (!in_rows[i]) return fail(c, HRS_EINVAL, "input row %d is NULL but has nonzero coefficients", i);
      live.push_back(i);
    }
  }
  if (static_cast<int>(live.size()) != nin || !static_encode_family(c) || m != c->g.data()) static_kp = false;
  bool vec_ok = (in_stride % 16 == 0) && (out_stride % 16 == 0);
  for (int i : live) vec_ok &= aligned16(in_rows[i]);
  for (int o = 0; o < nout; ++o) vec_ok &= aligned16(out_rows[o]);
  const int mode = c->kernel_mode;
  if (mode == 2) vec_ok = false;
  if (mode == 1 || mode == 2) static_kp = false;

  const uint64_t nwin = vec_ok ? len / hrs::kWindowBytes : 0;
  const uint64_t tail_off = nwin * hrs::kWindowBytes;
  const uint64_t tail = len - tail_off;

  if (live.empty()) {  // all-zero matrix: outputs are zero
    for (int o = 0; o < nout; ++o)
      for (size_t st = 0; st < nstripes; ++st) {
        hipError_t e = hipMemsetAsync(out_rows[o] + st * out_stride, 0, len, s);
        if (e != hipSuccess) return hip_fail(c, e, "hipMemsetAsync");
      }
    c->last_kernel.clear();  // no kernel ran
    return HRS_OK;
  }

  if (static_kp && nwin > 0) {
    RowArgs a{};
    for (int i = 0; i < nin; ++i) a.in[i] = in_rows[i];
    for (int o = 0; o < nout; ++o) a.out[o] = out_rows[o];
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.len = len;
    a.nwin = nwin;
    a.ntasks = nwin * nstripes;
    a.nin = nin;
    a.nout = nout;
    bool handled = false;
    const int family = c->kind == HRS_CODE_NRS ? hrs::kStaticCauchy : hrs::kStaticRs;
    hipError_t e = hrs::launch_static_encode(family, c->k, c->p, a, s, &handled);
    if (e != hipSuccess) return hip_fail(c, e, "static encode launch");
    if (handled) {
      c->last_kernel = hrs::last_kernel();
      if (tail == 0) return HRS_OK;
      std::vector<const uint8_t*> tin(nin);
      std::vector<uint8_t*> tout(nout);
      for (int i = 0; i < nin; ++i) tin[i] = in_rows[i] + tail_off;
      for (int o = 0; o < nout; ++o) tout[o] = out_rows[o] + tail_off;
      // tail < one window: run_apply sends it to the byte-granular kernel;
      // the call keeps naming the static kernel
      const std::string main_kernel = c->last_kernel;
      const hrs_status st =
          run_apply(c, m, nout, nin, tin.data(), in_stride, tout.data(), out_stride, tail, nstripes, s, false);
      c->last_kernel = main_kernel;
      return st;
    }
  }

  const int nlive = static_cast<int>(live.size());
  // A single output whose live coefficients are all 1 is a plain XOR of rows
  // (the XOR code, XORCode.java:99-145): no bit-slicing needed.
  bool all_ones = (nout == 1) && nwin > 0 && mode == 0;
  for (int i : live) all_ones &= m[i] == 1;
  if (all_ones) {
    for (int i0 = 0; i0 < nlive; i0 += hrs::kMaxInRuntime) {
      const int ni = std::min(hrs::kMaxInRuntime, nlive - i0);
      RowArgs a{};
      for (int i = 0; i < ni; ++i) a.in[i] = in_rows[live[i0 + i]];
      a.out[0] = out_rows[0];
      a.in_stride = in_stride;
      a.out_stride = out_stride;
      a.len = len;
      a.nwin = nwin;
      a.ntasks = nwin * nstripes;
      a.nin = ni;
      a.nout = 1;
      a.accumulate = i0 > 0;
      hipError_t e = hrs::launch_xor(a, s);
      if (e != hipSuccess) return hip_fail(c, e, "xor launch");
      c->last_kernel = hrs::last_kernel();
      if (tail > 0) {
        RowArgs b = a;
        for (int i = 0; i < ni; ++i) {
          b.in[i] = a.in[i] + tail_off;
          hrs::set_coef(b, 0, i, 1);
        }
        b.out[0] = a.out[0] + tail_off;
        b.len = tail;
        b.nwin = 0;
        b.ntasks = tail * nstripes;
        e = hrs::launch_bytewise(b, s);
        if (e != hipSuccess) return hip_fail(c, e, "bytewise launch");
      }
    }
    return HRS_OK;
  }
  // Shapes the register-resident kernels would take in several launches go to
  // the streaming kernel (each input read once, each output written once, up
  // to kMaxIn inputs per launch), and so do 13-16 inputs with 3+ outputs, where
  // holding all 16 rows costs the resident kernel its occupancy (RS(16,4)
  // encode 4.50 -> 3.03 ms; 1-2 outputs and <= 12 inputs stay resident, where
  // streaming measured equal or slower: profiles/r02/stream). HRS_STREAM=0
  // keeps the chunked launches, 2 streams every runtime-matrix launch.
  static const int stream_mode = [] {
    const char* e = getenv("HRS_STREAM");
    return e ? atoi(e) : 1;
  }();
  const bool stream_ok = stream_mode != 0;
  for (int o0 = 0; o0 < nout; o0 += hrs::kMaxOut) {
    const int no = std::min(hrs::kMaxOut, nout - o0);
    const int resident = hrs::runtime_in_chunk(no);
    const bool stream = stream_ok && mode == 0 && nwin > 0 &&
                        (nlive > resident || (nlive > 12 && no >= 3) || stream_mode == 2);
    const int chunk = stream ? hrs::kMaxIn : resident;
    for (int i0 = 0; i0 < nlive; i0 += chunk) {
      const int ni = std::min(chunk, nlive - i0);
      RowArgs a{};
      for (int i = 0; i < ni; ++i) a.in[i] = in_rows[live[i0 + i]];
      for (int o = 0; o < no; ++o) {
        a.out[o] = out_rows[o0 + o];
        for (int i = 0; i < ni; ++i) hrs::set_coef(a, o, i, m[(o0 + o) * nin + live[i0 + i]]);
      }
      a.in_stride = in_stride;
      a.out_stride = out_stride;
      a.nin = ni;
      a.nout = no;
      a.accumulate = i0 > 0;
      if (nwin > 0) {
        a.len = len;
        a.nwin = nwin;
        a.ntasks = nwin * nstripes;
        hipError_t e = stream ? hrs::launch_bitsliced_stream(a, s) : hrs::launch_bitsliced(a, s);
        if (e != hipSuccess) return hip_fail(c, e, "bitsliced launch");
        c->last_kernel = hrs::last_kernel();
      }
      if (tail > 0) {
        RowArgs b = a;
        for (int i = 0; i < ni; ++i) b.in[i] = a.in[i] + tail_off;
        for (int o = 0; o < no; ++o) b.out[o] = a.out[o] + tail_off;
        b.len = tail;
        b.nwin = 0;
        b.ntasks = tail * nstripes;
        hipError_t e = hrs::launch_bytewise(b, s);
        if (e != hipSuccess) return hip_fail(c, e, "bytewise launch");
        if (nwin == 0) c->last_kernel = hrs::last_kernel();  // the call's only kernel
      }
    }
  }
  return HRS_OK;
}

hrs_status ragged_valid_ok(hrs_codec* c, const uint32_t* valid, size_t len, size_t nstripes, bool* all_full) {
  if (len > UINT32_MAX) return fail(c, HRS_EINVAL, "ragged encode: len %zu exceeds 2^32 - 1", len);
  const size_t k = static_cast<size_t>(c->k);
  bool full = true;
  for (size_t s = 0; s < nstripes; ++s)
    for (size_t j = 0; j < k; ++j) {
      const uint32_t v = valid[s * k + j];
      if (v > len) return fail(c, HRS_EINVAL, "stripe %zu row %zu: valid %u exceeds len %zu", s, j, v, len);
      full &= v == len;
    }
  *all_full = full;
  return HRS_OK;
}

hrs_status run_ragged(hrs_codec* c, const uint8_t* const* in_rows, size_t in_stride, uint8_t* const* out_rows,
                      size_t out_stride, size_t len, size_t nstripes, const uint32_t* dvalid, hipStream_t s) {
  const int k = c->k, p = c->p;
  bool vec_ok = c->kernel_mode != 2 && static_encode_family(c) && k <= hrs::kMaxIn && p <= hrs::kMaxOut &&
                in_stride % 16 == 0 && out_stride % 16 == 0;
  for (int i = 0; i < k && vec_ok; ++i) vec_ok = aligned16(in_rows[i]);
  for (int o = 0; o < p && vec_ok; ++o) vec_ok = aligned16(out_rows[o]);
  uint64_t col0 = 0;  // columns the vector kernel has covered
  const uint64_t nwin = vec_ok ? len / hrs::kWindowBytes : 0;
  if (nwin > 0) {
    hrs::RaggedArgs a{};
    for (int i = 0; i < k; ++i) a.r.in[i] = in_rows[i];
    for (int o = 0; o < p; ++o) a.r.out[o] = out_rows[o];
    a.r.in_stride = in_stride;
    a.r.out_stride = out_stride;
    a.r.len = len;
    a.r.nwin = nwin;
    a.r.ntasks = nwin * nstripes;
    a.r.nin = k;
    a.r.nout = p;
    a.valid = dvalid;
    a.k = k;
    bool handled = false;
    const int family = c->kind == HRS_CODE_NRS ? hrs::kStaticCauchy : hrs::kStaticRs;
    const hipError_t e = hrs::launch_ragged_encode(family, k, p, a, s, &handled);
    if (e != hipSuccess) return hip_fail(c, e, "ragged encode launch");
    if (handled) {
      c->last_kernel = hrs::last_kernel();
      col0 = nwin * hrs::kWindowBytes;
    }
  }
  if (col0 == len) return HRS_OK;
  // the byte-granular kernel over columns [col0, len): outputs in chunks of
  // kMaxOut, inputs in chunks of kMaxIn (later chunks accumulate)
  const uint8_t* m = c->g.data();
  for (int o0 = 0; o0 < p; o0 += hrs::kMaxOut) {
    const int no = std::min(hrs::kMaxOut, p - o0);
    for (int i0 = 0; i0 < k; i0 += hrs::kMaxIn) {
      const int ni = std::min(hrs::kMaxIn, k - i0);
      hrs::RaggedArgs b{};
      for (int i = 0; i < ni; ++i) b.r.in[i] = in_rows[i0 + i];
      for (int o = 0; o < no; ++o) {
        b.r.out[o] = out_rows[o0 + o];
        for (int i = 0; i < ni; ++i) hrs::set_coef(b.r, o, i, m[(o0 + o) * k + i0 + i]);
      }
      b.r.in_stride = in_stride;
      b.r.out_stride = out_stride;
      b.r.len = len;
      b.r.ntasks = (len - col0) * nstripes;
      b.r.nin = ni;
      b.r.nout = no;
      b.r.accumulate = i0 > 0;
      b.valid = dvalid;
      b.col0 = col0;
      b.k = k;
      b.row0 = i0;
      const hipError_t e = hrs::launch_ragged_bytewise(b, s);
      if (e != hipSuccess) return hip_fail(c, e, "ragged bytewise launch");
      if (col0 == 0) c->last_kernel = hrs::last_kernel();  // the call's only kernel
    }
  }
  return HRS_OK;
}

}  // namespace hrs::api

using namespace hrs::api;

extern "C" {

hrs_status hrs_encode_dev(hrs_codec* c, const uint8_t* const* in_rows, size_t in_stride, uint8_t* const* out_rows,
                          size_t out_stride, size_t len, size_t nstripes, void* stream) {
  if (!c) return HRS_EINVAL;
  if (!in_rows || !out_rows) return fail(c, HRS_EINVAL, "row arrays are NULL");
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  return run_apply(c, c->g.data(), c->p, c->k, in_rows, in_stride, out_rows, out_stride, len, nstripes,
                   static_cast<hipStream_t>(stream), static_encode_family(c));
}

hrs_status hrs_encode_ragged_dev(hrs_codec* c, const uint8_t* const* in_rows, size_t in_stride,
                                 uint8_t* const* out_rows, size_t out_stride, size_t len, size_t nstripes,
                                 const uint32_t* valid, void* stream) {
  if (!c) return HRS_EINVAL;
  if (!in_rows || !out_rows || !valid) return fail(c, HRS_EINVAL, "row arrays or valid are NULL");
  if (len == 0 || nstripes == 0) return HRS_OK;
  bool all_full = false;
  hrs_status st = ragged_valid_ok(c, valid, len, nstripes, &all_full);
  if (st != HRS_OK) return st;
  for (int i = 0; i < c->k; ++i)
    if (!in_rows[i]) return fail(c, HRS_EINVAL, "input row %d is NULL", i);
  for (int o = 0; o < c->p; ++o)
    if (!out_rows[o]) return fail(c, HRS_EINVAL, "output row %d is NULL", o);
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (ragged_takes_plain(c, all_full))
    return run_apply(c, c->g.data(), c->p, c->k, in_rows, in_stride, out_rows, out_stride, len, nstripes, hs,
                     static_encode_family(c));
  hrs_codec::BatchSlot* slot = nullptr;
  st = upload(c, valid, nstripes * static_cast<size_t>(c->k) * sizeof(uint32_t), valid, 0, hs, &slot);
  if (st != HRS_OK) return st;
  st = run_ragged(c, in_rows, in_stride, out_rows, out_stride, len, nstripes,
                  reinterpret_cast<const uint32_t*>(slot->dev), hs);
  slot_used(slot, hs);
  return st;
}

hrs_status hrs_decode_dev(hrs_codec* c, const uint8_t* const* rows, size_t in_stride, uint8_t* const* out_rows,
                          size_t out_stride, const int* erased, int ne, const int* ntr, int nn, size_t len,
                          size_t nstripes, void* stream) {
  if (!c) return HRS_EINVAL;
  if (!rows || ne < 0 || nn < 0 || (ne > 0 && (!out_rows || !erased)) || (nn > 0 && !ntr))
    return fail(c, HRS_EINVAL, "bad decode arguments");
  if (ne == 0 && c->kind == HRS_CODE_RS) return HRS_OK;
  std::vector<uint8_t> tmp;
  const uint8_t* d = nullptr;
  hrs_status st = decode5_matrix(c, erased, ne, ntr, nn, rows, tmp, &d);
  if (st != HRS_OK) return st;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  return run_apply(c, d, ne, c->n, rows, in_stride, out_rows, out_stride, len, nstripes,
                   static_cast<hipStream_t>(stream), false);
}

hrs_status hrs_apply_dev(hrs_codec* c, const uint8_t* m, int nout, int nin, const uint8_t* const* in_rows,
                         size_t in_stride, uint8_t* const* out_rows, size_t out_stride, size_t len, size_t nstripes,
                         void* stream) {
  if (!c) return HRS_EINVAL;
  if (!m || !in_rows || !out_rows || nout < 1 || nin < 1 || nout > 255 || nin > 255)
    return fail(c, HRS_EINVAL, "bad apply arguments");
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  return run_apply(c, m, nout, nin, in_rows, in_stride, out_rows, out_stride, len, nstripes,
                   static_cast<hipStream_t>(stream), false);
}

}  // extern "C"
