// Internal interface of the CRC-32 kernels (hrs_crc.hip, hrs_fused.hip) for hrs_dispatch.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "crc32.hpp"
#include "hrs_internal.hpp"

namespace hrs {

constexpr int kCrcWindow = static_cast<int>(crc::kWindowBytes);  // bytes per wave task (32 KiB)
constexpr int kCrcRep = 32;          // slicing tables replicated: lane l reads copy l % 32 (its own bank)
// slicing image word of (table j, entry e, copy c); layout: hrs_device.hpp slice4
constexpr int crc_slice_word(int j, int e, int c) { return (j >> 1) * 16384 + e * 64 + (j & 1) * 32 + c; }
constexpr int kCrcGroup = 8;         // chunks loaded and chained together (ILP)
constexpr int kCrcBlockThreads = 1024;  // 16 waves share one table image per CU
constexpr int kCrcMaxRows = 32;      // rows per window launch
constexpr int kCrcSliceWords = 4 * 256 * kCrcRep;           // 128 KiB
constexpr int kCrcLdsWordsA = kCrcSliceWords + 7 * 1024;    // + Z_1024, Z_{16*2^t} t = 0..5 (156 KiB)
constexpr int kCrcLdsWordsB = 9 * 1024;                     // Z_window, 6 tree levels, Z_tail, Z_len (36 KiB)
constexpr int kCrcFoldBlocksPerCU = 3;

// The LDS image of the window kernels (crc_window_kernel, the fused encode +
// CRC), built on the host and uploaded once per handle: the slicing-by-4
// tables (kCrcRep bank-private copies; table j = a byte followed by j more
// bytes of its word, i.e. the zlib slicing tables T8_0..T8_3), then Z_chunk
// (joins a lane's successive pieces, `chunk` bytes apart) and the lane tree
// Z_{piece * 2^t}, t = 0..5 (lane l + 2^t is piece * 2^t bytes later).
// tests/cpp/crc_tables dumps it for tests/test_crc_tables.py.
inline std::vector<uint32_t> crc_window_image(uint64_t piece, uint64_t chunk) {
  std::vector<uint32_t> h(kCrcLdsWordsA);
  const crc::Slice4 sl = crc::make_slice4();
  for (int j = 0; j < 4; ++j)
    for (int v = 0; v < 256; ++v)
      for (int r = 0; r < kCrcRep; ++r) h[crc_slice_word(j, v, r)] = sl.s[j].t[v];
  crc::to_tables(crc::zeros(chunk), &h[kCrcSliceWords]);
  for (int t = 0; t < 6; ++t) crc::to_tables(crc::zeros(piece << t), &h[kCrcSliceWords + (1 + t) * 1024]);
  return h;
}

struct CrcWinArgs {
  const uint8_t* rows[kCrcMaxRows];
  int nrows;        // rows in this launch
  int row0;         // index of rows[0] among all rows of the call
  int nrows_total;  // rows of the call (raw layout [stripe][row][window])
  int order;        // window -> wave order (task_order), set at launch
  uint64_t stride[kCrcMaxRows];  // bytes between stripes, per row
  uint64_t len;
  uint64_t nwin;    // full windows per row
  uint64_t tail;    // len - nwin * kCrcWindow
  uint64_t nstripes;
  uint32_t* raw;
  const uint32_t* tables;  // kCrcLdsWordsA words (device)
};

struct CrcFoldArgs {
  const uint32_t* raw;
  uint64_t nwin;
  uint64_t tail;
  uint64_t nsr;    // nstripes * nrows
  int G;           // full windows per lane: ceil(nwin / 64)
  int pad_;
  const uint32_t* tables;  // kCrcLdsWordsB words (device), built for this len
  const uint32_t* crc_in;  // nullable
  uint32_t* crc_out;
};

hipError_t launch_crc_windows(const CrcWinArgs& a, bool aligned, int cus, hipStream_t s);
hipError_t launch_crc_fold(const CrcFoldArgs& a, int cus, hipStream_t s);

// Fused encode + CRC-32 (hrs_fused.hip): one wave per (stripe, window of
// `subs` 2 KiB sub-windows: 32 KiB for large jobs, smaller when a job has too
// few 32 KiB windows to fill the chip) encodes the window's sub-windows and
// keeps the raw CRC of every data and parity row of the window, in the window
// kernel's decomposition (lane pieces joined with Z_1024, lanes with
// Z_{16*2^t}), so crc_fold_kernel finishes them with Z_window tables. Raw
// layout [stripe][row][window], rows = [data 0..k-1, parity 0..p-1].
constexpr int kFusedMaxK = 16;
constexpr int kFusedMaxP = 4;
struct EncodeCrcArgs {
  const uint8_t* in[kFusedMaxK];
  uint8_t* out[kFusedMaxP];
  uint64_t in_stride;
  uint64_t out_stride;
  uint64_t nwin;      // windows per row (len / (subs * 2 KiB), len a multiple)
  uint64_t nstripes;
  uint32_t subs;      // 2 KiB sub-windows per window: 1, 2, 4, 8 or 16
  uint32_t rep_mask;  // slicing-table copy of lane l = l & rep_mask (kCrcRep - 1; HRS_CRC_REP A/B)
  int order;          // window -> wave order (task_order), set at launch
  int pad_;
  uint32_t* raw;
  const uint32_t* tables;  // kCrcLdsWordsA words (device)
};

// family: kStaticRs / kStaticCauchy (hrs_internal.hpp). *handled = false when
// (family, k, p) has no fused kernel (the caller runs encode, then CRC).
hipError_t launch_encode_crc(int family, int k, int p, const EncodeCrcArgs& a, int cus, hipStream_t s,
                             bool* handled);

// Fused repair + CRC-32 (hrs_decode_crc.hip): the runtime-matrix apply of
// `r` (whole 2 KiB windows: r.nwin = len / 2 KiB, no accumulate) with the raw
// CRC of every output's window in raw[stripe][output][window]
// (crc_fold_kernel finishes them with 2 KiB windows). *handled = false for
// shapes without a fused kernel (> 4 outputs, > 12 inputs, > 8 at 4 outputs).
struct DecodeCrcArgs {
  RowArgs r;
  uint32_t* raw;
  const uint32_t* tables;  // kCrcLdsWordsA words (device)
};
hipError_t launch_decode_crc(const DecodeCrcArgs& d, int cus, hipStream_t s, bool* handled);

// Fused heterogeneous repair batch + CRC-32 (hrs_batch_crc.hip): the batch
// launch `b` (whole 2 KiB windows; b.ntasks = b.nwin * stripes) with the raw
// CRC of every PRESENT output's window in
// raw[(stripe * rows_per_stripe + output) * nwin + window]; rows_per_stripe is
// the caller's max_erased, so (stripe, output) indexes crc_out. Outputs past a
// stripe's losses get no raw word. Shapes: max_nout 1-4, max_nin <= 12 (<= 8
// at 4 outputs); anything else is hipErrorInvalidValue (the host checks first).
struct BatchCrcArgs {
  BatchArgs b;
  uint32_t* raw;
  const uint32_t* tables;  // kCrcLdsWordsA words (device)
  int rows_per_stripe;
  int pad_;
};
hipError_t launch_batch_decode_crc(const BatchCrcArgs& d, int max_nout, int max_nin, int cus, hipStream_t s);

// The fold of a batch's raw window CRCs: f as for launch_crc_fold with
// f.nsr = stripes * rows_per_stripe; pair (s, t) with t >= plans[pat[s]].nout
// yields crc_in (0 when NULL) without reading raw, so crc_out may alias crc_in.
struct BatchCrcFoldArgs {
  CrcFoldArgs f;
  const BatchPlan* plans;  // device table
  const int32_t* pat;      // device: pattern index of each stripe
  int rows_per_stripe;
  int pad_;
};
hipError_t launch_batch_crc_fold(const BatchCrcFoldArgs& b, int cus, hipStream_t s);

// Fused scrub / heal + CRC-32 (hrs_scrub_crc.hip): scrub_kernel's walk over
// whole 2 KiB windows (ntasks = nwin * stripes, 16-byte aligned rows and
// stride) with the raw CRC of every location's window in
// raw[(stripe * n + l) * nwin + window], hops order (crc_fold_kernel finishes
// them with 2 KiB windows). Shapes: 2 <= p <= kScrubCrcMaxP and
// n <= kScrubCrcMaxRows; anything else is hipErrorInvalidValue (the host
// checks first).
// heal: the kernel also writes the resolved columns back and lists every task
// in which it stored a byte in `dirty` (dirty[0] = how many, zeroed by the
// caller; dirty[1 + i] = task; room for ntasks). launch_scrub_crc_redo, after
// it on the same stream, rewrites the raw words of the listed windows from
// the bytes as they are then.
constexpr int kScrubCrcMaxRows = 16;
constexpr int kScrubCrcMaxP = 4;
struct ScrubCrcArgs {
  const uint8_t* rows[kScrubCrcMaxRows];  // location l of stripe s at rows[l] + s * stride
  uint64_t stride;
  uint64_t nwin;     // 2 KiB windows per row (len / 2 KiB, len a multiple)
  uint64_t ntasks;   // nstripes * nwin
  uint32_t* reports;  // initialised (launch_scrub_init); stripe s at reports + s * report_stride
  uint64_t report_stride;
  uint32_t* raw;
  const uint32_t* tables;  // kCrcLdsWordsA words (device)
  uint64_t* dirty;         // heal only
  int n, p;
  int order;  // window -> wave order (task_order), set at launch
  int pad_;
};
hipError_t launch_scrub_crc(const ScrubCrcArgs& a, bool heal, int cus, hipStream_t s);
hipError_t launch_scrub_crc_redo(const ScrubCrcArgs& a, int cus, hipStream_t s);

// Fused heal with known erasures + CRC-32 (hrs_heal_erased_crc.hip):
// heal_erased_kernel's walk with the raw window CRCs of ScrubCrcArgs, same
// shapes. Every window with a bad column is listed in c.dirty (zeroed by the
// caller), and launch_scrub_crc_redo(c) after it rewrites those windows' words.
struct ErasePattern;  // hrs_heal_erased.hpp
struct HealErasedCrcArgs {
  ScrubCrcArgs c;            // rows are written: erased cells filled, survivors patched
  const ErasePattern* pats;  // device table
  const int32_t* pat;        // device: pattern index of each stripe
};
hipError_t launch_heal_erased_crc(const HealErasedCrcArgs& a, int cus, hipStream_t s);

}  // namespace hrs
