// Ragged encode (hrs_ragged.hip): encodeBulk over data cells of which only
// the leading valid[s * k + j] bytes hold data and the rest reads as zeros
// (include/hrs.h, "ragged encode"). Kernel arguments and launchers.
#pragma once
#include "hrs_crc.hpp"
#include "hrs_internal.hpp"

namespace hrs {

struct RaggedArgs {
  RowArgs r;              // the encode's rows, strides and geometry (cw, accumulate: byte-granular kernel only)
  const uint32_t* valid;  // device table: input i of stripe s holds valid[s * k + row0 + i] leading data bytes
  uint64_t col0;          // byte-granular: first column covered; r.ntasks = nstripes * (r.len - col0)
  int k;                  // table words per stripe
  int row0;               // byte-granular: the launch's first input row (input chunking)
};

// encode_ragged_kernel<K, P> over the whole 2 KiB windows of a static shape
// (family as for launch_static_encode); *handled = false for any other shape.
hipError_t launch_ragged_encode(int family, int k, int p, const RaggedArgs& a, hipStream_t s, bool* handled);
// encode_ragged_bytewise_kernel over columns [col0, len): any code, shape and alignment.
hipError_t launch_ragged_bytewise(const RaggedArgs& a, hipStream_t s);

// Ragged encode + CRC-32 in one pass (hrs_ragged_crc.hip): the fused encode +
// CRC's launch `e` (hrs_crc.hpp: windows of e.subs 2 KiB sub-windows, raw
// layout [stripe][row][window], rows = [data 0..k-1, parity 0..p-1]) with the
// data rows cut at valid[s * k + j] (DEVICE words, at the launch's first
// stripe). *handled = false when (family, k, p) has no such kernel.
struct EncodeRaggedCrcArgs {
  EncodeCrcArgs e;
  const uint32_t* valid;
};
hipError_t launch_encode_ragged_crc(int family, int k, int p, const EncodeRaggedCrcArgs& a, int cus, hipStream_t s,
                                    bool* handled);

// The window pass of the two-pass route: launch_crc_windows' launch `w` over
// rows of which row w.row0 + r, when below k, reads as zero from
// valid[s * k + w.row0 + r] on (DEVICE words); the other rows are full.
struct RaggedCrcWinArgs {
  CrcWinArgs w;
  const uint32_t* valid;
  int k;
  int pad_;
};
hipError_t launch_crc_ragged_windows(const RaggedCrcWinArgs& a, bool aligned, int cus, hipStream_t s);

}  // namespace hrs
