// Ragged encode (hrs_ragged.hip): encodeBulk over data cells of which only
// the leading valid[s * k + j] bytes hold data and the rest reads as zeros
// (include/hrs.h, "ragged encode"). Kernel arguments and launchers.
#pragma once
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

}  // namespace hrs
