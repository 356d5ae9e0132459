// Ragged repair batches (hrs_batch_ragged.hip): hrs_decode_batch_dev over
// cells of which only the leading bytes hold data (include/hrs.h, "ragged
// repair"). Kernel arguments and launchers.
#pragma once
#include "hrs_internal.hpp"

namespace hrs {

// The batch launch `b` plus the per-call length table, in PLAN order: stripe i
// of the launch owns lens[i * words ..): nin_words survivor lengths in the
// order of its plan's inputs (loc[0], loc[1], ...; 0 past the plan's nin),
// then the lengths of its outputs (0 past the plan's nout). A zero length is a
// dead row, so the slots a plan does not use need no test of their own.
struct BatchRaggedArgs {
  BatchArgs b;
  const uint32_t* lens;  // device table, at the launch's first stripe
  int words;             // table words per stripe (nin_words + output words)
  int nin_words;         // the batch's max_nin
};

// Vector shapes of batch_ragged_kernel<NOUT, NINB>: max_nout <= 4, max_nin <= 16.
inline bool batch_ragged_vector_shape(int max_nout, int max_nin) {
  return max_nout >= 1 && max_nout <= 4 && max_nin >= 1 && max_nin <= 16;
}

// batch_ragged_kernel over the whole 2 KiB windows (b.nwin per row);
// hipErrorInvalidValue outside batch_ragged_vector_shape.
hipError_t launch_batch_ragged(const BatchRaggedArgs& a, int max_nout, int max_nin, hipStream_t s);
// batch_ragged_bytewise_kernel over columns [b.col0, b.len): any shape and alignment.
hipError_t launch_batch_ragged_bytewise(const BatchRaggedArgs& a, hipStream_t s);

}  // namespace hrs
