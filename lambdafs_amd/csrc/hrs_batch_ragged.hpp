// Ragged repair batches (hrs_batch_ragged.hip): hrs_decode_batch_dev over
// cells of which only the leading bytes hold data (include/hrs.h, "ragged
// repair"). Kernel arguments and launchers.
#pragma once
#include "hrs_crc.hpp"
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

// ---- ragged repair + CRC-32 (hrs_batch_ragged_crc.hip)

// batch_ragged_crc_kernel: the ragged launch `r` (whole 2 KiB windows) with
// the raw CRC of every LIVE output window, taken from the registers (the
// boundary window's words masked from the boundary on), in
// raw[(stripe * rows_per_stripe + output) * r.b.nwin + window]. A dead output
// window gets no raw word. Shapes: batch_ragged_crc_shape.
struct BatchRaggedCrcArgs {
  BatchRaggedArgs r;
  uint32_t* raw;
  const uint32_t* tables;  // kCrcLdsWordsA words (device)
  int rows_per_stripe;     // the caller's max_erased
  int pad_;
};
// The fused shapes, those of batch_decode_crc_kernel: 1-4 outputs, at most 12
// live inputs (8 at 4 outputs).
inline bool batch_ragged_crc_shape(int max_nout, int max_nin) {
  return max_nout >= 1 && max_nout <= 4 && max_nin >= 1 && max_nin <= (max_nout == 4 ? 8 : 12);
}
hipError_t launch_batch_ragged_crc(const BatchRaggedCrcArgs& d, int max_nout, int max_nin, int cus, hipStream_t s);

// batch_ragged_crc_fold_kernel: the fold of a ragged batch's raw words, each
// cell over its own length v = lens[stripe * words + nin_words + t] (the
// plan-order table's output words; 0 for t >= max_nout). f as for
// launch_crc_fold with f.nsr = stripes * rows_per_stripe and the tables of
// (len, win). fused (win = 2 KiB): the ceil(v / 2 KiB) leading words of a cell
// exist and the last one is padded to 2 KiB; else (win = 32 KiB, the window
// pass) all words exist and the row is padded to len. A cell of length 0
// yields crc_in (0 when NULL) without reading raw, so crc_out may alias crc_in.
struct BatchRaggedCrcFoldArgs {
  CrcFoldArgs f;
  const uint32_t* lens;  // device table, at the launch's first stripe
  int words, nin_words;
  int max_nout, rows_per_stripe;
  uint32_t len;
  int fused;
};
hipError_t launch_batch_ragged_crc_fold(const BatchRaggedCrcFoldArgs& b, int cus, hipStream_t s);

}  // namespace hrs
