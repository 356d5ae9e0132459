// Device helpers of the ragged encode + CRC kernels (hrs_ragged_crc.hip): the
// scalar read of a stripe's valid words and the mask of the one window that
// holds a cell's boundary. hrs_ragged.hip keeps its own copies of the two: its
// code object, and the line numbers its resource report prints, stay as they
// were. window_live and store_row_below are the ragged repair's
// (hrs_batch_ragged.hip), shared with its CRC form (hrs_batch_ragged_crc.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hrs_device.hpp"

namespace hrs {

// A word every lane of the wave reads from one address: constant address
// space (the table does not change under the kernel) and a uniform address, so
// the load is scalar and the value lives in an SGPR.
typedef __attribute__((address_space(4))) const uint32_t c_u32;

__device__ __forceinline__ uint32_t uniform_word(const uint32_t* p) {
  return __builtin_amdgcn_readfirstlane(*reinterpret_cast<c_u32*>(uniform_addr(p)));
}

// Clears the bytes at or beyond `nbytes` (0 < nbytes < 2 KiB) of the lane's
// words of a window (load_row's layout: words 0-3 at 16 lane, 4-7 1 KiB later).
__device__ __forceinline__ void mask_row(uint32_t (&w)[8], int lane, uint32_t nbytes) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int at = (i < 4 ? 0 : 1024) + lane * 16 + (i & 3) * 4;
    const int d = static_cast<int>(nbytes) - at;  // data bytes of this word
    w[i] &= d >= 4 ? 0xFFFFFFFFu : d <= 0 ? 0u : (1u << (8 * d)) - 1u;
  }
}

// Bytes of a cell of length v inside the window [lo, lo + 2 KiB): 0 dead,
// 2048 full, else the boundary.
__device__ __forceinline__ uint32_t window_live(uint32_t v, uint32_t lo) {
  const uint32_t d = v > lo ? v - lo : 0u;
  return d < kWindowBytes ? d : kWindowBytes;
}

// store_row of the bytes below `nbytes` (0 < nbytes < 2 KiB) of the window: a
// lane's 16-byte piece wholly below the boundary goes out as a vector, the one
// straddling piece as whole words and then single bytes of exactly the bytes
// below it (no read-modify-write), a piece at or beyond it not at all.
__device__ __forceinline__ void store_row_below(uint8_t* p, int lane, const uint32_t (&w)[8], uint32_t nbytes) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int at = h * 1024 + lane * 16;
    const int nb = static_cast<int>(nbytes) - at;  // bytes of this piece below the boundary
    uint8_t* q = p + at;
    if (nb >= 16) {
      const u32x4 x = {w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
      __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(q));
    } else if (nb > 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rem = nb - 4 * j;
        const uint32_t x = w[4 * h + j];
        if (rem >= 4) {
          *reinterpret_cast<uint32_t*>(q + 4 * j) = x;
        } else {
#pragma unroll
          for (int b = 0; b < 3; ++b)
            if (b < rem) q[4 * j + b] = static_cast<uint8_t>(x >> (8 * b));
        }
      }
    }
  }
}

}  // namespace hrs
