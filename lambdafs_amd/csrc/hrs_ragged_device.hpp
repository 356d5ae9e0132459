// Device helpers of the ragged encode + CRC kernels (hrs_ragged_crc.hip): the
// scalar read of a stripe's valid words and the mask of the one window that
// holds a cell's boundary. hrs_ragged.hip keeps its own copies of the two: its
// code object, and the line numbers its resource report prints, stay as they
// were.
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

}  // namespace hrs
