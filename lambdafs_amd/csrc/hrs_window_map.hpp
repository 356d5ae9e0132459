// The window map of the plain static encode and the runtime-matrix repairs:
// where in its row a wave task's two 1 KiB pieces lie. Plain integer code, no
// device intrinsics: the kernels, the probe, the launchers and the CPU test
// (tests/cpp/window_map.cpp) all include it.
//
// A window is 2 KiB of a row, moved as two coalesced 1 KiB wave accesses
// `half` bytes apart. With half = 1 KiB the window is contiguous (the map of
// every other kernel family). With half = H > 1 KiB (a power of two), the
// row's leading floor(nwin * 2 KiB / 2H) groups of 2H bytes are strided:
// window c of group g covers [g 2H + c KiB, +1 KiB) and the same H further
// on, so the H / 1 KiB windows of a group tile it exactly. The windows after
// the last whole group stay contiguous; a row shorter than 2H has no group.
// The map is a bijection of the row's 1 KiB pieces onto (window, piece): loads
// and stores go through the same offsets, so accumulate launches and in-place
// callers see the bytes they wrote.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HRS_HD __host__ __device__ __forceinline__
#else
#define HRS_HD inline
#endif

namespace hrs {

constexpr uint32_t kPieceBytes = 1024;       // one wave access: 64 lanes x 16 B
constexpr uint32_t kSplitMinBytes = 1024;    // contiguous windows
constexpr uint32_t kSplitMaxBytes = 1 << 20;

struct WindowPos {
  uint64_t off;   // row offset of the window's first piece
  uint32_t half;  // bytes from the first piece to the second
};

// split = log2(H / 1 KiB): 0 = contiguous windows.
HRS_HD WindowPos window_pos(uint64_t w, uint64_t nwin, int split) {
  const uint64_t strided = (nwin >> split) << split;  // windows in whole groups
  if (w >= strided) return {w * (2 * kPieceBytes), kPieceBytes};
  const uint64_t g = w >> split;
  const uint64_t c = w - (g << split);
  return {(g << (split + 11)) + c * kPieceBytes, kPieceBytes << split};
}

// log2(H / 1 KiB) of a half distance in bytes; -1 unless H is a power of two
// in [1 KiB, 1 MiB].
HRS_HD int split_of_bytes(int64_t h) {
  if (h < kSplitMinBytes || h > kSplitMaxBytes || (h & (h - 1)) != 0) return -1;
  int s = 0;
  while ((int64_t{kPieceBytes} << s) < h) ++s;
  return s;
}

}  // namespace hrs
