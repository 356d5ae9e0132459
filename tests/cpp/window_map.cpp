// The window map of the static encode and the runtime-matrix repairs
// (lambdafs_amd/csrc/hrs_window_map.hpp) enumerated on the CPU: for every row
// of nwin in [0, 600] whole windows and every half distance H in
// {1 KiB (contiguous), 2 KiB ... 256 KiB, 512 KiB, 1 MiB}, all tasks' two
// 1 KiB pieces must cover [0, nwin * 2 KiB) exactly once, none may cross the
// row end, H = 1 KiB must give today's offsets (w * 2 KiB and 1 KiB later),
// strided windows must lie where the map's definition puts them, and a row
// shorter than 2H must be all contiguous. Also the parser of the
// HRS_WINDOW_SPLIT values. Plain host code: prints one JSON line, exit 0 = ok.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../lambdafs_amd/csrc/hrs_window_map.hpp"

int main() {
  long cases = 0, bad_cover = 0, bad_bounds = 0, bad_contig = 0, bad_def = 0, bad_parse = 0;
  for (int split = 0; split <= 10; ++split) {
    const uint64_t H = uint64_t{1024} << split;
    if (hrs::split_of_bytes(static_cast<int64_t>(H)) != split) ++bad_parse;
    for (uint64_t nwin = 0; nwin <= 600; ++nwin) {
      ++cases;
      const uint64_t row = nwin * 2048, npieces = nwin * 2;
      const uint64_t groups = row / (2 * H), per_group = H / 1024;
      std::vector<uint8_t> hits(npieces, 0);
      for (uint64_t w = 0; w < nwin; ++w) {
        const hrs::WindowPos p = hrs::window_pos(w, nwin, split);
        const uint64_t a = p.off, b = p.off + p.half;
        if (a % 1024 || b % 1024 || a + 1024 > row || b + 1024 > row) {
          ++bad_bounds;
          continue;
        }
        ++hits[a / 1024];
        ++hits[b / 1024];
        if (split == 0 && (a != w * 2048 || p.half != 1024)) ++bad_contig;
        if (w < groups * per_group) {  // the definition: window c of group g
          const uint64_t g = w / per_group, c = w % per_group;
          if (a != g * 2 * H + c * 1024 || p.half != H) ++bad_def;
        } else if (a != w * 2048 || p.half != 1024) {  // the rest, and rows shorter than 2H
          ++bad_contig;
        }
      }
      for (uint64_t i = 0; i < npieces; ++i)
        if (hits[i] != 1) ++bad_cover;
    }
  }
  const int64_t rejected[] = {0, -1024, 1, 512, 1023, 1025, 3072, 65535, 65537, 98304, (1 << 20) + 1, 1 << 21, int64_t{1} << 40};
  for (int64_t v : rejected)
    if (hrs::split_of_bytes(v) != -1) ++bad_parse;
  std::printf(
      "{\"window_map_cases\": %ld, \"bad_cover\": %ld, \"bad_bounds\": %ld, \"bad_contiguous\": %ld, "
      "\"bad_definition\": %ld, \"bad_parse\": %ld}\n",
      cases, bad_cover, bad_bounds, bad_contig, bad_def, bad_parse);
  return (bad_cover | bad_bounds | bad_contig | bad_def | bad_parse) ? 1 : 0;
}
