// CPU model of the ragged encode + CRC kernels' CRC side
// (lambdafs_amd/csrc/hrs_ragged_crc.hip), with the tables of crc32.hpp and
// checked against zlib over the zero-filled cell: a data cell holds `valid`
// leading bytes and reads as zeros behind them, whatever its storage holds.
//
//  fused form (encode_ragged_crc_kernel): windows of `subs` 2 KiB sub-windows;
//    lane l holds the 16-byte pieces at 16 l and 1024 + 16 l of a sub-window;
//    a boundary sub-window's words are masked (mask_row) before the CRC sees
//    them; a dead sub-window does no lookups and advances the lane's chain by
//    two Z_1024 steps, unless the row has been dead since the window's first
//    sub-window (the chain is 0 and stays 0); a window wholly behind `valid`
//    yields raw 0; the fold (crc_fold_kernel) joins the raw words with
//    Z_window and chains from crc_in with Z_len.
//  window form (crc_ragged_window_kernel): 32 KiB windows and the
//    right-aligned tail window, bytes at or beyond `valid` read as zero, a
//    window wholly behind it yields raw 0 without a look at the bytes; the
//    fold adds the tail window with Z_tail.
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../lambdafs_amd/csrc/crc32.hpp"

using namespace hrs::crc;

static uint32_t zmul(const std::vector<uint32_t>& z, uint32_t c) {
  return z[c & 255] ^ z[256 + ((c >> 8) & 255)] ^ z[512 + ((c >> 16) & 255)] ^ z[768 + (c >> 24)];
}
static std::vector<uint32_t> tab(uint64_t n) {
  std::vector<uint32_t> t(1024);
  to_tables(zeros(n), t.data());
  return t;
}

static const Slice4 sl = make_slice4();
static const std::vector<uint32_t> zchunk = tab(kChunkBytes);
static std::vector<std::vector<uint32_t>> tree;
static const int64_t SUB = 2048;                                // a sub-window: the encode kernels' task
static const int64_t W = static_cast<int64_t>(kWindowBytes);   // the window kernel's 32 KiB

static uint32_t slice4(uint32_t y) {
  return sl.s[3].t[y & 255] ^ sl.s[2].t[(y >> 8) & 255] ^ sl.s[1].t[(y >> 16) & 255] ^ sl.s[0].t[y >> 24];
}
static uint32_t piece_crc(const uint32_t* w) {
  uint32_t c = 0;
  for (int j = 0; j < 4; ++j) c = slice4(c ^ w[j]);
  return c;
}
static uint32_t lane_tree(uint32_t* c) {
  for (int lvl = 0; lvl < 6; ++lvl) {
    uint32_t n[64];
    for (int l = 0; l < 64; ++l) n[l] = zmul(tree[lvl], c[l]) ^ (l + (1 << lvl) < 64 ? c[l + (1 << lvl)] : 0);
    for (int l = 0; l < 64; ++l) c[l] = n[l];
  }
  return c[0];
}

// mask_row: the lane's 8 words of a sub-window with the bytes at or beyond nbytes cleared
static void mask_row(uint32_t* w, int lane, uint32_t nbytes) {
  for (int i = 0; i < 8; ++i) {
    const int at = (i < 4 ? 0 : 1024) + lane * 16 + (i & 3) * 4;
    const int d = static_cast<int>(nbytes) - at;
    w[i] &= d >= 4 ? 0xFFFFFFFFu : d <= 0 ? 0u : (1u << (8 * d)) - 1u;
  }
}

// crc_fold_kernel: nwin raw words of `win`-byte windows, the tail window's word after them.
static uint32_t fold(const std::vector<uint32_t>& raw, uint64_t nwin, uint64_t win, uint64_t tail, uint64_t len,
                     uint32_t crc_in) {
  const uint64_t G = (nwin + 63) / 64;
  const auto zw = tab(win), ztail = tab(tail), zlen = tab(len);
  std::vector<std::vector<uint32_t>> ft;
  for (int t = 0; t < 6; ++t) ft.push_back(tab(win * G << t));
  uint32_t c[64];
  const int64_t pad = (int64_t)G * 64 - (int64_t)nwin;
  for (int l = 0; l < 64; ++l) {
    c[l] = 0;
    for (uint64_t g = 0; g < G; ++g) {
      const int64_t w = (int64_t)l * G + g - pad;
      if (w >= 0) c[l] = zmul(zw, c[l]) ^ raw[w];
    }
  }
  for (int lvl = 0; lvl < 6; ++lvl) {
    uint32_t n[64];
    for (int l = 0; l < 64; ++l) n[l] = zmul(ft[lvl], c[l]) ^ (l + (1 << lvl) < 64 ? c[l + (1 << lvl)] : 0);
    for (int l = 0; l < 64; ++l) c[l] = n[l];
  }
  uint32_t r = c[0];
  if (tail) r = zmul(ztail, r) ^ raw[nwin];
  return zmul(zlen, crc_in ^ 0xFFFFFFFFu) ^ r ^ 0xFFFFFFFFu;
}

// The fused kernel's raw words of one data row; *dead_nonzero counts dead windows whose word is not 0.
static std::vector<uint32_t> fused_raw(const uint8_t* p, uint64_t len, uint32_t valid, int subs, int* dead_nonzero) {
  const uint64_t nwin = len / (subs * SUB);
  std::vector<uint32_t> raw(nwin);
  for (uint64_t w = 0; w < nwin; ++w) {
    const uint32_t win_lo = static_cast<uint32_t>(w * subs * SUB);
    uint32_t crc[64];
    for (int lane = 0; lane < 64; ++lane) crc[lane] = 0;
    for (int sub = 0; sub < subs; ++sub) {
      const uint32_t lo = win_lo + sub * SUB;
      const uint32_t d = valid > lo ? valid - lo : 0u;
      const uint32_t live = d < SUB ? d : SUB;
      for (int lane = 0; lane < 64; ++lane) {
        if (live) {
          uint32_t x[8];
          for (int i = 0; i < 8; ++i) {
            const uint8_t* q = p + lo + (i < 4 ? 0 : 1024) + lane * 16 + (i & 3) * 4;  // loaded whole, then masked
            x[i] = q[0] | q[1] << 8 | q[2] << 16 | (uint32_t)q[3] << 24;
          }
          if (live < SUB) mask_row(x, lane, live);
          crc[lane] = zmul(zchunk, zmul(zchunk, crc[lane]) ^ piece_crc(x)) ^ piece_crc(x + 4);
        } else if (valid > win_lo) {  // dead after a live sub-window of this window
          crc[lane] = zmul(zchunk, zmul(zchunk, crc[lane]));
        }  // dead since the window's start: the chain is 0 and stays 0
      }
    }
    raw[w] = lane_tree(crc);
    if (valid <= win_lo && raw[w] != 0) ++*dead_nonzero;
  }
  return raw;
}

// The window kernel's raw word of window w (w == nwin: the right-aligned tail window).
static uint32_t window_raw_to(const uint8_t* p, uint64_t w, uint64_t nwin, uint64_t len, uint64_t valid, bool* looked) {
  const bool full = w < nwin;
  const int64_t end = full ? (int64_t)((w + 1) * W) : (int64_t)len;
  const int64_t lo = full ? (int64_t)(w * W) : (int64_t)(nwin * W);
  const int64_t hi = std::min<int64_t>((int64_t)valid, end);
  *looked = hi > lo;
  if (hi <= lo) return 0u;  // raw 0, no load
  uint32_t c[64];
  for (int lane = 0; lane < 64; ++lane) {
    uint32_t x = 0;
    for (int q = 0; q < kPieces; ++q) {
      uint32_t ch = 0;
      for (int j = 0; j < 4; ++j) {
        uint32_t word = 0;
        for (int b = 0; b < 4; ++b) {
          const int64_t pos = end - W + (int64_t)q * kChunkBytes + lane * kPieceBytes + 4 * j + b;
          if (pos >= lo && pos < hi) word |= (uint32_t)p[pos] << (8 * b);
        }
        ch = slice4(ch ^ word);
      }
      x = q == 0 ? ch : (zmul(zchunk, x) ^ ch);
    }
    c[lane] = x;
  }
  return lane_tree(c);
}

// ragged_inputs.valid_classes(L), plus the 32 KiB window's own boundaries
static std::vector<uint32_t> valid_classes(uint64_t L) {
  std::set<uint32_t> s;
  for (uint64_t v : {0ul, 1ul, 15ul, 16ul, 17ul, 1023ul, 1024ul, 1025ul, 2047ul, 2048ul, 2049ul, 4095ul, 4096ul,
                     (unsigned long)L - 1, (unsigned long)L, 6144ul, 30720ul, 32767ul, 32768ul, 32769ul})
    s.insert(static_cast<uint32_t>(std::min<uint64_t>(v, L)));
  return std::vector<uint32_t>(s.begin(), s.end());
}

int main() {
  for (int t = 0; t < 6; ++t) tree.push_back(tab((uint64_t)kPieceBytes << t));
  int bad = 0, cases = 0, dead_nonzero = 0, dead_looked = 0;
  uint64_t seed = 11;
  auto fill = [&](std::vector<uint8_t>& d) {  // non-zero bytes throughout: a byte behind `valid` that is used shows
    for (auto& x : d) x = (uint8_t)(1 + ((seed = seed * 6364136223846793005ull + 1442695040888963407ull) >> 56) % 255);
  };
  auto reference = [](const std::vector<uint8_t>& d, uint32_t valid, uint32_t crc_in) {
    std::vector<uint8_t> z(d);
    std::fill(z.begin() + valid, z.end(), 0);
    return (uint32_t)crc32(crc_in, z.data(), (uInt)z.size());
  };
  // the fused form: whole sub-windows; subs 16 needs whole 32 KiB windows
  struct Fused { uint64_t len; int subs; };
  for (const Fused f : {Fused{4096, 1}, Fused{4096, 2}, Fused{32768, 16}, Fused{65536, 16}, Fused{65536, 2}}) {
    std::vector<uint8_t> d(f.len);
    fill(d);
    for (uint32_t valid : valid_classes(f.len))
      for (uint32_t crc_in : {0u, 0xDEADBEEFu}) {
        const auto raw = fused_raw(d.data(), f.len, valid, f.subs, &dead_nonzero);
        const uint32_t out = fold(raw, raw.size(), f.subs * SUB, 0, f.len, crc_in);
        const uint32_t ref = reference(d, valid, crc_in);
        ++cases;
        if (out != ref) {
          ++bad;
          printf("fused len %zu subs %d valid %u crc_in %08x: model %08x zlib %08x\n", (size_t)f.len, f.subs, valid,
                 crc_in, out, ref);
        }
      }
  }
  // the window form, with its right-aligned tail window
  for (uint64_t len : {4096ul, 4096ul + 80, 32768ul + 80, 65536ul}) {
    std::vector<uint8_t> d(len);
    fill(d);
    const uint64_t nwin = len / W, tail = len % W;
    for (uint32_t valid : valid_classes(len))
      for (uint32_t crc_in : {0u, 0x1234567u}) {
        std::vector<uint32_t> raw(nwin + 1);
        for (uint64_t w = 0; w < nwin + (tail ? 1 : 0); ++w) {
          bool looked = false;
          raw[w] = window_raw_to(d.data(), w, nwin, len, valid, &looked);
          const uint64_t first = w < nwin ? w * W : nwin * W;
          if (valid <= first && (looked || raw[w] != 0)) ++dead_looked;
        }
        const uint32_t out = fold(raw, nwin, W, tail, len, crc_in);
        const uint32_t ref = reference(d, valid, crc_in);
        ++cases;
        if (out != ref) {
          ++bad;
          printf("window len %zu valid %u crc_in %08x: model %08x zlib %08x\n", (size_t)len, valid, crc_in, out, ref);
        }
      }
  }
  printf("{\"ragged_crc_model_cases\": %d, \"mismatches\": %d, \"dead_windows_nonzero\": %d, \"dead_windows_read\": %d}\n",
         cases, bad, dead_nonzero, dead_looked);
  return bad || dead_nonzero || dead_looked ? 1 : 0;
}
