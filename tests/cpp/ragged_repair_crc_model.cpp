// CPU model of the ragged repair + CRC-32 fold
// (lambdafs_amd/csrc/hrs_batch_ragged_crc.hip), with the tables and the
// field algebra of crc32.hpp (mulmod, xpow8, unpad: the text the fold kernel
// compiles) and checked against zlib over EXACTLY the cell's first v bytes,
// with no zero fill behind them (Decoder.java:360-369).
//
//  fused form (batch_ragged_crc_kernel): one raw word per 2 KiB window of the
//    rebuilt cell; a boundary window's words are masked (mask_row) before the
//    CRC sees them, so its word is that of the live bytes followed by zeros up
//    to 2 KiB; a dead window has NO word (the model poisons it: a fold that
//    reads one fails). The fold joins the ceil(v / 2 KiB) leading words
//    right-aligned over the lanes and takes the padding off: unpad by
//    ceil(v / 2 KiB) * 2 KiB - v.
//  window form (crc_ragged_window_kernel over the outputs): 32 KiB windows and
//    the right-aligned tail window, bytes at or beyond v read as zero, a dead
//    window's word is 0; the fold joins all of them and unpads by len - v.
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
static const int64_t SUB = 2048;                               // the repair kernels' window
static const int64_t W = static_cast<int64_t>(kWindowBytes);  // the window kernel's 32 KiB
static const uint32_t POISON = 0xA5A5A5A5u;                    // a raw word no kernel wrote

static uint32_t slice4(uint32_t y) {
  return sl.s[3].t[y & 255] ^ sl.s[2].t[(y >> 8) & 255] ^ sl.s[1].t[(y >> 16) & 255] ^ sl.s[0].t[y >> 24];
}
static uint32_t piece_crc(const uint32_t* w) {
  uint32_t c = 0;
  for (int j = 0; j < 4; ++j) c = slice4(c ^ w[j]);
  return c;
}
static uint32_t lane_tree(const std::vector<std::vector<uint32_t>>& z, uint32_t* c) {
  for (int lvl = 0; lvl < 6; ++lvl) {
    uint32_t n[64];
    for (int l = 0; l < 64; ++l) n[l] = zmul(z[lvl], c[l]) ^ (l + (1 << lvl) < 64 ? c[l + (1 << lvl)] : 0);
    for (int l = 0; l < 64; ++l) c[l] = n[l];
  }
  return c[0];
}

static void mask_row(uint32_t* w, int lane, uint32_t nbytes) {
  for (int i = 0; i < 8; ++i) {
    const int at = (i < 4 ? 0 : 1024) + lane * 16 + (i & 3) * 4;
    const int d = static_cast<int>(nbytes) - at;
    w[i] &= d >= 4 ? 0xFFFFFFFFu : d <= 0 ? 0u : (1u << (8 * d)) - 1u;
  }
}

// batch_ragged_crc_fold_kernel: the tables are those of (len, win), G windows
// per lane by len's window count; a cell folds its `nw` leading words
// right-aligned (and the tail window's word after them when `tail`), then
// unpads. *reads counts the raw words looked at.
static uint32_t fold(const std::vector<uint32_t>& raw, uint64_t len, uint64_t win, uint64_t nw, bool tail, uint32_t v,
                     uint32_t total, uint32_t crc_in, std::vector<int>* reads) {
  if (v == 0) return crc_in;  // continues over no bytes; raw is not read
  const uint64_t G = (len / win + 63) / 64;
  const auto zw = tab(win), ztail = tab(len % win);
  std::vector<std::vector<uint32_t>> ft;
  for (int t = 0; t < 6; ++t) ft.push_back(tab(win * G << t));
  uint32_t c[64];
  const int64_t pad = (int64_t)G * 64 - (int64_t)nw;
  for (int l = 0; l < 64; ++l) {
    c[l] = 0;
    for (uint64_t g = 0; g < G; ++g) {
      const int64_t w = (int64_t)l * G + g - pad;
      if (w >= 0) {
        c[l] = zmul(zw, c[l]) ^ raw[w];
        ++(*reads)[w];
      }
    }
  }
  uint32_t r = lane_tree(ft, c);
  if (tail) {
    r = zmul(ztail, r) ^ raw[nw];
    ++(*reads)[nw];
  }
  return unpad(crc_in, r, total, total - v);
}

// The fused kernel's raw words of one rebuilt cell: dead windows keep the poison.
static std::vector<uint32_t> fused_raw(const uint8_t* p, uint64_t len, uint32_t v) {
  const uint64_t nwin = len / SUB;
  std::vector<uint32_t> raw(nwin, POISON);
  for (uint64_t w = 0; w < nwin; ++w) {
    const uint32_t lo = static_cast<uint32_t>(w * SUB);
    const uint32_t d = v > lo ? v - lo : 0u;
    const uint32_t live = d < SUB ? d : SUB;
    if (!live) continue;  // no store, no lookups, no raw word
    uint32_t crc[64];
    for (int lane = 0; lane < 64; ++lane) {
      uint32_t x[8];
      for (int i = 0; i < 8; ++i) {
        const uint8_t* q = p + lo + (i < 4 ? 0 : 1024) + lane * 16 + (i & 3) * 4;  // registers: the whole window
        x[i] = q[0] | q[1] << 8 | q[2] << 16 | (uint32_t)q[3] << 24;
      }
      if (live < SUB) mask_row(x, lane, live);
      crc[lane] = zmul(zchunk, piece_crc(x)) ^ piece_crc(x + 4);
    }
    raw[w] = lane_tree(tree, crc);
  }
  return raw;
}

// crc_ragged_window_kernel's raw word of window w (w == nwin: the right-aligned tail window).
static uint32_t window_raw_to(const uint8_t* p, uint64_t w, uint64_t nwin, uint64_t len, uint64_t v) {
  const bool full = w < nwin;
  const int64_t end = full ? (int64_t)((w + 1) * W) : (int64_t)len;
  const int64_t lo = full ? (int64_t)(w * W) : (int64_t)(nwin * W);
  const int64_t hi = std::min<int64_t>((int64_t)v, end);
  if (hi <= lo) return 0u;
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
  return lane_tree(tree, c);
}

// ragged_repair_inputs.length_classes(L); for cells of more than 64 windows
// also the 63-66-window lengths, where a lane of the fold holds two windows
static std::vector<uint32_t> length_classes(uint64_t L) {
  std::set<uint32_t> s;
  for (uint64_t v : {0ul, 1ul, 15ul, 16ul, 17ul, 1024ul, 1025ul, 2047ul, 2048ul, 2049ul, (unsigned long)L - 1,
                     (unsigned long)L})
    s.insert(static_cast<uint32_t>(std::min<uint64_t>(v, L)));
  if (L > 64 * SUB)
    for (uint64_t n : {63ul, 64ul, 65ul, 66ul})
      for (int64_t d : {-1, 0, 1}) s.insert(static_cast<uint32_t>(std::min<uint64_t>(n * SUB + d, L)));
  return std::vector<uint32_t>(s.begin(), s.end());
}

int main() {
  for (int t = 0; t < 6; ++t) tree.push_back(tab((uint64_t)kPieceBytes << t));
  int bad = 0, cases = 0, stray_reads = 0, algebra = 0;
  // the algebra against the matrices: x * x^-1 = 1, x^(8n) is Z_n, x^(-8n) undoes it
  if (mulmod(kOne >> 1, kXInv) != kOne) ++algebra;
  for (uint32_t n : {0u, 1u, 2u, 80u, 2047u, 2048u, 32768u, 135168u, 135248u, 0xFFFFFFFFu})
    for (uint32_t c : {1u, 0x80000000u, 0xDEADBEEFu, 0x12345678u}) {
      if (mulmod(xpow8(n), c) != apply(zeros(n), c)) ++algebra;
      if (mulmod(xpow8(n, true), mulmod(xpow8(n), c)) != c) ++algebra;
    }
  uint64_t seed = 17;
  auto fill = [&](std::vector<uint8_t>& d) {  // non-zero bytes throughout: a byte at or beyond v that is used shows
    for (auto& x : d) x = (uint8_t)(1 + ((seed = seed * 6364136223846793005ull + 1442695040888963407ull) >> 56) % 255);
  };
  for (uint64_t len : {4096ul, 4176ul, 66ul * 2048, 66ul * 2048 + 80}) {
    std::vector<uint8_t> d(len);
    fill(d);
    for (uint32_t v : length_classes(len))
      for (uint32_t crc_in : {0u, 0xDEADBEEFu}) {
        const uint32_t ref = (uint32_t)crc32(crc_in, d.data(), v);
        if (len % SUB == 0) {  // the fused form: whole 2 KiB windows
          const auto raw = fused_raw(d.data(), len, v);
          const uint64_t nw = (v + SUB - 1) / SUB;
          std::vector<int> reads(raw.size() + 1, 0);
          const uint32_t out = fold(raw, len, SUB, nw, false, v, (uint32_t)(nw * SUB), crc_in, &reads);
          for (size_t w = 0; w < raw.size(); ++w)
            if (reads[w] && raw[w] == POISON) ++stray_reads;
          ++cases;
          if (out != ref) {
            ++bad;
            printf("fused len %zu v %u crc_in %08x: model %08x zlib %08x\n", (size_t)len, v, crc_in, out, ref);
          }
        }
        {  // the window form, with its right-aligned tail window
          const uint64_t nwin = len / W, tail = len % W;
          std::vector<uint32_t> raw(nwin + 1, POISON);
          for (uint64_t w = 0; w < nwin + (tail ? 1 : 0); ++w) raw[w] = window_raw_to(d.data(), w, nwin, len, v);
          std::vector<int> reads(raw.size(), 0);
          const uint32_t out = fold(raw, len, W, nwin, tail != 0, v, (uint32_t)len, crc_in, &reads);
          for (size_t w = 0; w < raw.size(); ++w)
            if (reads[w] && raw[w] == POISON) ++stray_reads;
          ++cases;
          if (out != ref) {
            ++bad;
            printf("window len %zu v %u crc_in %08x: model %08x zlib %08x\n", (size_t)len, v, crc_in, out, ref);
          }
        }
      }
  }
  printf("{\"ragged_repair_crc_model_cases\": %d, \"mismatches\": %d, \"unwritten_words_read\": %d, "
         "\"algebra_failures\": %d}\n",
         cases, bad, stray_reads, algebra);
  return bad || stray_reads || algebra ? 1 : 0;
}
