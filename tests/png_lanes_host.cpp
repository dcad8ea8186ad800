// The per-lane code of the PNG encoder (swem_amd/csrc/png_core.h) run on the host: the 64 lanes of a wavefront as a loop, the
// shuffles of csrc/png.hip as plain sums.  tests/test_png_host.py compiles this as ordinary C++, runs it and reads the files back
// with tests/png_ref.py, so that the token codes, the bit writer, the CRC combine and the Adler sums are checked without a GPU.
//   png_lanes_host maps.raw T H W palette.raw|- out_prefix      ->  out_prefix.<t>.png
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "png_core.h"

typedef unsigned char u8;
static uint32_t tab[256];

static void lane_range(int lane, unsigned n, unsigned *a0, unsigned *a1) {
  const unsigned piece = (n + 63) / 64;
  *a0 = lane * piece < n ? lane * piece : n;
  *a1 = *a0 + piece < n ? *a0 + piece : n;
}

static uint32_t wave_crc(const u8 *pre, int npre, const u8 *data, unsigned n) {
  uint32_t x = 0;
  for (int lane = 0; lane < 64; ++lane) {
    unsigned a0, a1;
    lane_range(lane, n, &a0, &a1);
    uint32_t st = lane == 0 ? png_crc_run(tab, 0xffffffffu, pre, npre) : 0u;
    st = png_crc_run(tab, st, data + a0, a1 - a0);
    x ^= png_crc_shift(st, n - a1);
  }
  return ~x;
}

static void chunk(std::vector<u8> &f, const char *type, const u8 *extra, int nextra, const u8 *data, unsigned n) {
  u8 pre[8], b[4];
  memcpy(pre, type, 4);
  if (nextra) memcpy(pre + 4, extra, nextra);
  png_be32(b, n + nextra);
  f.insert(f.end(), b, b + 4);
  f.insert(f.end(), pre, pre + 4 + nextra);
  f.insert(f.end(), data, data + n);
  png_be32(b, wave_crc(pre, 4 + nextra, data, n));
  f.insert(f.end(), b, b + 4);
}

int main(int argc, char **argv) {
  if (argc != 7) return 2;
  const int T = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]);
  const bool has_palette = strcmp(argv[5], "-") != 0;
  std::vector<u8> maps((size_t)T * H * W);
  u8 pal[768];
  FILE *fp = fopen(argv[1], "rb");
  if (!fp || fread(maps.data(), 1, maps.size(), fp) != maps.size()) return 3;
  fclose(fp);
  if (has_palette) {
    fp = fopen(argv[5], "rb");
    if (!fp || fread(pal, 1, 768, fp) != 768) return 3;
    fclose(fp);
  }
  for (int k = 0; k < 256; ++k) tab[k] = png_crc_entry(k);
  const int rw = W + 1, seg_rows = 65535 / rw < 16 ? 65535 / rw : 16, nseg = (H + seg_rows - 1) / seg_rows;
  for (int t = 0; t < T; ++t) {
    std::vector<u8> file;
    const u8 sig[8] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10};
    file.insert(file.end(), sig, sig + 8);
    u8 ih[13];
    png_be32(ih, W);
    png_be32(ih + 4, H);
    ih[8] = 8;
    ih[9] = has_palette ? 3 : 0;
    ih[10] = ih[11] = ih[12] = 0;
    chunk(file, "IHDR", 0, 0, ih, 13);
    if (has_palette) chunk(file, "PLTE", 0, 0, pal, 768);
    unsigned long long A = 1, B = 0;
    for (int s = 0; s < nseg; ++s) {
      const int row0 = s * seg_rows, rows = H - row0 < seg_rows ? H - row0 : seg_rows, n = rows * rw;
      std::vector<u8> seg(n);
      for (int r = 0; r < rows; ++r) {
        seg[r * rw] = 0;
        memcpy(&seg[r * rw + 1], &maps[((size_t)t * H + row0 + r) * W], W);
      }
      unsigned start[64], bits = 0;
      unsigned long long sa = 0, sw = 0;
      for (int lane = 0; lane < 64; ++lane) {
        unsigned p0, p1;
        lane_range(lane, n, &p0, &p1);
        PngCountSink c = {0};
        png_tokens(seg.data(), (int)p0, (int)p1, c);
        start[lane] = bits;
        bits += c.bits + (lane == 0 ? 3 : 0);
        unsigned long long a, w;
        png_adler_piece(seg.data() + p0, (int)(p1 - p0), &a, &w);
        sa += a;
        sw += w + a * (unsigned long long)(n - p1);
      }
      const unsigned coded = (bits + 10 + 7) / 8 + 4, stored = n + 5;
      std::vector<uint32_t> words((stored + 3) / 4 + 1, 0xa5a5a5a5u);      // (not zero: the encoder must zero what it ORs into)
      u8 *out = (u8 *)words.data();
      unsigned len;
      if (coded < stored) {
        len = coded;
        for (unsigned w = 0; w < (coded + 3) / 4; ++w) words[w] = 0;
        for (int lane = 0; lane < 64; ++lane) {
          unsigned p0, p1;
          lane_range(lane, n, &p0, &p1);
          PngBitSink b;
          b.open(words.data(), start[lane]);
          if (lane == 0) {
            const PngTok fixed_block = {2u, 3};
            b.put(fixed_block);
          }
          png_tokens(seg.data(), (int)p0, (int)p1, b);
          b.close();
        }
        png_or_byte(words.data(), coded - 2, 0xff);
        png_or_byte(words.data(), coded - 1, 0xff);
      } else {
        len = stored;
        out[0] = 0;
        out[1] = (u8)n;
        out[2] = (u8)(n >> 8);
        out[3] = (u8)~n;
        out[4] = (u8)(~n >> 8);
        memcpy(out + 5, seg.data(), n);
      }
      const u8 zlib_header[2] = {0x78, 0x01};
      chunk(file, "IDAT", zlib_header, s == 0 ? 2 : 0, out, len);
      B = (B + (unsigned long long)n * A + sw % PNG_ADLER_MOD) % PNG_ADLER_MOD;
      A = (A + sa % PNG_ADLER_MOD) % PNG_ADLER_MOD;
    }
    u8 fin[9] = {1, 0, 0, 0xff, 0xff};
    png_be32(fin + 5, (uint32_t)((B << 16) | A));
    chunk(file, "IDAT", 0, 0, fin, 9);
    chunk(file, "IEND", 0, 0, fin, 0);
    char name[4096];
    snprintf(name, sizeof name, "%s.%d.png", argv[6], t);
    fp = fopen(name, "wb");
    if (!fp || fwrite(file.data(), 1, file.size(), fp) != file.size()) return 4;
    fclose(fp);
  }
  return 0;
}
