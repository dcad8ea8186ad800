// The lane code of the PNG encoder's second form (swem_amd/csrc/png_core.h: symbol tokeniser, histogram / bit-count / code
// sinks, the length builder, canonical codes, the dynamic block header, the scanline filters) run on the host: the 64 lanes of
// png_encode_px_kernel (csrc/png.hip) as a loop, its shuffles as plain sums.  tests/test_png_dyn_host.py compiles this as
// ordinary C++ and reads the files back with tests/png_ref_px.py; tests/test_gpu_png_dyn.py compares the device's files with
// these byte for byte.
//   png_dyn_host encode pixels.raw T H W channels palette.raw|- fixed|dynamic out_prefix   ->  out_prefix.<t>.png
//   png_dyn_host lengths maxbits f0 f1 ...                                                  ->  the code lengths, one line
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

static int lengths_mode(int argc, char **argv) {
  const int maxbits = atoi(argv[2]), n = argc - 3;
  if (n < 1 || n > PNG_NSYM || maxbits < 1 || maxbits > PNG_MAXBITS) return 2;
  std::vector<uint32_t> freq(n);
  for (int i = 0; i < n; ++i) freq[i] = (uint32_t)strtoul(argv[3 + i], 0, 10);
  std::vector<u8> len(n);
  static PngBuildScratch S;
  png_code_lengths(freq.data(), n, maxbits, len.data(), &S);
  for (int i = 0; i < n; ++i) printf("%d%c", len[i], i + 1 < n ? ' ' : '\n');
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 4 && strcmp(argv[1], "lengths") == 0) return lengths_mode(argc, argv);
  if (argc != 10 || strcmp(argv[1], "encode") != 0) return 2;
  const int T = atoi(argv[3]), H = atoi(argv[4]), W = atoi(argv[5]), channels = atoi(argv[6]);
  const bool has_palette = strcmp(argv[7], "-") != 0;
  const bool dynamic = strcmp(argv[8], "dynamic") == 0;
  if ((channels != 1 && channels != 3) || (channels == 3 && has_palette) || (!dynamic && strcmp(argv[8], "fixed") != 0)) return 2;
  const int rb = channels * W, rw = rb + 1;
  if (T < 1 || H < 1 || W < 1 || rw > 65535) return 2;
  std::vector<u8> px((size_t)T * H * rb);
  u8 pal[768];
  FILE *fp = fopen(argv[2], "rb");
  if (!fp || fread(px.data(), 1, px.size(), fp) != px.size()) return 3;
  fclose(fp);
  if (has_palette) {
    fp = fopen(argv[7], "rb");
    if (!fp || fread(pal, 1, 768, fp) != 768) return 3;
    fclose(fp);
  }
  for (int k = 0; k < 256; ++k) tab[k] = png_crc_entry(k);
  const int seg_rows = 65535 / rw < 16 ? 65535 / rw : 16, nseg = (H + seg_rows - 1) / seg_rows;
  // what the kernel keeps in LDS behind the segment
  static uint32_t freq[288], hdr[PNG_HDR_WORDS];
  static uint16_t code[288];
  static u8 len[288];
  static PngBuildScratch S;
  for (int t = 0; t < T; ++t) {
    std::vector<u8> file;
    const u8 sig[8] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10};
    file.insert(file.end(), sig, sig + 8);
    u8 ih[13];
    png_be32(ih, W);
    png_be32(ih + 4, H);
    ih[8] = 8;
    ih[9] = channels == 3 ? 2 : (has_palette ? 3 : 0);
    ih[10] = ih[11] = ih[12] = 0;
    chunk(file, "IHDR", 0, 0, ih, 13);
    if (has_palette) chunk(file, "PLTE", 0, 0, pal, 768);
    unsigned long long A = 1, B = 0;
    for (int s = 0; s < nseg; ++s) {
      const int row0 = s * seg_rows, rows = H - row0 < seg_rows ? H - row0 : seg_rows, n = rows * rw;
      std::vector<u8> seg(n);
      const u8 *src = px.data() + ((size_t)t * H + row0) * rb;
      for (int r = 0; r < rows; ++r) {
        const u8 *cur = src + (size_t)r * rb;
        int type = 0;
        if (channels == 3) {
          const u8 *up = row0 + r > 0 ? cur - rb : 0;
          PngFilterSums sums = {{0u, 0u, 0u, 0u, 0u}};
          for (int lane = 0; lane < 64; ++lane) png_filter_sums(cur, up, lane, 64, rb, 3, &sums);
          type = png_filter_choice(sums);
          for (int lane = 0; lane < 64; ++lane) png_filter_row(type, cur, up, lane, 64, rb, 3, &seg[r * rw]);
        } else {
          memcpy(&seg[r * rw + 1], cur, W);
        }
        seg[r * rw] = (u8)type;
      }
      unsigned p0[64], p1[64], mine_f[64], mine_d[64], start_f[64], start_d[64], hdr_bits = 0, eob_d = 0;
      for (int lane = 0; lane < 64; ++lane) lane_range(lane, n, &p0[lane], &p1[lane]);
      if (dynamic) {
        memset(freq, 0, sizeof freq);
        memset(len, 0, sizeof len);
        memset(hdr, 0, sizeof hdr);
        for (int lane = 0; lane < 64; ++lane) {
          PngHistSink hist = {freq};
          png_symbols(seg.data(), (int)p0[lane], (int)p1[lane], hist);
        }
        png_count_one(freq + PNG_EOB);
        int used = 0;
        for (int i = 0; i < PNG_NSYM; ++i)
          if (freq[i]) {
            S.order[png_rank(freq, PNG_NSYM, i)] = (uint16_t)i;
            ++used;
          }
        png_lengths_sorted(freq, S.order, used, PNG_MAXBITS, len, &S);
        png_canonical(len, PNG_NSYM, code, &S);
        hdr_bits = png_dynamic_header(len, hdr, &S);
        eob_d = len[PNG_EOB];
      }
      unsigned bits_f = 0, bits_d = 0;
      unsigned long long sa = 0, sw = 0;
      for (int lane = 0; lane < 64; ++lane) {
        if (dynamic) {
          PngFixedCountSink cf = {0u};
          PngLenCountSink cd = {len, 1u, 0u};
          PngBothSinks<PngFixedCountSink, PngLenCountSink> both = {cf, cd};
          png_symbols(seg.data(), (int)p0[lane], (int)p1[lane], both);
          mine_f[lane] = cf.bits;
          mine_d[lane] = cd.bits + (lane == 0 ? hdr_bits : 0u);
        } else {
          PngCountSink c = {0u};
          png_tokens(seg.data(), (int)p0[lane], (int)p1[lane], c);
          mine_f[lane] = c.bits;
          mine_d[lane] = 0;
        }
        mine_f[lane] += lane == 0 ? 3u : 0u;
        start_f[lane] = bits_f;
        start_d[lane] = bits_d;
        bits_f += mine_f[lane];
        bits_d += mine_d[lane];
        unsigned long long a, w;
        png_adler_piece(seg.data() + p0[lane], (int)(p1[lane] - p0[lane]), &a, &w);
        sa += a;
        sw += w + a * (unsigned long long)(n - p1[lane]);
      }
      const unsigned coded_f = (bits_f + 7 + 3 + 7) / 8 + 4, coded_d = (bits_d + eob_d + 3 + 7) / 8 + 4;
      const bool use_d = dynamic && coded_d < coded_f;
      const unsigned coded = use_d ? coded_d : coded_f, stored = n + 5;
      std::vector<uint32_t> words((stored + 3) / 4 + 1, 0xa5a5a5a5u);      // (not zero: the encoder must zero what it ORs into)
      u8 *out = (u8 *)words.data();
      unsigned outlen;
      if (coded < stored) {
        outlen = coded;
        for (unsigned w = 0; w < (coded + 3) / 4; ++w) words[w] = 0;
        if (use_d) {
          for (unsigned w = 0; w < (hdr_bits + 31) / 32; ++w) png_or_word(words.data() + w, hdr[w]);
          for (int lane = 0; lane < 64; ++lane) {
            PngCodeSink b;
            b.code = code;
            b.len = len;
            b.out.open(words.data(), start_d[lane] + (lane == 0 ? hdr_bits : 0u));
            png_symbols(seg.data(), (int)p0[lane], (int)p1[lane], b);
            if (lane == 63) b.literal(PNG_EOB);
            b.out.close();
          }
        } else {
          for (int lane = 0; lane < 64; ++lane) {
            PngBitSink b;
            b.open(words.data(), start_f[lane]);
            if (lane == 0) {
              const PngTok fixed_block = {2u, 3};
              b.put(fixed_block);
            }
            png_tokens(seg.data(), (int)p0[lane], (int)p1[lane], b);
            b.close();
          }
        }
        png_or_byte(words.data(), coded - 2, 0xff);
        png_or_byte(words.data(), coded - 1, 0xff);
      } else {
        outlen = stored;
        out[0] = 0;
        out[1] = (u8)n;
        out[2] = (u8)(n >> 8);
        out[3] = (u8)~n;
        out[4] = (u8)(~n >> 8);
        memcpy(out + 5, seg.data(), n);
      }
      const u8 zlib_header[2] = {0x78, 0x01};
      chunk(file, "IDAT", zlib_header, s == 0 ? 2 : 0, out, outlen);
      B = (B + (unsigned long long)n * A + sw % PNG_ADLER_MOD) % PNG_ADLER_MOD;
      A = (A + sa % PNG_ADLER_MOD) % PNG_ADLER_MOD;
    }
    u8 fin[9] = {1, 0, 0, 0xff, 0xff};
    png_be32(fin + 5, (uint32_t)((B << 16) | A));
    chunk(file, "IDAT", 0, 0, fin, 9);
    chunk(file, "IEND", 0, 0, fin, 0);
    char name[4096];
    snprintf(name, sizeof name, "%s.%d.png", argv[9], t);
    fp = fopen(name, "wb");
    if (!fp || fwrite(file.data(), 1, file.size(), fp) != file.size()) return 4;
    fclose(fp);
  }
  return 0;
}
