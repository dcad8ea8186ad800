// The per-lane pieces of the PNG encoder (png.hip), written so that a host compiler takes them too: the token codes of
// RFC 1951 section 3.2.6, the bit writer, CRC-32 with its x^(8n) combine, the Adler-32 piece sums; for the second form the
// symbol tokeniser and its sinks, the length-limited code-length builder, canonical codes and the dynamic block header of
// sections 3.2.2 and 3.2.7, and the scanline filters.  Nothing here knows about wavefronts; png.hip joins the lanes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ __forceinline__
#else
#define PNG_HD inline
#endif

#define PNG_ADLER_MOD 65521u
#define PNG_CRC_POLY 0xEDB88320u /* CRC-32 of PNG / zlib, reflected */
#define PNG_MAX_MATCH 258
#define PNG_MIN_MATCH 3

// `n` bits of a token, least significant bit first in the stream
struct PngTok {
  uint32_t bits;
  int n;
};

// Huffman codes go into the stream most significant bit first: reverse the low n bits
PNG_HD uint32_t png_rev(uint32_t v, int n) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  v = (v >> 16) | (v << 16);
  return v >> (32 - n);
}

// fixed codes: literals 0..143 are the 8-bit codes 0x30.., 144..255 the 9-bit codes 0x190..
PNG_HD PngTok png_literal(uint32_t c) {
  PngTok t;
  if (c < 144u) {
    t.bits = png_rev(0x30u + c, 8);
    t.n = 8;
  } else {
    t.bits = png_rev(0x190u + (c - 144u), 9);
    t.n = 9;
  }
  return t;
}

// the length symbol (257..285) of a match of `len` (3..258) bytes, the number of its extra bits and their value
PNG_HD void png_length_symbol(int len, uint32_t *sym, uint32_t *nextra, uint32_t *extra) {
  *nextra = 0;
  *extra = 0;
  if (len == PNG_MAX_MATCH) {
    *sym = 285;
    return;
  }
  const uint32_t l = (uint32_t)(len - PNG_MIN_MATCH);        // 0..254
  if (l < 8u) {
    *sym = 257u + l;
  } else {
    const uint32_t e = (uint32_t)(31 - __builtin_clz(l)) - 2u; // 1..5 extra bits; four symbols per count
    *sym = 261u + 4u * e + ((l >> e) & 3u);
    *nextra = e;
    *extra = l & ((1u << e) - 1u);
  }
}

// a match of `len` (3..258) bytes at distance 1: the length symbol (257..279 are 7-bit codes 1.., 280..285 the 8-bit codes
// 0xC0..), its extra bits (least significant first), and distance code 0 = five zero bits
PNG_HD PngTok png_match(int len) {
  uint32_t sym, e, extra;
  png_length_symbol(len, &sym, &e, &extra);
  PngTok t;
  if (sym < 280u) {
    t.bits = png_rev(sym - 256u, 7) | (extra << 7);
    t.n = 7 + (int)e + 5;
  } else {
    t.bits = png_rev(0xC0u + (sym - 280u), 8) | (extra << 8);
    t.n = 8 + (int)e + 5;
  }
  return t;
}

// The tokens of bytes [p0, p1) of a segment `b`: a byte equal to its predecessor starts a match over the rest of its run (as far
// as the piece and 258 reach) when that is at least 3 bytes; everything else is a literal.  b[p0 - 1] belongs to another piece;
// the decoder has it by then.  Byte 0 of a segment never matches: segments are coded independently.
// png_symbols hands the sink `literal(c)` and `match(len)`; png_tokens hands it the tokens of the fixed codes.
template <class Sink>
PNG_HD void png_symbols(const unsigned char *b, int p0, int p1, Sink &sink) {
  int i = p0;
  while (i < p1) {
    const unsigned c = b[i];
    if (i > 0 && c == b[i - 1]) {
      const int lim = p1 - i < PNG_MAX_MATCH ? p1 - i : PNG_MAX_MATCH;
      int r = 1;
      while (r < lim && b[i + r] == c) ++r;
      if (r >= PNG_MIN_MATCH) {
        sink.match(r);
        i += r;
        continue;
      }
    }
    sink.literal(c);
    ++i;
  }
}

template <class Sink>
struct PngFixedCodes {
  Sink &sink;
  PNG_HD void literal(unsigned c) { sink.put(png_literal(c)); }
  PNG_HD void match(int len) { sink.put(png_match(len)); }
};

template <class Sink>
PNG_HD void png_tokens(const unsigned char *b, int p0, int p1, Sink &sink) {
  PngFixedCodes<Sink> fixed = {sink};
  png_symbols(b, p0, p1, fixed);
}

struct PngCountSink {
  uint32_t bits;
  PNG_HD void put(PngTok t) { bits += (uint32_t)t.n; }
};

PNG_HD void png_or_word(uint32_t *p, uint32_t v) {
  if (!v) return;
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);
#else
  *p |= v;
#endif
}

// Writes a lane's tokens from bit `start` of a ZEROED word buffer.  The first and the last word it touches may be shared with
// the neighbouring lanes and are OR-ed in; the words in between are its own.
struct PngBitSink {
  uint32_t *w;
  uint64_t acc;
  int nacc;
  bool head;
  PNG_HD void open(uint32_t *words, uint32_t start) {
    w = words + (start >> 5);
    acc = 0;
    nacc = (int)(start & 31u);
    head = true;
  }
  PNG_HD void put(PngTok t) {
    acc |= (uint64_t)t.bits << nacc;     // nacc < 32 and t.n <= 18
    nacc += t.n;
    if (nacc >= 32) {
      if (head)
        png_or_word(w, (uint32_t)acc);
      else
        *w = (uint32_t)acc;
      head = false;
      ++w;
      acc >>= 32;
      nacc -= 32;
    }
  }
  PNG_HD void close() {
    if (nacc > 0) png_or_word(w, (uint32_t)acc);
  }
};

PNG_HD void png_or_byte(uint32_t *words, uint32_t pos, uint32_t v) { png_or_word(words + (pos >> 2), v << (8u * (pos & 3u))); }

// ---- CRC-32
PNG_HD uint32_t png_crc_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? PNG_CRC_POLY ^ (c >> 1) : c >> 1;
  return c;
}
// the shift register (no pre- or post-inversion) over n bytes
PNG_HD uint32_t png_crc_run(const uint32_t *tab, uint32_t state, const unsigned char *p, size_t n) {
  for (size_t i = 0; i < n; ++i) state = tab[(state ^ p[i]) & 0xffu] ^ (state >> 8);
  return state;
}
// a * b mod P, polynomials over GF(2) in the reflected representation (bit 31 = x^0)
PNG_HD uint32_t png_gf2_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ PNG_CRC_POLY : b >> 1;
  }
  return p;
}
// what `nbytes` further bytes do to a register: register * x^(8 nbytes) mod P (the register is linear in its start value, so
// the registers of adjoining pieces, each started at 0, are shifted to the end of the message and XOR-ed)
PNG_HD uint32_t png_crc_shift(uint32_t state, uint32_t nbytes) {
  uint32_t r = state, base = 0x00800000u;      // x^8
  while (nbytes && r) {
    if (nbytes & 1u) r = png_gf2_mul(base, r);
    base = png_gf2_mul(base, base);
    nbytes >>= 1;
  }
  return r;
}

// ---- Adler-32 of a piece of n <= 65535 bytes: a = sum b[i], w = sum (n - i) * b[i]; both fit 64 bits with room
PNG_HD void png_adler_piece(const unsigned char *p, int n, unsigned long long *a, unsigned long long *w) {
  unsigned long long sa = 0, sw = 0;
  for (int i = 0; i < n; ++i) {
    sa += p[i];
    sw += (unsigned long long)(n - i) * p[i];
  }
  *a = sa;
  *w = sw;
}

PNG_HD void png_be32(unsigned char *p, uint32_t v) {
  p[0] = (unsigned char)(v >> 24);
  p[1] = (unsigned char)(v >> 16);
  p[2] = (unsigned char)(v >> 8);
  p[3] = (unsigned char)v;
}

// ---- dynamic Huffman tables (RFC 1951 sections 3.2.2 and 3.2.7).  Only distance 1 is ever emitted: the distance alphabet of
// a dynamic block is the single code 0 of length 1 (HDIST = 0), one zero bit per match; no distance tree is built.
#define PNG_NSYM 286         /* literal/length symbols */
#define PNG_EOB 256          /* end of block: always used, so a block has at least two symbols */
#define PNG_NCL 19           /* code-length symbols */
#define PNG_MAXBITS 15
#define PNG_CL_MAXBITS 7
#define PNG_PM_ITEMS (2 * PNG_NSYM - 2)
#define PNG_PM_WORDS ((PNG_PM_ITEMS + 31) / 32)
#define PNG_HDR_WORDS 132    /* 17 + 19 * 3 + 287 * (7 + 7) bits at the very most */

PNG_HD void png_count_one(uint32_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, 1u);
#else
  ++*p;
#endif
}

// the histogram of a piece's symbols (the end-of-block symbol is the caller's to add)
struct PngHistSink {
  uint32_t *freq;
  PNG_HD void literal(unsigned c) { png_count_one(freq + c); }
  PNG_HD void match(int len) {
    uint32_t sym, e, extra;
    png_length_symbol(len, &sym, &e, &extra);
    png_count_one(freq + sym);
  }
};

// the bits of a piece under a table of code lengths, a match's distance code taking `dist_bits`
struct PngLenCountSink {
  const unsigned char *len;
  uint32_t dist_bits;
  uint32_t bits;
  PNG_HD void literal(unsigned c) { bits += len[c]; }
  PNG_HD void match(int l) {
    uint32_t sym, e, extra;
    png_length_symbol(l, &sym, &e, &extra);
    bits += len[sym] + e + dist_bits;
  }
};

// the bits of a piece under the fixed codes
struct PngFixedCountSink {
  uint32_t bits;
  PNG_HD void literal(unsigned c) { bits += c < 144u ? 8u : 9u; }
  PNG_HD void match(int l) { bits += (uint32_t)png_match(l).n; }
};

// one pass of the tokeniser for two sinks
template <class A, class B>
struct PngBothSinks {
  A &a;
  B &b;
  PNG_HD void literal(unsigned c) {
    a.literal(c);
    b.literal(c);
  }
  PNG_HD void match(int l) {
    a.match(l);
    b.match(l);
  }
};

// writes a piece under a table of codes (already bit-reversed: png_canonical) and their lengths; a match is its length code,
// the extra bits, and the one zero bit of distance code 0
struct PngCodeSink {
  const uint16_t *code;
  const unsigned char *len;
  PngBitSink out;
  PNG_HD void literal(unsigned c) {
    const PngTok t = {code[c], (int)len[c]};
    out.put(t);
  }
  PNG_HD void match(int l) {
    uint32_t sym, e, extra;
    png_length_symbol(l, &sym, &e, &extra);
    const int n = (int)len[sym];
    const PngTok t = {(uint32_t)code[sym] | (extra << n), n + (int)e + 1};      // <= 15 + 5 + 1 bits
    out.put(t);
  }
};

// what the length builder and the header writer work in (LDS on the device)
struct PngBuildScratch {
  uint32_t w[2][PNG_PM_ITEMS];                 // the item weights of two adjoining levels of the package-merge
  uint32_t is_pkg[PNG_MAXBITS][PNG_PM_WORDS];  // per level and item: a package (1) or a leaf (0)
  uint32_t leaf[PNG_NSYM];                     // the used symbols' frequencies in ascending order
  uint32_t clfreq[PNG_NCL];
  uint32_t next[PNG_MAXBITS + 2];              // png_canonical: codes per length, then the next code of each length
  uint16_t order[PNG_NSYM];                   // the used symbols by (frequency, index)
  uint16_t cnt[PNG_MAXBITS];                   // items per level
  uint16_t clcode[PNG_NCL];
  unsigned char cllen[PNG_NCL];
};

// the place of symbol i (freq[i] > 0) among the used symbols ordered by (frequency, index): ties go by symbol index, so every
// order is the same on the host and on the device
PNG_HD int png_rank(const uint32_t *freq, int n, int i) {
  const uint32_t f = freq[i];
  int r = 0;
  for (int j = 0; j < n; ++j) {
    const uint32_t g = freq[j];
    r += (g != 0u && (g < f || (g == f && j < i))) ? 1 : 0;
  }
  return r;
}

PNG_HD uint32_t png_add_sat(uint32_t a, uint32_t b) {
  const uint32_t s = a + b;
  return s < a ? 0xffffffffu : s;
}

// Optimal code lengths of at most `maxbits` bits for the m used symbols order[0..m) (ascending frequency) by package-merge
// (Larmore and Hirschberg 1990): level 0 is the list of leaves; every further level merges the leaves with the packages (pairs
// of adjoining items) of the level before, a leaf going first where the weights tie; a list is cut at 2m - 2 items.  The first
// 2m - 2 items of the last level are the solution: a symbol's length is the number of levels at which its leaf is among the
// items taken, the packages taken at a level standing for twice as many items of the level before.  Leaves are taken in order,
// so a more frequent symbol never has a longer code, and for m >= 2 the Kraft sum is exactly 1.  `len` is added to: zero it
// first.  min(maxbits, m - 1) levels are run: no code of m symbols is longer than m - 1 bits, so the shorter limit leaves the
// optimum where it was.  Needs m <= 2^maxbits; sum(freq) * maxbits < 2^32 keeps every weight that can be taken exact (larger
// ones saturate).
PNG_HD void png_lengths_sorted(const uint32_t *freq, const uint16_t *order, int m, int maxbits, unsigned char *len,
                               PngBuildScratch *S) {
  if (m <= 0) return;
  if (m == 1) {
    len[order[0]] = 1;
    return;
  }
  const int K = 2 * m - 2;
  const int levels = maxbits < m - 1 ? maxbits : m - 1;      // (no code of m symbols is longer than m - 1 bits)
  for (int i = 0; i < m; ++i) S->leaf[i] = S->w[0][i] = freq[order[i]];
  for (int k = 0; k < PNG_PM_WORDS; ++k) S->is_pkg[0][k] = 0u;
  S->cnt[0] = (uint16_t)m;
  for (int lv = 1; lv < levels; ++lv) {
    const uint32_t *P = S->w[(lv - 1) & 1];
    uint32_t *C = S->w[lv & 1], *F = S->is_pkg[lv];
    for (int k = 0; k < PNG_PM_WORDS; ++k) F[k] = 0u;
    const int npk = (int)S->cnt[lv - 1] / 2;
    int i = 0, k = 0, t = 0;
    while (t < K && (i < m || k < npk)) {
      const uint32_t pw = k < npk ? png_add_sat(P[2 * k], P[2 * k + 1]) : 0u;
      if (i < m && (k >= npk || S->leaf[i] <= pw)) {
        C[t] = S->leaf[i];
        ++i;
      } else {
        C[t] = pw;
        F[t >> 5] |= 1u << (t & 31);
        ++k;
      }
      ++t;
    }
    S->cnt[lv] = (uint16_t)t;
  }
  int need = K;
  for (int lv = levels - 1; lv >= 0 && need > 0; --lv) {
    if (need > (int)S->cnt[lv]) need = (int)S->cnt[lv];       // (never with m <= 2^maxbits)
    const uint32_t *F = S->is_pkg[lv];
    int pk = 0;
    for (int k = 0; 32 * k < need; ++k) {
      const int nb = need - 32 * k;
      pk += __builtin_popcount(nb >= 32 ? F[k] : F[k] & ((1u << nb) - 1u));
    }
    const int leaves = need - pk;
    for (int i = 0; i < leaves; ++i) ++len[order[i]];
    need = 2 * pk;
  }
}

// lengths = f(freq[n], n, maxbits): 0 for a symbol that does not occur, 1 for the only symbol that does
PNG_HD void png_code_lengths(const uint32_t *freq, int n, int maxbits, unsigned char *len, PngBuildScratch *S) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    len[i] = 0;
    if (freq[i]) {
      S->order[png_rank(freq, n, i)] = (uint16_t)i;
      ++m;
    }
  }
  png_lengths_sorted(freq, S->order, m, maxbits, len, S);
}

// RFC 1951 section 3.2.2: codes of one length are consecutive in symbol order, shorter codes precede longer ones; stored
// bit-reversed, as the stream takes them
PNG_HD void png_canonical(const unsigned char *len, int n, uint16_t *code, PngBuildScratch *S) {
  uint32_t *next = S->next;
  for (int b = 0; b <= PNG_MAXBITS + 1; ++b) next[b] = 0u;
  for (int i = 0; i < n; ++i)
    if (len[i]) ++next[len[i] + 1];                           // next[b + 1] = how many codes of b bits
  uint32_t c = 0;
  for (int b = 1; b <= PNG_MAXBITS; ++b) {
    c = (c + next[b]) << 1;                                   // (next[b] still is the count of b - 1 bits)
    next[b] = c;
  }
  for (int i = 0; i < n; ++i) code[i] = len[i] ? (uint16_t)png_rev(next[len[i]]++, len[i]) : (uint16_t)0;
}

// The code lengths a dynamic block's header carries: the literal/length lengths up to the last used symbol (257 at the least)
// and then the one distance length, run-length coded as one sequence: 16 repeats the length before 3..6 times (2 extra bits),
// 17 is 3..10 zeros (3 bits), 18 is 11..138 zeros (7 bits).  The sink gets put(symbol, extra, number of extra bits).
PNG_HD int png_hlit_count(const unsigned char *len) {
  int n = PNG_NSYM;
  while (n > PNG_EOB + 1 && !len[n - 1]) --n;
  return n;
}
template <class Sink>
PNG_HD void png_header_lengths(const unsigned char *len, int nlit, Sink &sink) {
  const int N = nlit + 1;
  int i = 0;
  while (i < N) {
    const unsigned v = i < nlit ? len[i] : 1u;
    int run = 1;
    while (i + run < N && (i + run < nlit ? len[i + run] : 1u) == v) ++run;
    i += run;
    if (v == 0u) {
      while (run >= 11) {
        const int t = run < 138 ? run : 138;
        sink.put(18u, (uint32_t)(t - 11), 7);
        run -= t;
      }
      if (run >= 3) {
        sink.put(17u, (uint32_t)(run - 3), 3);
        run = 0;
      }
    } else {
      sink.put(v, 0u, 0);
      --run;
      while (run >= 3) {
        const int t = run < 6 ? run : 6;
        sink.put(16u, (uint32_t)(t - 3), 2);
        run -= t;
      }
    }
    for (; run > 0; --run) sink.put(v, 0u, 0);
  }
}
struct PngClHistSink {
  uint32_t *freq;
  PNG_HD void put(uint32_t sym, uint32_t, int) { ++freq[sym]; }
};
struct PngClCodeSink {
  const uint16_t *code;
  const unsigned char *len;
  PngBitSink out;
  uint32_t bits;
  PNG_HD void put(uint32_t sym, uint32_t extra, int nextra) {
    const int n = (int)len[sym];
    const PngTok t = {(uint32_t)code[sym] | (extra << n), n + nextra};
    out.put(t);
    bits += (uint32_t)t.n;
  }
};

// The header of a dynamic block (BFINAL 0) for the literal/length lengths `len`, written from bit 0 of the ZEROED words
// hdr[PNG_HDR_WORDS] by one lane; returns its bits.
PNG_HD uint32_t png_dynamic_header(const unsigned char *len, uint32_t *hdr, PngBuildScratch *S) {
  const int nlit = png_hlit_count(len);
  for (int k = 0; k < PNG_NCL; ++k) S->clfreq[k] = 0u;
  PngClHistSink hist = {S->clfreq};
  png_header_lengths(len, nlit, hist);
  png_code_lengths(S->clfreq, PNG_NCL, PNG_CL_MAXBITS, S->cllen, S);
  png_canonical(S->cllen, PNG_NCL, S->clcode, S);
  // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 (a literal: constant data on the host and on the device)
  const char *perm = "\020\021\022\000\010\007\011\006\012\005\013\004\014\003\015\002\016\001\017";
  int ncl = PNG_NCL;
  while (ncl > 4 && !S->cllen[(int)perm[ncl - 1]]) --ncl;
  PngClCodeSink w;
  w.code = S->clcode;
  w.len = S->cllen;
  w.bits = 0u;
  w.out.open(hdr, 0u);
  const PngTok head = {4u | ((uint32_t)(nlit - 257) << 3) | (0u << 8) | ((uint32_t)(ncl - 4) << 13), 17};  // BTYPE 10, HLIT, HDIST, HCLEN
  w.out.put(head);
  for (int k = 0; k < ncl; ++k) {
    const PngTok t = {S->cllen[(int)perm[k]], 3};
    w.out.put(t);
  }
  png_header_lengths(len, nlit, w);
  w.out.close();
  return 17u + 3u * (uint32_t)ncl + w.bits;
}

// ---- scanline filters (PNG specification section 9) for `bpp` bytes per pixel.  `cur` and `up` are the unfiltered scanline and
// the one above it (NULL above row 0: zeros); x counts the row's bytes.
PNG_HD int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}
PNG_HD int png_predict(int type, int a, int b, int c) {
  return type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
}
struct PngFilterSums {
  uint32_t s[5];
};
// adds sum |signed residual| over the bytes x0, x0 + step, .. < nbytes of a row for each of the five types
PNG_HD void png_filter_sums(const unsigned char *cur, const unsigned char *up, int x0, int step, int nbytes, int bpp,
                            PngFilterSums *sums) {
  for (int x = x0; x < nbytes; x += step) {
    const int v = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int type = 0; type < 5; ++type) {
      const int r = (v - png_predict(type, a, b, c)) & 255;
      sums->s[type] += (uint32_t)(r < 128 ? r : 256 - r);
    }
  }
}
// the type of the smallest sum; ties go to the lower type
PNG_HD int png_filter_choice(const PngFilterSums &sums) {
  int best = 0;
  uint32_t least = sums.s[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int type = 1; type < 5; ++type)
    if (sums.s[type] < least) {
      least = sums.s[type];
      best = type;
    }
  return best;
}
// dst[1 + x] = the residual of byte x under `type`, for x0, x0 + step, ..; dst[0] (the type byte) is the caller's
PNG_HD void png_filter_row(int type, const unsigned char *cur, const unsigned char *up, int x0, int step, int nbytes, int bpp,
                           unsigned char *dst) {
  for (int x = x0; x < nbytes; x += step) {
    const int v = cur[x], a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
    dst[1 + x] = (unsigned char)(v - png_predict(type, a, b, c));
  }
}
