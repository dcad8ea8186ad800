// The PNG decoder (png_decode.hip) without its wavefront: the bit reader, the code-table builder and symbol
// decode of RFC 1951, the chunk walk of the PNG specification section 5, the zlib wrapper of RFC 1950, the unfilter recurrences
// of section 9 and the sub-byte unpack, as functions a host compiler takes too (tests/png_decode_host.cpp).  CRC-32, Adler-32
// and their combines are png_core.h's.
//
// One file is decoded by 64 lanes.  Whatever decides the control flow -- the bit reader's state, the status, every position -- is
// the same in all lanes: each lane computes it redundantly from the same memory.  Work that is divided is a loop
//   PNGD_EACH(wv, lane) { ... }
// over the lanes an executor stands for, stores of lane-independent values are guarded by wv.first(), and wv.sync() stands
// between a store and another lane's load of the same byte.  `wv` is the includer's: the kernel's runs one lane per thread and
// joins them with a fence and a barrier; the host program's runs the 64 lanes as a loop and joins nothing.  Lane sums meet in
// PngdLds::red, which every lane then reads.
//
// Bounded by construction: a read of the file is checked against its length `n`, a read of the compacted stream against
// `comp_len` <= n, a write of inflated bytes against `expect` <= raw_cap, and every loop consumes at least one bit of the stream,
// 12 bytes of the file or one byte of the output per trip, or leaves with a status.
#pragma once
#include "png_core.h"

#define PNGD_RING 65536u      /* the last 64 KiB of inflated bytes: the 32 KiB a match may reach into and what is not yet flushed */
#define PNGD_FLUSH 32768u     /* the ring goes to the workspace whenever this much is waiting */
#define PNGD_STEP 16384u      /* a stored block is copied in steps of at most this */
#define PNGD_INBUF 4096u      /* bytes of the compacted stream held for the bit reader */
#define PNGD_TILE 6144u       /* bytes of a scanline unfiltered serially at a time: a multiple of 64 and of 3 */
#define PNGD_FAST 10          /* codes up to this many bits are decoded by one table look-up */

// the per-file status words: include/swem_hip_io.h (SWEM_PNG_ST_*) holds the same names with the same values
enum {
  PNGD_OK = 0,
  PNGD_OFFSETS = 1,
  PNGD_SIGNATURE = 2,
  PNGD_CHUNK = 3,
  PNGD_CRC = 4,
  PNGD_IHDR = 5,
  PNGD_DIMENSIONS = 6,
  PNGD_UNSUPPORTED = 7,
  PNGD_METHOD = 8,
  PNGD_PLTE = 9,
  PNGD_IDAT = 10,
  PNGD_CRITICAL = 11,
  PNGD_IEND = 12,
  PNGD_TRAILING = 13,
  PNGD_TOO_LARGE = 14,
  PNGD_ZLIB_CM = 15,
  PNGD_ZLIB_CINFO = 16,
  PNGD_ZLIB_FCHECK = 17,
  PNGD_ZLIB_FDICT = 18,
  PNGD_BLOCK_TYPE = 19,
  PNGD_STORED_LEN = 20,
  PNGD_HLIT_HDIST = 21,
  PNGD_REPEAT = 22,
  PNGD_OVERSUBSCRIBED = 23,
  PNGD_INCOMPLETE = 24,
  PNGD_NO_EOB = 25,
  PNGD_BAD_SYMBOL = 26,
  PNGD_DISTANCE = 27,
  PNGD_NO_FINAL = 28,
  PNGD_TRUNCATED = 29,
  PNGD_IDAT_LEFT = 30,
  PNGD_LENGTH = 31,
  PNGD_ADLER = 32,
  PNGD_FILTER = 33,
  PNGD_INDEX = 34
};

#define PNGD_EACH(wv, lane) for (int lane = (wv).lane_begin(); lane < (wv).lane_end(); ++lane)

// one alphabet's decoder: the canonical form (codes per length, the symbols in code order) and a look-up of the first
// PNGD_FAST bits: (symbol << 4) | length, 0 where the code is longer or none
struct PngdTable {
  uint32_t next[16];
  uint16_t count[16];
  uint16_t offs[16];
  uint16_t sym[288];
  uint16_t fast[1 << PNGD_FAST];
};

// what a file's 64 lanes share (LDS on the device)
struct PngdLds {
  unsigned char ring[PNGD_RING];           // inflate: the output ring; unfilter: two tiles of PNGD_TILE bytes
  unsigned char inbuf[PNGD_INBUF];
  uint32_t crc_tab[256];
  unsigned long long red[3][64];           // the lanes' partial results
  PngdTable ll, dd;                        // literal/length; distance, and before it the code-length code
  unsigned char lens[320];
  unsigned char pal[768];
};

// the file under work: lane-independent values, held by every lane
struct PngdFile {
  const unsigned char *f;                  // the file
  uint32_t n;
  unsigned char *comp;                     // the IDAT payloads back to back (workspace, n bytes)
  uint32_t comp_len;
  unsigned char *raw;                      // the inflated scanlines, unfiltered in place (workspace, raw_cap bytes)
  uint32_t raw_cap;
  uint32_t w, h, rb;                       // rb: bytes of a scanline without its filter byte
  int depth, colour, n_pal;
  uint32_t expect;                         // h * (rb + 1)
};

PNG_HD uint32_t pngd_be32(const unsigned char *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
PNG_HD void pngd_lane_range(int lane, uint32_t n, uint32_t *a0, uint32_t *a1) {
  const uint32_t piece = (n + 63u) / 64u;
  const uint64_t lo = (uint64_t)lane * piece;
  *a0 = lo < n ? (uint32_t)lo : n;
  *a1 = n - *a0 > piece ? *a0 + piece : n;
}

// ---- chunk walk
// CRC-32 of p[0..m) (a chunk's type and payload) by all lanes, joined as png.hip joins it
template <class Wave>
PNG_HD uint32_t pngd_crc(const Wave &wv, PngdLds *S, const unsigned char *p, uint32_t m) {
  PNGD_EACH(wv, lane) {
    uint32_t a0, a1;
    pngd_lane_range(lane, m, &a0, &a1);
    uint32_t st = lane == 0 ? 0xffffffffu : 0u;
    st = png_crc_run(S->crc_tab, st, p + a0, a1 - a0);
    S->red[0][lane] = png_crc_shift(st, m - a1);
  }
  wv.sync();
  uint32_t x = 0;
  for (int l = 0; l < 64; ++l) x ^= (uint32_t)S->red[0][l];
  wv.sync();
  return ~x;
}

PNG_HD bool pngd_is(const unsigned char *t, char a, char b, char c, char d) {
  return t[0] == (unsigned char)a && t[1] == (unsigned char)b && t[2] == (unsigned char)c && t[3] == (unsigned char)d;
}

// IHDR's 13 bytes against what the decoder reads and what the caller's slot takes
PNG_HD int pngd_ihdr(const unsigned char *b, int Hs, int Ws, int channels, PngdFile *F) {
  const uint32_t w = pngd_be32(b), h = pngd_be32(b + 4);
  const int depth = b[8], colour = b[9];
  if (w < 1u || h < 1u || w > 0x7fffffffu || h > 0x7fffffffu) return PNGD_DIMENSIONS;
  const bool sub = depth == 1 || depth == 2 || depth == 4;
  if (b[12] != 0 || !(((colour == 0 || colour == 3) && (sub || depth == 8)) || (colour == 2 && depth == 8))) return PNGD_UNSUPPORTED;
  if (b[10] != 0 || b[11] != 0) return PNGD_METHOD;
  if ((colour == 2) != (channels == 3)) return PNGD_UNSUPPORTED;
  if (w > (uint32_t)Ws || h > (uint32_t)Hs) return PNGD_TOO_LARGE;
  F->w = w;
  F->h = h;
  F->depth = depth;
  F->colour = colour;
  F->rb = colour == 2 ? 3u * w : (w * (uint32_t)depth + 7u) / 8u;      // <= channels * Ws
  F->expect = h * (F->rb + 1u);                                          // <= Hs * (channels * Ws + 1) <= raw_cap
  return F->expect <= F->raw_cap ? PNGD_OK : PNGD_TOO_LARGE;
}

// The whole file, chunk by chunk: lengths, CRCs and order as tests/png_ref.py has them; the IDAT payloads go to F->comp, the
// palette to S->pal.  A chunk takes at least 12 bytes, so the loop runs at most n / 12 times.
template <class Wave>
PNG_HD int pngd_walk(const Wave &wv, PngdLds *S, PngdFile *F, int Hs, int Ws, int channels) {
  const unsigned char *f = F->f;
  const uint32_t n = F->n;
  const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  if (n < 8u) return PNGD_SIGNATURE;
  for (int k = 0; k < 8; ++k)
    if (f[k] != sig[k]) return PNGD_SIGNATURE;
  uint32_t pos = 8;
  int idat = 0;                                   // 0: none yet, 1: the run is open, 2: it is closed
  bool first = true, plte = false;
  F->comp_len = 0;
  F->n_pal = 0;
  for (;;) {
    if (pos == n) return PNGD_IEND;
    if (n - pos < 12u) return PNGD_CHUNK;
    const uint32_t len = pngd_be32(f + pos);
    if (len > n - pos - 12u) return PNGD_CHUNK;
    const unsigned char *type = f + pos + 4, *body = f + pos + 8;
    if (pngd_crc(wv, S, type, len + 4u) != pngd_be32(body + len)) return PNGD_CRC;
    const bool is_idat = pngd_is(type, 'I', 'D', 'A', 'T');
    if (first) {
      if (!pngd_is(type, 'I', 'H', 'D', 'R') || len != 13u) return PNGD_IHDR;
      const int st = pngd_ihdr(body, Hs, Ws, channels, F);
      if (st) return st;
    } else if (pngd_is(type, 'I', 'H', 'D', 'R')) {
      return PNGD_IHDR;
    } else if (pngd_is(type, 'P', 'L', 'T', 'E')) {
      if (F->colour != 3 || plte || idat || len % 3u || len < 3u || len > 768u) return PNGD_PLTE;
      plte = true;
      F->n_pal = (int)(len / 3u);
      PNGD_EACH(wv, lane)
        for (uint32_t i = (uint32_t)lane; i < 768u; i += 64u) S->pal[i] = i < len ? body[i] : (unsigned char)0;
    } else if (is_idat) {
      if (idat == 2) return PNGD_IDAT;
      idat = 1;
      if (len > F->n - F->comp_len) return PNGD_CHUNK;            // (never: the payloads are disjoint parts of the file)
      unsigned char *dst = F->comp + F->comp_len;
      PNGD_EACH(wv, lane)
        for (uint32_t i = (uint32_t)lane; i < len; i += 64u) dst[i] = body[i];
      F->comp_len += len;
    } else if (pngd_is(type, 'I', 'E', 'N', 'D')) {
      if (len) return PNGD_IEND;
      pos += 12u;
      break;
    } else if (!(type[0] & 0x20u)) {
      return PNGD_CRITICAL;
    }
    if (!is_idat && idat == 1) idat = 2;
    first = false;
    pos += 12u + len;
  }
  if (pos != n) return PNGD_TRAILING;
  if (!idat) return PNGD_IDAT;
  if (F->colour == 3 && !plte) return PNGD_PLTE;
  wv.sync();                                      // the compacted stream and the palette are in place
  return PNGD_OK;
}

// ---- bit reader over the compacted stream, least significant bit first.  Bits past the end read as zeros and are never
// counted: `nbits` only ever holds bits that exist.
struct PngdBits {
  const unsigned char *in;
  uint32_t end, pos, base;                        // S->inbuf holds in[base, base + PNGD_INBUF)
  uint64_t acc;
  int nbits;
};
template <class Wave>
PNG_HD void pngd_load_inbuf(const Wave &wv, PngdLds *S, PngdBits *B, uint32_t at) {
  wv.sync();
  PNGD_EACH(wv, lane)
    for (uint32_t i = (uint32_t)lane; i < PNGD_INBUF; i += 64u) S->inbuf[i] = i < B->end - at ? B->in[at + i] : (unsigned char)0;
  wv.sync();
  B->base = at;
}
template <class Wave>
PNG_HD void pngd_refill(const Wave &wv, PngdLds *S, PngdBits *B) {
  while (B->nbits <= 56 && B->pos < B->end) {
    if (B->pos - B->base >= PNGD_INBUF) pngd_load_inbuf(wv, S, B, B->pos);      // (unsigned: also after stepping back)
    B->acc |= (uint64_t)S->inbuf[B->pos - B->base] << B->nbits;
    ++B->pos;
    B->nbits += 8;
  }
}
template <class Wave>
PNG_HD bool pngd_need(const Wave &wv, PngdLds *S, PngdBits *B, int k) {
  if (B->nbits < k) pngd_refill(wv, S, B);
  return B->nbits >= k;
}
PNG_HD uint32_t pngd_take(PngdBits *B, int k) {     // k <= 16 bits that pngd_need found
  const uint32_t v = (uint32_t)B->acc & ((1u << k) - 1u);
  B->acc >>= k;
  B->nbits -= k;
  return v;
}
// drops the bits up to the next byte boundary and hands the whole bytes still held back to the stream
PNG_HD void pngd_to_byte(PngdBits *B) {
  B->pos -= (uint32_t)(B->nbits >> 3);
  B->acc = 0;
  B->nbits = 0;
}

// ---- code tables (RFC 1951 section 3.2.2) of n <= 288 lengths <= 15; `codes`: the code-length code, which must be complete.
// zlib's rule otherwise: over-subscribed is an error, incomplete is one unless the set is empty or a single code of one bit.
template <class Wave>
PNG_HD int pngd_build(const Wave &wv, PngdTable *T, const unsigned char *lens, int n, bool codes) {
  wv.sync();                                      // the lengths are in place
  if (wv.first()) {
    for (int b = 0; b < 16; ++b) T->count[b] = 0;
    for (int i = 0; i < n; ++i) ++T->count[lens[i]];
  }
  PNGD_EACH(wv, lane)
    for (int i = lane; i < (1 << PNGD_FAST); i += 64) T->fast[i] = 0;
  wv.sync();
  int left = 1, longest = 0;
  for (int b = 1; b <= 15; ++b) {
    left = (left << 1) - (int)T->count[b];
    if (left < 0) return PNGD_OVERSUBSCRIBED;
    if (T->count[b]) longest = b;
  }
  if (left > 0 && longest != 0 && (codes || longest != 1)) return PNGD_INCOMPLETE;
  if (wv.first()) {
    uint32_t code = 0;
    T->offs[1] = 0;
    for (int b = 1; b <= 15; ++b) {
      T->next[b] = code;
      code = (code + T->count[b]) << 1;
      if (b < 15) T->offs[b + 1] = (uint16_t)(T->offs[b] + T->count[b]);
    }
    for (int i = 0; i < n; ++i) {
      const int l = lens[i];
      if (!l) continue;
      T->sym[T->offs[l]++] = (uint16_t)i;          // (the offsets end as the running totals; decode uses `count` alone)
      const uint32_t c = T->next[l]++;
      if (l <= PNGD_FAST)
        for (uint32_t k = png_rev(c, l); k < (1u << PNGD_FAST); k += 1u << l) T->fast[k] = (uint16_t)((i << 4) | l);
    }
  }
  wv.sync();
  return PNGD_OK;
}

// one symbol: >= 0, or -status.  Takes at least one bit or fails.
template <class Wave>
PNG_HD int pngd_symbol(const Wave &wv, PngdLds *S, PngdBits *B, const PngdTable *T) {
  if (B->nbits < 15) pngd_refill(wv, S, B);
  const uint32_t e = T->fast[(uint32_t)B->acc & ((1u << PNGD_FAST) - 1u)];
  if (e) {
    const int l = (int)(e & 15u);
    if (l > B->nbits) return -PNGD_TRUNCATED;
    B->acc >>= l;
    B->nbits -= l;
    return (int)(e >> 4);
  }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    if (B->nbits < l) return -PNGD_TRUNCATED;
    code |= (int)((B->acc >> (l - 1)) & 1u);
    const int cnt = (int)T->count[l];
    if (code - cnt < first) {
      B->acc >>= l;
      B->nbits -= l;
      return (int)T->sym[index + (code - first)];
    }
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  return -PNGD_BAD_SYMBOL;                        // a code no symbol has: only an incomplete set leaves one
}

// length symbol 257..285 and distance symbol 0..29: base value and number of extra bits (RFC 1951 section 3.2.5)
PNG_HD void pngd_length_base(int sym, uint32_t *base, int *extra) {
  const int s = sym - 257;
  if (s < 8) {
    *base = 3u + (uint32_t)s;
    *extra = 0;
  } else if (sym == 285) {
    *base = 258u;
    *extra = 0;
  } else {
    const int e = (s - 4) >> 2;
    *base = 3u + ((4u + (uint32_t)((s - 4) & 3)) << e);
    *extra = e;
  }
}
PNG_HD void pngd_distance_base(int sym, uint32_t *base, int *extra) {
  if (sym < 4) {
    *base = 1u + (uint32_t)sym;
    *extra = 0;
  } else {
    const int e = (sym >> 1) - 1;
    *base = 1u + ((2u + (uint32_t)(sym & 1)) << e);
    *extra = e;
  }
}

// ---- the output: a ring in S->ring, flushed to F->raw
struct PngdOut {
  uint32_t p, flushed;                            // bytes produced / bytes already in F->raw
};
template <class Wave>
PNG_HD void pngd_flush(const Wave &wv, PngdLds *S, const PngdFile *F, PngdOut *O) {
  wv.sync();
  const uint32_t m = O->p - O->flushed;           // < PNGD_RING; O->p <= F->expect <= F->raw_cap
  PNGD_EACH(wv, lane)
    for (uint32_t i = (uint32_t)lane; i < m; i += 64u) F->raw[O->flushed + i] = S->ring[(O->flushed + i) & (PNGD_RING - 1u)];
  O->flushed = O->p;
}
// a lane's part of a match of `len` bytes at distance d <= p: byte i comes from p - d + (i % d), which was there before the match
PNG_HD void pngd_match_lane(unsigned char *ring, uint32_t p, uint32_t d, uint32_t len, int lane) {
  if (d >= len) {                                 // (the same in every lane) no byte of the match is its own source: i % d == i
    for (uint32_t i = (uint32_t)lane; i < len; i += 64u) ring[(p + i) & (PNGD_RING - 1u)] = ring[(p - d + i) & (PNGD_RING - 1u)];
    return;
  }
  for (uint32_t i = (uint32_t)lane; i < len; i += 64u) ring[(p + i) & (PNGD_RING - 1u)] = ring[(p - d + i % d) & (PNGD_RING - 1u)];
}

// the code lengths of a dynamic block's header (section 3.2.7) into S->lens, and both tables
template <class Wave>
PNG_HD int pngd_dynamic_tables(const Wave &wv, PngdLds *S, PngdBits *B) {
  if (!pngd_need(wv, S, B, 14)) return PNGD_TRUNCATED;
  const int nlen = (int)pngd_take(B, 5) + 257, ndist = (int)pngd_take(B, 5) + 1, ncode = (int)pngd_take(B, 4) + 4;
  if (nlen > 286 || ndist > 30) return PNGD_HLIT_HDIST;
  const char *perm = "\020\021\022\000\010\007\011\006\012\005\013\004\014\003\015\002\016\001\017";
  wv.sync();
  if (wv.first())
    for (int k = 0; k < 19; ++k) S->lens[k] = 0;
  for (int k = 0; k < ncode; ++k) {
    if (!pngd_need(wv, S, B, 3)) return PNGD_TRUNCATED;
    const unsigned v = pngd_take(B, 3);
    if (wv.first()) S->lens[(int)perm[k]] = (unsigned char)v;
  }
  int st = pngd_build(wv, &S->dd, S->lens, 19, true);
  if (st) return st;
  int i = 0, prev = -1, eob = 0;
  while (i < nlen + ndist) {
    const int sym = pngd_symbol(wv, S, B, &S->dd);
    if (sym < 0) return -sym;
    int rep = 1, v = sym;
    if (sym == 16) {
      if (prev < 0) return PNGD_REPEAT;
      if (!pngd_need(wv, S, B, 2)) return PNGD_TRUNCATED;
      rep = 3 + (int)pngd_take(B, 2);
      v = prev;
    } else if (sym == 17) {
      if (!pngd_need(wv, S, B, 3)) return PNGD_TRUNCATED;
      rep = 3 + (int)pngd_take(B, 3);
      v = 0;
    } else if (sym == 18) {
      if (!pngd_need(wv, S, B, 7)) return PNGD_TRUNCATED;
      rep = 11 + (int)pngd_take(B, 7);
      v = 0;
    }
    if (rep > nlen + ndist - i) return PNGD_REPEAT;
    if (i <= PNG_EOB && PNG_EOB < i + rep) eob = v;
    if (wv.first())
      for (int k = 0; k < rep; ++k) S->lens[i + k] = (unsigned char)v;
    i += rep;
    prev = v;
  }
  if (!eob) return PNGD_NO_EOB;
  st = pngd_build(wv, &S->dd, S->lens + nlen, ndist, false);     // (the code-length code is done with)
  if (st) return st;
  return pngd_build(wv, &S->ll, S->lens, nlen, false);
}

template <class Wave>
PNG_HD int pngd_fixed_tables(const Wave &wv, PngdLds *S) {
  wv.sync();
  PNGD_EACH(wv, lane)
    for (int i = lane; i < 320; i += 64) S->lens[i] = (unsigned char)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
  int st = pngd_build(wv, &S->ll, S->lens, 288, false);
  if (st) return st;
  return pngd_build(wv, &S->dd, S->lens + 288, 32, false);       // (30 and 31 have codes and no meaning)
}

// the zlib stream F->comp[0, comp_len) -> F->raw[0, expect); the Adler-32 the stream carries goes to *adler
template <class Wave>
PNG_HD int pngd_inflate(const Wave &wv, PngdLds *S, const PngdFile *F, uint32_t *adler) {
  if (F->comp_len < 2u) return PNGD_TRUNCATED;
  const unsigned cmf = F->comp[0], flg = F->comp[1];
  if ((cmf & 15u) != 8u) return PNGD_ZLIB_CM;
  if ((cmf >> 4) > 7u) return PNGD_ZLIB_CINFO;
  if ((cmf * 256u + flg) % 31u) return PNGD_ZLIB_FCHECK;
  if (flg & 0x20u) return PNGD_ZLIB_FDICT;
  PngdBits B = {F->comp, F->comp_len, 2u, 0u, 0u, 0};
  pngd_load_inbuf(wv, S, &B, 2u);
  PngdOut O = {0u, 0u};
  bool fixed_built = false;
  for (;;) {                                      // a block takes at least 3 bits
    if (!pngd_need(wv, S, &B, 3)) return PNGD_NO_FINAL;
    const uint32_t last = pngd_take(&B, 1), btype = pngd_take(&B, 2);
    if (btype == 3u) return PNGD_BLOCK_TYPE;
    if (btype == 0u) {
      pngd_to_byte(&B);
      if (B.end - B.pos < 4u) return PNGD_TRUNCATED;
      const unsigned char *q = B.in + B.pos;
      const uint32_t len = q[0] | ((uint32_t)q[1] << 8), nlen = q[2] | ((uint32_t)q[3] << 8);
      if (len != (nlen ^ 0xffffu)) return PNGD_STORED_LEN;
      B.pos += 4u;
      if (len > B.end - B.pos) return PNGD_TRUNCATED;
      if (len > F->expect - O.p) return PNGD_LENGTH;
      for (uint32_t done = 0; done < len;) {
        const uint32_t m = len - done < PNGD_STEP ? len - done : PNGD_STEP;
        const unsigned char *src = B.in + B.pos + done;
        PNGD_EACH(wv, lane)
          for (uint32_t i = (uint32_t)lane; i < m; i += 64u) S->ring[(O.p + i) & (PNGD_RING - 1u)] = src[i];
        O.p += m;
        done += m;
        if (O.p - O.flushed >= PNGD_FLUSH) pngd_flush(wv, S, F, &O);
      }
      B.pos += len;
    } else {
      if (btype == 1u) {
        if (!fixed_built) {
          const int st = pngd_fixed_tables(wv, S);
          if (st) return st;
        }
        fixed_built = true;
      } else {
        fixed_built = false;
        const int st = pngd_dynamic_tables(wv, S, &B);
        if (st) return st;
      }
      for (;;) {                                  // a symbol takes at least one bit
        const int sym = pngd_symbol(wv, S, &B, &S->ll);
        if (sym < 0) return -sym;
        if (sym < 256) {
          if (O.p >= F->expect) return PNGD_LENGTH;
          if (wv.first()) S->ring[O.p & (PNGD_RING - 1u)] = (unsigned char)sym;
          ++O.p;
        } else if (sym == PNG_EOB) {
          break;
        } else {
          if (sym > 285) return PNGD_BAD_SYMBOL;
          uint32_t len, dist;
          int extra;
          pngd_length_base(sym, &len, &extra);
          if (!pngd_need(wv, S, &B, extra)) return PNGD_TRUNCATED;
          len += pngd_take(&B, extra);
          const int ds = pngd_symbol(wv, S, &B, &S->dd);
          if (ds < 0) return -ds;
          if (ds > 29) return PNGD_BAD_SYMBOL;
          pngd_distance_base(ds, &dist, &extra);
          if (!pngd_need(wv, S, &B, extra)) return PNGD_TRUNCATED;
          dist += pngd_take(&B, extra);
          if (dist > O.p) return PNGD_DISTANCE;
          if (len > F->expect - O.p) return PNGD_LENGTH;
          wv.sync();                              // the bytes before the match are in the ring
          PNGD_EACH(wv, lane) pngd_match_lane(S->ring, O.p, dist, len, lane);
          O.p += len;
        }
        if (O.p - O.flushed >= PNGD_FLUSH) pngd_flush(wv, S, F, &O);
      }
    }
    if (last) break;
  }
  pngd_flush(wv, S, F, &O);
  wv.sync();                                      // F->raw is whole
  pngd_to_byte(&B);
  if (B.end - B.pos < 4u) return PNGD_TRUNCATED;
  *adler = pngd_be32(B.in + B.pos);
  if (B.end - B.pos > 4u) return PNGD_IDAT_LEFT;
  return O.p == F->expect ? PNGD_OK : PNGD_LENGTH;
}

// Adler-32 of F->raw[0, expect), expect < 2^31: the lanes' piece sums joined as png.hip joins the segments'
template <class Wave>
PNG_HD uint32_t pngd_adler(const Wave &wv, PngdLds *S, const PngdFile *F) {
  const uint32_t N = F->expect;
  PNGD_EACH(wv, lane) {
    uint32_t a0, a1;
    pngd_lane_range(lane, N, &a0, &a1);
    unsigned long long a, w;
    png_adler_piece(F->raw + a0, (int)(a1 - a0), &a, &w);       // a piece is < 2^25 bytes: w < 2^8 * 2^50
    a %= PNG_ADLER_MOD;
    S->red[0][lane] = a;
    S->red[1][lane] = (w % PNG_ADLER_MOD + a * ((N - a1) % PNG_ADLER_MOD)) % PNG_ADLER_MOD;
  }
  wv.sync();
  unsigned long long A = 1, Bs = N % PNG_ADLER_MOD;              // (A starts at 1: every byte adds it to B once)
  for (int l = 0; l < 64; ++l) {
    A += S->red[0][l];
    Bs += S->red[1][l];
  }
  wv.sync();
  return (uint32_t)(((Bs % PNG_ADLER_MOD) << 16) | (A % PNG_ADLER_MOD));
}

// ---- unfilter (PNG specification section 9.2).  Types 3 and 4 are recurrences along the row: one lane runs them over a tile
// in LDS.  a[], c[]: the bpp bytes left of the tile in this row and in the row above.
PNG_HD void pngd_unfilter_serial(int type, unsigned char *cur, const unsigned char *up, uint32_t m, int bpp, unsigned char *a,
                                 unsigned char *c) {
  for (uint32_t x = 0; x < m; ++x) {
    const int k = (int)(x % (uint32_t)bpp);
    const int b = up[x];
    const int v = (cur[x] + (type == 3 ? (a[k] + b) >> 1 : png_paeth(a[k], b, c[k]))) & 255;
    cur[x] = (unsigned char)v;
    a[k] = (unsigned char)v;
    c[k] = (unsigned char)b;
  }
}
// type 1 is a prefix sum mod 256 per channel: a lane sums its pixels [px0, px1), then adds what stands left of them
PNG_HD void pngd_sub_sums(const unsigned char *cur, uint32_t px0, uint32_t px1, int bpp, uint32_t nbytes, unsigned *sum) {
  for (int k = 0; k < 3; ++k) sum[k] = 0;
  for (uint32_t x = px0 * (uint32_t)bpp; x < px1 * (uint32_t)bpp && x < nbytes; ++x) sum[x % (uint32_t)bpp] += cur[x];
}
PNG_HD void pngd_sub_apply(unsigned char *cur, uint32_t px0, uint32_t px1, int bpp, uint32_t nbytes, unsigned *carry) {
  for (uint32_t x = px0 * (uint32_t)bpp; x < px1 * (uint32_t)bpp && x < nbytes; ++x) {
    const uint32_t k = x % (uint32_t)bpp;
    carry[k] = (carry[k] + cur[x]) & 255u;
    cur[x] = (unsigned char)carry[k];
  }
}

// all rows of F->raw in place; PNGD_FILTER for a type byte past 4
template <class Wave>
PNG_HD int pngd_unfilter(const Wave &wv, PngdLds *S, const PngdFile *F) {
  const uint32_t rb = F->rb, rw = rb + 1u;
  const int bpp = F->colour == 2 ? 3 : 1;
  unsigned char *tile_c = S->ring, *tile_u = S->ring + PNGD_TILE;
  for (uint32_t y = 0; y < F->h; ++y) {
    unsigned char *cur = F->raw + (size_t)y * rw + 1;
    const unsigned char *up = y ? cur - rw : nullptr;
    const int type = cur[-1];
    if (type > 4) return PNGD_FILTER;
    if (type == 2) {
      if (up) PNGD_EACH(wv, lane)
        for (uint32_t x = (uint32_t)lane; x < rb; x += 64u) cur[x] = (unsigned char)(cur[x] + up[x]);
    } else if (type == 1) {
      const uint32_t npx = (rb + (uint32_t)bpp - 1u) / (uint32_t)bpp;
      PNGD_EACH(wv, lane) {
        uint32_t p0, p1;
        unsigned sum[3];
        pngd_lane_range(lane, npx, &p0, &p1);
        pngd_sub_sums(cur, p0, p1, bpp, rb, sum);
        for (int k = 0; k < 3; ++k) S->red[k][lane] = sum[k];
      }
      wv.sync();
      PNGD_EACH(wv, lane) {
        uint32_t p0, p1;
        unsigned carry[3] = {0u, 0u, 0u};
        pngd_lane_range(lane, npx, &p0, &p1);
        for (int l = 0; l < lane; ++l)
          for (int k = 0; k < 3; ++k) carry[k] += (unsigned)S->red[k][l];
        for (int k = 0; k < 3; ++k) carry[k] &= 255u;
        pngd_sub_apply(cur, p0, p1, bpp, rb, carry);
      }
    } else if (type == 3 || type == 4) {
      unsigned char a[3] = {0, 0, 0}, c[3] = {0, 0, 0};
      for (uint32_t t0 = 0; t0 < rb; t0 += PNGD_TILE) {
        const uint32_t m = rb - t0 < PNGD_TILE ? rb - t0 : PNGD_TILE;
        PNGD_EACH(wv, lane)
          for (uint32_t x = (uint32_t)lane; x < m; x += 64u) {
            tile_c[x] = cur[t0 + x];
            tile_u[x] = up ? up[t0 + x] : (unsigned char)0;
          }
        wv.sync();
        if (wv.first()) pngd_unfilter_serial(type, tile_c, tile_u, m, bpp, a, c);
        wv.sync();
        // every lane takes the carries from the tile: its last bpp bytes (PNGD_TILE is a multiple of 3)
        for (int k = 0; k < bpp && (uint32_t)k < m; ++k) {
          const uint32_t x = m - (uint32_t)bpp + (uint32_t)k;
          if (m >= (uint32_t)bpp) {
            a[x % (uint32_t)bpp] = tile_c[x];
            c[x % (uint32_t)bpp] = tile_u[x];
          }
        }
        PNGD_EACH(wv, lane)
          for (uint32_t x = (uint32_t)lane; x < m; x += 64u) cur[t0 + x] = tile_c[x];
        wv.sync();
      }
    }
    wv.sync();                                    // the row is whole before the next one reads it
  }
  return PNGD_OK;
}

// sample x of an unfiltered row: depths 1, 2 and 4 most significant bits first
PNG_HD unsigned pngd_sample(const unsigned char *row, uint32_t x, int depth) {
  if (depth == 8) return row[x];
  const uint32_t bit = x * (uint32_t)depth;
  return (row[bit >> 3] >> (8u - (uint32_t)depth - (bit & 7u))) & ((1u << depth) - 1u);
}

// ---- one file of a call, start to end.  `blob`, `offsets` as the encoder leaves them; o0, o1 = offsets[t], offsets[t + 1];
// comp_ws: blob_bytes bytes, file t's compacted stream at comp_ws + o0; raw: this file's raw_cap bytes.  Writes the file's slot
// of pixels ([Hs][Ws][channels], zero outside h x w or when refused), sizes2 (h, w), pal_out (768) and npal_out if given, status.
template <class Wave>
PNG_HD void pngd_decode_file(const Wave &wv, PngdLds *S, const unsigned char *blob, size_t blob_bytes, long long o0, long long o1,
                             int Hs, int Ws, int channels, unsigned char *pixels, int *sizes2, unsigned char *pal_out,
                             int *npal_out, int *status, unsigned char *comp_ws, unsigned char *raw, uint32_t raw_cap) {
  PNGD_EACH(wv, lane)
    for (int k = lane; k < 256; k += 64) S->crc_tab[k] = png_crc_entry((uint32_t)k);
  wv.sync();
  PngdFile F = {};
  int st = PNGD_OK;
  if (o0 < 0 || o1 < o0 || (unsigned long long)o1 > (unsigned long long)blob_bytes || o1 - o0 > 0x7fffffffll) {
    st = PNGD_OFFSETS;
  } else {
    F.f = blob + o0;
    F.n = (uint32_t)(o1 - o0);
    F.comp = comp_ws + o0;
    F.raw = raw;
    F.raw_cap = raw_cap;
    st = pngd_walk(wv, S, &F, Hs, Ws, channels);
    uint32_t adler = 0;
    if (!st) st = pngd_inflate(wv, S, &F, &adler);
    if (!st && pngd_adler(wv, S, &F) != adler) st = PNGD_ADLER;
    if (!st) st = pngd_unfilter(wv, S, &F);
    if (!st && F.colour == 3) {
      PNGD_EACH(wv, lane) {
        unsigned most = 0;
        for (uint32_t y = 0; y < F.h; ++y) {
          const unsigned char *row = F.raw + (size_t)y * (F.rb + 1u) + 1;
          for (uint32_t x = (uint32_t)lane; x < F.w; x += 64u) {
            const unsigned v = pngd_sample(row, x, F.depth);
            most = v > most ? v : most;
          }
        }
        S->red[0][lane] = most;
      }
      wv.sync();
      unsigned most = 0;
      for (int l = 0; l < 64; ++l) most = (unsigned)S->red[0][l] > most ? (unsigned)S->red[0][l] : most;
      wv.sync();
      if ((int)most >= F.n_pal) st = PNGD_INDEX;
    }
  }
  const uint32_t h = st ? 0u : F.h, w = st ? 0u : F.w;
  PNGD_EACH(wv, lane) {
    for (uint32_t y = 0; y < (uint32_t)Hs; ++y) {
      unsigned char *dst = pixels + (size_t)y * Ws * channels;
      const unsigned char *row = y < h ? F.raw + (size_t)y * (F.rb + 1u) + 1 : nullptr;
      if (channels == 3) {
        for (uint32_t x = (uint32_t)lane; x < 3u * (uint32_t)Ws; x += 64u) dst[x] = (row && x < 3u * w) ? row[x] : (unsigned char)0;
      } else {
        for (uint32_t x = (uint32_t)lane; x < (uint32_t)Ws; x += 64u)
          dst[x] = (row && x < w) ? (unsigned char)pngd_sample(row, x, F.depth) : (unsigned char)0;
      }
    }
    if (pal_out)
      for (int k = lane; k < 768; k += 64) pal_out[k] = (!st && F.colour == 3) ? S->pal[k] : (unsigned char)0;
  }
  if (wv.first()) {
    sizes2[0] = (int)h;
    sizes2[1] = (int)w;
    if (npal_out) *npal_out = st ? 0 : F.n_pal;
    *status = st;
  }
}
