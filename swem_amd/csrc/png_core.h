// The per-lane pieces of the PNG encoder (png.hip), written so that a host compiler takes them too: the token codes of
// RFC 1951 section 3.2.6, the bit writer, CRC-32 with its x^(8n) combine, the Adler-32 piece sums.  Nothing here knows about
// wavefronts; png.hip joins the lanes.
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

// a match of `len` (3..258) bytes at distance 1: the length symbol (257..279 are 7-bit codes 1.., 280..285 the 8-bit codes
// 0xC0..), its extra bits (least significant first), and distance code 0 = five zero bits
PNG_HD PngTok png_match(int len) {
  uint32_t sym, e = 0, extra = 0;
  if (len == PNG_MAX_MATCH) {
    sym = 285;
  } else {
    const uint32_t l = (uint32_t)(len - PNG_MIN_MATCH);      // 0..254
    if (l < 8u) {
      sym = 257u + l;
    } else {
      e = (uint32_t)(31 - __builtin_clz(l)) - 2u;            // 1..5 extra bits; four symbols per count
      sym = 261u + 4u * e + ((l >> e) & 3u);
      extra = l & ((1u << e) - 1u);
    }
  }
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
template <class Sink>
PNG_HD void png_tokens(const unsigned char *b, int p0, int p1, Sink &sink) {
  int i = p0;
  while (i < p1) {
    const unsigned c = b[i];
    if (i > 0 && c == b[i - 1]) {
      const int lim = p1 - i < PNG_MAX_MATCH ? p1 - i : PNG_MAX_MATCH;
      int r = 1;
      while (r < lim && b[i + r] == c) ++r;
      if (r >= PNG_MIN_MATCH) {
        sink.put(png_match(r));
        i += r;
        continue;
      }
    }
    sink.put(png_literal(c));
    ++i;
  }
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
