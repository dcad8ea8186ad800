// Result PNGs on the device (include/swem_hip_io.h): T uint8 index maps in, T complete PNG files out.
//   png_encode_kernel   one wavefront per segment of whole scanlines (filter type 0), all frames in one launch: the filtered bytes
//                       go to LDS, every lane codes a contiguous piece of them (literals and matches at distance 1 with the
//                       fixed Huffman codes, csrc/png_core.h), a prefix sum over the lanes' bit counts places the pieces, and
//                       the bits are OR-ed into the segment's zeroed slot of the workspace.  A segment that would not shrink is a
//                       stored block.  Every segment ends on a byte boundary (an empty stored block after the coded one), so
//                       that segments are joined by copying bytes.  Also the segment's Adler-32 sums.
//   png_encode_px_kernel  the second form (swem_png_encode_px_u8): 1 or 3 channels -- truecolour
//                       scanlines under a filter type of their own --, and with dynamic codes a Huffman table per segment
//                       (histogram in LDS, lengths, codes and block header by lane 0), taken where it is the smallest form
//   png_offsets_kernel file sizes from the segment lengths, prefix-summed into offsets[T + 1]
//   png_pack_kernel     one wavefront per chunk: copies a segment's bytes to its place in the blob as an IDAT chunk with its
//                       CRC-32 (every lane runs the table over a piece, the registers are joined with x^(8n) mod P); the last
//                       wavefront of a frame writes the signature, IHDR, PLTE, the closing IDAT (final empty block and the
//                       Adler-32 joined from the segments' sums) and IEND.
// The palette travels in the launch by value, as the tables of stage.hip do.
#include "common.h"
#include "../../include/swem_hip_io.h"
#include "png_core.h"

namespace {

#define PNG_SEG_ROWS 16      /* scanlines per segment (fewer where 16 would pass 65535 bytes) */
#define PNG_SEG_MAX 65535    /* LEN of a stored block */
#define PNG_STORED_EXTRA 5   /* a stored block's header byte, LEN and NLEN */
#define PNG_CHUNK_EXTRA 12   /* a chunk's length, type and CRC */
#define PNG_FIXED_HEAD (8 + 25)             /* signature, IHDR */
#define PNG_PLTE_BYTES (PNG_CHUNK_EXTRA + 768)
#define PNG_TAIL_BYTES (PNG_CHUNK_EXTRA + 9 + PNG_CHUNK_EXTRA) /* closing IDAT (01 00 00 FF FF + Adler-32), IEND */

struct PngPalette {
  unsigned char rgb[768];
};

struct PngLayout {
  int rw;               // bytes of a filtered scanline
  int rows;             // scanlines per segment
  int nseg;             // segments per frame
  size_t slot;          // bytes of a segment's slot in the workspace (its stored form, rounded up to words)
};

inline PngLayout png_layout(int H, int row_bytes) {
  PngLayout L;
  L.rw = row_bytes + 1;
  L.rows = PNG_SEG_MAX / L.rw < PNG_SEG_ROWS ? PNG_SEG_MAX / L.rw : PNG_SEG_ROWS;
  L.nseg = (H + L.rows - 1) / L.rows;
  L.slot = align_up((size_t)L.rows * L.rw + PNG_STORED_EXTRA, 16);
  return L;
}

// meta[t * nseg + s] = (payload bytes, Adler a, Adler w, 0): a = sum of the segment's bytes, w = sum (n - i) * b[i], mod 65521
__global__ __launch_bounds__(64) void png_encode_kernel(const unsigned char *__restrict__ maps, unsigned char *__restrict__ slots,
                                                        uint4 *__restrict__ meta, int H, int W, int seg_rows, size_t slot_bytes) {
  extern __shared__ unsigned char seg[];
  const int lane = threadIdx.x;
  const int nseg = gridDim.x;
  const size_t t = blockIdx.y, s = blockIdx.x;
  const int row0 = (int)s * seg_rows;
  const int rows = H - row0 < seg_rows ? H - row0 : seg_rows;
  const int rw = W + 1;
  const int n = rows * rw;                           // 1 < n <= 65535
  const unsigned char *src = maps + (t * H + row0) * W;
  for (int r = 0; r < rows; ++r) {
    if (lane == 0) seg[r * rw] = 0;                  // filter type 0
    for (int x = lane; x < W; x += 64) seg[r * rw + 1 + x] = src[(size_t)r * W + x];
  }
  __syncthreads();

  const int piece = (n + 63) / 64;
  const int p0 = lane * piece < n ? lane * piece : n;
  const int p1 = p0 + piece < n ? p0 + piece : n;
  PngCountSink cnt = {0u};
  png_tokens(seg, p0, p1, cnt);
  const unsigned mine = cnt.bits + (lane == 0 ? 3u : 0u);       // the block header goes first
  unsigned incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned v = __shfl_up(incl, d);
    if (lane >= d) incl += v;
  }
  // header and tokens, the end-of-block code (7 zero bits), an empty stored block: 3 zero bits, padding, 00 00 FF FF
  const unsigned total_bits = __shfl(incl, 63) + 7u + 3u;
  const unsigned coded = (total_bits + 7u) / 8u + 4u;
  const unsigned stored = (unsigned)n + PNG_STORED_EXTRA;
  unsigned char *out = slots + (t * nseg + s) * slot_bytes;
  unsigned len;
  if (coded < stored) {
    len = coded;
    uint32_t *words = reinterpret_cast<uint32_t *>(out);
    for (unsigned w = lane; w < (coded + 3u) / 4u; w += 64) words[w] = 0u;     // (coded + 3) / 4 * 4 <= slot_bytes
    __threadfence();                                  // the zeros are in place before any lane ORs into them
    __syncthreads();
    PngBitSink bits;
    bits.open(words, incl - mine);
    if (lane == 0) {
      const PngTok fixed_block = {2u, 3};             // BFINAL 0, BTYPE 01
      bits.put(fixed_block);
    }
    png_tokens(seg, p0, p1, bits);
    bits.close();
    if (lane == 0) {
      png_or_byte(words, coded - 2u, 0xffu);
      png_or_byte(words, coded - 1u, 0xffu);
    }
  } else {
    len = stored;
    if (lane == 0) {
      out[0] = 0;                                     // BFINAL 0, BTYPE 00
      out[1] = (unsigned char)n;
      out[2] = (unsigned char)(n >> 8);
      out[3] = (unsigned char)~n;
      out[4] = (unsigned char)(~n >> 8);
    }
    for (int i = lane; i < n; i += 64) out[PNG_STORED_EXTRA + i] = seg[i];
  }

  unsigned long long a, w;
  png_adler_piece(seg + p0, p1 - p0, &a, &w);
  w += a * (unsigned long long)(n - p1);              // < 2^8 * 2^10 * 2^16
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off);
    w += __shfl_xor(w, off);
  }
  if (lane == 0) meta[t * nseg + s] = make_uint4(len, (unsigned)(a % PNG_ADLER_MOD), (unsigned)(w % PNG_ADLER_MOD), 0u);
}

// what the dynamic form keeps in LDS behind the segment
struct PngDynLds {
  uint32_t freq[288];                   // the segment's literal/length histogram
  uint32_t hdr[PNG_HDR_WORDS];          // the block header, from bit 0
  uint32_t hdr_bits;
  uint16_t code[288];
  unsigned char len[288];
  PngBuildScratch S;
};

// The second form: `channels` 1 (filter type 0, as above) or 3 (every scanline under the filter type 0-4 of the smallest sum of
// |signed residual|; the row above comes from the source picture, zeros above row 0), and with `dynamic` a Huffman table of the
// segment's own.  The lanes histogram their pieces into LDS; the used symbols are ranked by all lanes; lane 0 builds the
// lengths (package-merge, at most 15 bits), the codes and the block header; every lane then counts its piece under the fixed
// and the dynamic code at once and two prefix sums give the two coded sizes.  Dynamic only if strictly smaller than fixed; a
// coded form only if strictly smaller than stored.  Slots, meta and the closing empty stored block are those of the kernel above.
__global__ __launch_bounds__(64) void png_encode_px_kernel(const unsigned char *__restrict__ pixels, unsigned char *__restrict__ slots,
                                                           uint4 *__restrict__ meta, int H, int W, int channels, int dynamic,
                                                           int seg_rows, size_t slot_bytes) {
  extern __shared__ __align__(16) unsigned char seg[];
  const int lane = threadIdx.x;
  const int nseg = gridDim.x;
  const size_t t = blockIdx.y, s = blockIdx.x;
  const int row0 = (int)s * seg_rows;
  const int rows = H - row0 < seg_rows ? H - row0 : seg_rows;
  const int rb = channels * W, rw = rb + 1;
  const int n = rows * rw;                           // 1 < n <= 65535
  PngDynLds *D = reinterpret_cast<PngDynLds *>(seg + (((size_t)seg_rows * rw + 15) & ~(size_t)15));   // (only with `dynamic`)
  const unsigned char *src = pixels + (t * H + row0) * rb;
  for (int r = 0; r < rows; ++r) {
    const unsigned char *cur = src + (size_t)r * rb;
    int type = 0;
    if (channels == 3) {
      const unsigned char *up = row0 + r > 0 ? cur - rb : nullptr;
      PngFilterSums sums = {{0u, 0u, 0u, 0u, 0u}};
      png_filter_sums(cur, up, lane, 64, rb, 3, &sums);
#pragma unroll
      for (int k = 0; k < 5; ++k)
        for (int off = 32; off > 0; off >>= 1) sums.s[k] += __shfl_xor(sums.s[k], off);
      type = png_filter_choice(sums);
      png_filter_row(type, cur, up, lane, 64, rb, 3, seg + r * rw);
    } else {
      for (int x = lane; x < W; x += 64) seg[r * rw + 1 + x] = cur[x];
    }
    if (lane == 0) seg[r * rw] = (unsigned char)type;
  }
  if (dynamic) {
    for (int k = lane; k < 288; k += 64) {
      D->freq[k] = 0u;
      D->len[k] = 0;
    }
    for (int k = lane; k < PNG_HDR_WORDS; k += 64) D->hdr[k] = 0u;
  }
  __syncthreads();

  const int piece = (n + 63) / 64;
  const int p0 = lane * piece < n ? lane * piece : n;
  const int p1 = p0 + piece < n ? p0 + piece : n;
  unsigned mine_f, mine_d = 0u, eob_d = 0u;
  if (dynamic) {
    PngHistSink hist = {D->freq};
    png_symbols(seg, p0, p1, hist);
    if (lane == 0) png_count_one(D->freq + PNG_EOB);
    __syncthreads();
    int used = 0;
    for (int i = lane; i < PNG_NSYM; i += 64)
      if (D->freq[i]) {
        D->S.order[png_rank(D->freq, PNG_NSYM, i)] = (uint16_t)i;
        ++used;
      }
    for (int off = 32; off > 0; off >>= 1) used += __shfl_xor(used, off);
    __syncthreads();
    if (lane == 0) {
      png_lengths_sorted(D->freq, D->S.order, used, PNG_MAXBITS, D->len, &D->S);
      png_canonical(D->len, PNG_NSYM, D->code, &D->S);
      D->hdr_bits = png_dynamic_header(D->len, D->hdr, &D->S);
    }
    __syncthreads();
    PngFixedCountSink cf = {0u};
    PngLenCountSink cd = {D->len, 1u, 0u};
    PngBothSinks<PngFixedCountSink, PngLenCountSink> both = {cf, cd};
    png_symbols(seg, p0, p1, both);
    mine_f = cf.bits;
    mine_d = cd.bits + (lane == 0 ? D->hdr_bits : 0u);
    eob_d = D->len[PNG_EOB];
  } else {
    PngCountSink cnt = {0u};
    png_tokens(seg, p0, p1, cnt);
    mine_f = cnt.bits;
  }
  mine_f += lane == 0 ? 3u : 0u;                      // the block header goes first
  unsigned incl_f = mine_f, incl_d = mine_d;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned vf = __shfl_up(incl_f, d), vd = __shfl_up(incl_d, d);
    if (lane >= d) {
      incl_f += vf;
      incl_d += vd;
    }
  }
  // header and tokens, the end-of-block code, an empty stored block: 3 zero bits, padding, 00 00 FF FF
  const unsigned coded_f = (__shfl(incl_f, 63) + 7u + 3u + 7u) / 8u + 4u;
  const unsigned coded_d = (__shfl(incl_d, 63) + eob_d + 3u + 7u) / 8u + 4u;
  const bool use_d = dynamic && coded_d < coded_f;
  const unsigned coded = use_d ? coded_d : coded_f;
  const unsigned stored = (unsigned)n + PNG_STORED_EXTRA;
  unsigned char *out = slots + (t * nseg + s) * slot_bytes;
  unsigned len;
  if (coded < stored) {
    len = coded;
    uint32_t *words = reinterpret_cast<uint32_t *>(out);
    for (unsigned w = lane; w < (coded + 3u) / 4u; w += 64) words[w] = 0u;     // (coded + 3) / 4 * 4 <= slot_bytes
    __threadfence();                                  // the zeros are in place before any lane ORs into them
    __syncthreads();
    if (use_d) {
      for (unsigned w = lane; w < (D->hdr_bits + 31u) / 32u; w += 64) png_or_word(words + w, D->hdr[w]);
      PngCodeSink bits;
      bits.code = D->code;
      bits.len = D->len;
      bits.out.open(words, incl_d - mine_d + (lane == 0 ? D->hdr_bits : 0u));
      png_symbols(seg, p0, p1, bits);
      if (lane == 63) bits.literal(PNG_EOB);          // (its piece is the last, or empty at the end)
      bits.out.close();
    } else {
      PngBitSink bits;
      bits.open(words, incl_f - mine_f);
      if (lane == 0) {
        const PngTok fixed_block = {2u, 3};           // BFINAL 0, BTYPE 01
        bits.put(fixed_block);
      }
      png_tokens(seg, p0, p1, bits);
      bits.close();
    }
    if (lane == 0) {
      png_or_byte(words, coded - 2u, 0xffu);
      png_or_byte(words, coded - 1u, 0xffu);
    }
  } else {
    len = stored;
    if (lane == 0) {
      out[0] = 0;                                     // BFINAL 0, BTYPE 00
      out[1] = (unsigned char)n;
      out[2] = (unsigned char)(n >> 8);
      out[3] = (unsigned char)~n;
      out[4] = (unsigned char)(~n >> 8);
    }
    for (int i = lane; i < n; i += 64) out[PNG_STORED_EXTRA + i] = seg[i];
  }

  unsigned long long a, w;
  png_adler_piece(seg + p0, p1 - p0, &a, &w);
  w += a * (unsigned long long)(n - p1);              // < 2^8 * 2^10 * 2^16
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off);
    w += __shfl_xor(w, off);
  }
  if (lane == 0) meta[t * nseg + s] = make_uint4(len, (unsigned)(a % PNG_ADLER_MOD), (unsigned)(w % PNG_ADLER_MOD), 0u);
}

__device__ __forceinline__ long long png_frame_bytes(const uint4 *__restrict__ meta, size_t t, int nseg, int head) {
  long long sum = head + 2 + PNG_TAIL_BYTES;          // (2: the zlib header, in the first IDAT)
  for (int s = 0; s < nseg; ++s) sum += PNG_CHUNK_EXTRA + (long long)meta[t * nseg + s].x;
  return sum;
}

// one block: offsets[0] = 0, offsets[t + 1] = offsets[t] + bytes of file t
__global__ __launch_bounds__(256) void png_offsets_kernel(const uint4 *__restrict__ meta, long long *__restrict__ offsets, int T,
                                                          int nseg, int head) {
  __shared__ long long sh[256];
  __shared__ long long carry;
  const int tid = threadIdx.x;
  if (tid == 0) {
    carry = 0;
    offsets[0] = 0;
  }
  __syncthreads();
  for (int base = 0; base < T; base += 256) {
    const int t = base + tid;
    sh[tid] = t < T ? png_frame_bytes(meta, (size_t)t, nseg, head) : 0;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const long long v = tid >= d ? sh[tid - d] : 0;
      __syncthreads();
      sh[tid] += v;
      __syncthreads();
    }
    if (t < T) offsets[t + 1] = carry + sh[tid];
    __syncthreads();
    if (tid == 0) carry += sh[255];
    __syncthreads();
  }
}

// CRC-32 of `pre` (npre <= 8 bytes: the chunk type and, in a frame's first IDAT, the zlib header) followed by data[0..n), by
// the whole wavefront; every lane returns it.
__device__ __forceinline__ uint32_t png_wave_crc(const uint32_t *tab, const unsigned char *pre, int npre,
                                                 const unsigned char *data, unsigned n, int lane) {
  const unsigned piece = (n + 63u) / 64u;
  const unsigned a0 = lane * piece < n ? lane * piece : n;
  const unsigned a1 = a0 + piece < n ? a0 + piece : n;
  uint32_t state = 0;
  if (lane == 0) state = png_crc_run(tab, 0xffffffffu, pre, (size_t)npre);
  state = png_crc_run(tab, state, data + a0, a1 - a0);
  state = png_crc_shift(state, n - a1);
  for (int off = 32; off > 0; off >>= 1) state ^= (uint32_t)__shfl_xor((int)state, off);
  return ~state;
}

// a chunk at dst: length, type (+ `extra` bytes of payload before the data), data, CRC; by the whole wavefront
__device__ __forceinline__ void png_wave_chunk(const uint32_t *tab, unsigned char *dst, const char *type, const unsigned char *extra,
                                               int nextra, const unsigned char *data, unsigned n, int lane) {
  unsigned char pre[8];
  for (int k = 0; k < 4; ++k) pre[k] = (unsigned char)type[k];
  for (int k = 0; k < nextra; ++k) pre[4 + k] = extra[k];
  if (lane == 0) {
    png_be32(dst, n + (unsigned)nextra);
    for (int k = 0; k < 4 + nextra; ++k) dst[4 + k] = pre[k];
  }
  unsigned char *body = dst + 8 + nextra;
  for (unsigned i = lane; i < n; i += 64) body[i] = data[i];
  const uint32_t crc = png_wave_crc(tab, pre, 4 + nextra, data, n, lane);
  if (lane == 0) png_be32(body + n, crc);
}

// grid (nseg + 1, T), one wavefront each.  Block s < nseg: segment s of frame t as an IDAT chunk; block nseg: everything else
// of the file.
__global__ __launch_bounds__(64) void png_pack_kernel(const unsigned char *__restrict__ slots, const uint4 *__restrict__ meta,
                                                      const long long *__restrict__ offsets, unsigned char *__restrict__ blob,
                                                      const PngPalette pal, int has_palette, int H, int W, int channels,
                                                      int seg_rows, size_t slot_bytes) {
  __shared__ uint32_t tab[256];
  __shared__ unsigned char small[768];
  const int lane = threadIdx.x;
  const int nseg = (int)gridDim.x - 1;
  const size_t t = blockIdx.y;
  const int s = blockIdx.x;
  for (int k = lane; k < 256; k += 64) tab[k] = png_crc_entry((uint32_t)k);
  const int head = PNG_FIXED_HEAD + (has_palette ? PNG_PLTE_BYTES : 0);
  unsigned char *file = blob + offsets[t];
  // bytes of the IDAT chunks before this one
  long long before = 0;
  const int upto = s < nseg ? s : nseg;
  for (int k = lane; k < upto; k += 64) before += PNG_CHUNK_EXTRA + (long long)meta[t * nseg + k].x;
  for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
  __syncthreads();
  if (s < nseg) {
    const unsigned char zlib_header[2] = {0x78, 0x01};      // deflate, 32 KiB window, fastest; 0x7801 % 31 == 0
    const unsigned len = meta[t * nseg + s].x;
    unsigned char *dst = file + head + before + (s > 0 ? 2 : 0);
    png_wave_chunk(tab, dst, "IDAT", zlib_header, s == 0 ? 2 : 0, slots + (t * nseg + s) * slot_bytes, len, lane);
    return;
  }
  if (lane == 0) {
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int k = 0; k < 8; ++k) file[k] = sig[k];
    png_be32(small, (uint32_t)W);
    png_be32(small + 4, (uint32_t)H);
    small[8] = 8;                                     // bit depth
    small[9] = channels == 3 ? 2 : (has_palette ? 3 : 0);      // colour type: truecolour / palette / grayscale
    small[10] = small[11] = small[12] = 0;            // compression, filter method, no interlace
  }
  __syncthreads();
  png_wave_chunk(tab, file + 8, "IHDR", nullptr, 0, small, 13u, lane);
  __syncthreads();
  if (has_palette) {
    for (int k = lane; k < 768; k += 64) small[k] = pal.rgb[k];
    __syncthreads();
    png_wave_chunk(tab, file + PNG_FIXED_HEAD, "PLTE", nullptr, 0, small, 768u, lane);
    __syncthreads();
  }
  if (lane == 0) {
    // Adler-32 of the frame's filtered bytes from the segments' sums: A starts at 1, B at 0; a segment of n bytes adds
    // n * A + w to B and a to A
    unsigned long long A = 1, B = 0;
    for (int k = 0; k < nseg; ++k) {
      const uint4 m = meta[t * nseg + k];
      const int row0 = k * seg_rows;
      const unsigned long long n = (unsigned long long)(H - row0 < seg_rows ? H - row0 : seg_rows) * (unsigned)(channels * W + 1);
      B = (B + n * A + m.z) % PNG_ADLER_MOD;
      A = (A + m.y) % PNG_ADLER_MOD;
    }
    small[0] = 1;                                     // BFINAL 1, BTYPE 00: the final, empty stored block
    small[1] = small[2] = 0;
    small[3] = small[4] = 0xff;
    png_be32(small + 5, (uint32_t)((B << 16) | A));
  }
  __syncthreads();
  unsigned char *tail = file + head + 2 + before;
  png_wave_chunk(tab, tail, "IDAT", nullptr, 0, small, 9u, lane);
  png_wave_chunk(tab, tail + PNG_CHUNK_EXTRA + 9, "IEND", nullptr, 0, small, 0u, lane);
}

inline bool png_aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }
inline bool png_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)W + 1 <= PNG_SEG_MAX; }

}  // namespace

#define ST static_cast<hipStream_t>(stream)

extern "C" size_t swem_png_capacity(int H, int W) {
  if (!png_shape_ok(H, W)) return 0;
  const PngLayout L = png_layout(H, W);
  return (size_t)PNG_FIXED_HEAD + PNG_PLTE_BYTES + 2 + (size_t)H * L.rw + (size_t)L.nseg * (PNG_STORED_EXTRA + PNG_CHUNK_EXTRA) +
         PNG_TAIL_BYTES;
}

extern "C" size_t swem_png_workspace(int T, int H, int W) {
  if (T < 1 || !png_shape_ok(H, W)) return 0;
  const PngLayout L = png_layout(H, W);
  return (size_t)T * L.nseg * (sizeof(uint4) + L.slot);
}

extern "C" int swem_png_encode_u8(void *stream, const unsigned char *maps, const unsigned char *palette768, unsigned char *blob,
                                  size_t blob_bytes, long long *offsets, int T, int H, int W, void *ws, size_t ws_bytes) {
  SWEM_REQUIRE(maps && blob && offsets && ws, SWEM_E_ARG, "png_encode: null pointer");
  SWEM_REQUIRE(png_aligned(ws, 16) && png_aligned(offsets, 8), SWEM_E_ARG,
               "png_encode: ws must be 16-byte aligned, offsets 8-byte aligned");
  SWEM_REQUIRE(png_shape_ok(H, W), SWEM_E_SHAPE, "png_encode: need H >= 1, W >= 1 and W + 1 <= 65535, got %dx%d", H, W);
  SWEM_REQUIRE(T >= 1 && T <= 65535, SWEM_E_SHAPE, "png_encode: need 1 <= T <= 65535 frames, got %d", T);
  const PngLayout L = png_layout(H, W);
  SWEM_REQUIRE(L.nseg < 0x7fffffff, SWEM_E_SHAPE, "png_encode: %d segments exceed one launch", L.nseg);
  SWEM_REQUIRE(blob_bytes >=(size_t)T * swem_png_capacity(H, W), SWEM_E_WORKSPACE,
               "png_encode: insufficient workspace: blob %zu < %zu bytes (T * swem_png_capacity)", blob_bytes,
               (size_t)T * swem_png_capacity(H, W));
  SWEM_REQUIRE(ws_bytes >= swem_png_workspace(T, H, W), SWEM_E_WORKSPACE, "png_encode: insufficient workspace: %zu < %zu bytes",
               ws_bytes, swem_png_workspace(T, H, W));
  uint4 *meta = static_cast<uint4 *>(ws);
  unsigned char *slots = static_cast<unsigned char *>(ws) + (size_t)T * L.nseg * sizeof(uint4);
  PngPalette pal;
  __builtin_memset(pal.rgb, 0, 768);
  if (palette768) __builtin_memcpy(pal.rgb, palette768, 768);
  const int has_palette = palette768 ? 1 : 0;
  const size_t lds = align_up((size_t)L.rows * L.rw, 4);      // <= 65536
  hipLaunchKernelGGL(png_encode_kernel, dim3((unsigned)L.nseg, (unsigned)T), dim3(64), lds, ST, maps, slots, meta, H, W, L.rows,
                     L.slot);
  SWEM_CHECK_LAUNCH("png_encode");
  hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(256), 0, ST, meta, offsets, T, L.nseg,
                     PNG_FIXED_HEAD + (has_palette ? PNG_PLTE_BYTES : 0));
  SWEM_CHECK_LAUNCH("png_offsets");
  hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)L.nseg + 1u, (unsigned)T), dim3(64), 0, ST, slots, meta, offsets, blob, pal,
                     has_palette, H, W, 1, L.rows, L.slot);
  SWEM_CHECK_LAUNCH("png_pack");
  return SWEM_OK;
}

namespace {
inline bool png_shape_ok_px(int H, int W, int channels) {
  return (channels == 1 || channels == 3) && H >= 1 && W >= 1 && (long long)channels * W + 1 <= PNG_SEG_MAX;
}
}  // namespace

extern "C" size_t swem_png_capacity_px(int H, int W, int channels) {
  if (!png_shape_ok_px(H, W, channels)) return 0;
  const PngLayout L = png_layout(H, channels * W);
  return (size_t)PNG_FIXED_HEAD + (channels == 1 ? PNG_PLTE_BYTES : 0) + 2 + (size_t)H * L.rw +
         (size_t)L.nseg * (PNG_STORED_EXTRA + PNG_CHUNK_EXTRA) + PNG_TAIL_BYTES;
}

extern "C" size_t swem_png_workspace_px(int T, int H, int W, int channels) {
  if (T < 1 || !png_shape_ok_px(H, W, channels)) return 0;
  const PngLayout L = png_layout(H, channels * W);
  return (size_t)T * L.nseg * (sizeof(uint4) + L.slot);
}

extern "C" int swem_png_encode_px_u8(void *stream, const unsigned char *pixels, int channels, const unsigned char *palette768,
                                     int codes, unsigned char *blob, size_t blob_bytes, long long *offsets, int T, int H, int W,
                                     void *ws, size_t ws_bytes) {
  SWEM_REQUIRE(pixels && blob && offsets && ws, SWEM_E_ARG, "png_encode_px: null pointer");
  SWEM_REQUIRE(png_aligned(ws, 16) && png_aligned(offsets, 8), SWEM_E_ARG,
               "png_encode_px: ws must be 16-byte aligned, offsets 8-byte aligned");
  SWEM_REQUIRE(channels == 1 || channels == 3, SWEM_E_ARG, "png_encode_px: channels is 1 or 3, got %d", channels);
  SWEM_REQUIRE(channels == 1 || !palette768, SWEM_E_ARG, "png_encode_px: a truecolour picture takes no palette");
  SWEM_REQUIRE(codes == SWEM_PNG_CODES_FIXED || codes == SWEM_PNG_CODES_DYNAMIC, SWEM_E_ARG,
               "png_encode_px: codes is SWEM_PNG_CODES_FIXED or SWEM_PNG_CODES_DYNAMIC, got %d", codes);
  SWEM_REQUIRE(png_shape_ok_px(H, W, channels), SWEM_E_SHAPE,
               "png_encode_px: need H >= 1, W >= 1 and channels * W + 1 <= 65535, got %dx%d with %d channels", H, W, channels);
  SWEM_REQUIRE(T >= 1 && T <= 65535, SWEM_E_SHAPE, "png_encode_px: need 1 <= T <= 65535 frames, got %d", T);
  const PngLayout L = png_layout(H, channels * W);
  SWEM_REQUIRE(L.nseg < 0x7fffffff, SWEM_E_SHAPE, "png_encode_px: %d segments exceed one launch", L.nseg);
  const size_t cap = swem_png_capacity_px(H, W, channels), need = swem_png_workspace_px(T, H, W, channels);
  SWEM_REQUIRE(blob_bytes >= (size_t)T * cap, SWEM_E_WORKSPACE,
               "png_encode_px: insufficient workspace: blob %zu < %zu bytes (T * swem_png_capacity_px)", blob_bytes, (size_t)T * cap);
  SWEM_REQUIRE(ws_bytes >= need, SWEM_E_WORKSPACE, "png_encode_px: insufficient workspace: %zu < %zu bytes", ws_bytes, need);
  uint4 *meta = static_cast<uint4 *>(ws);
  unsigned char *slots = static_cast<unsigned char *>(ws) + (size_t)T * L.nseg * sizeof(uint4);
  PngPalette pal;
  __builtin_memset(pal.rgb, 0, 768);
  if (palette768) __builtin_memcpy(pal.rgb, palette768, 768);
  const int has_palette = palette768 ? 1 : 0;
  const int dynamic = codes == SWEM_PNG_CODES_DYNAMIC ? 1 : 0;
  // the segment (<= 65536 bytes) and, behind it, the tables of the dynamic form: past 64 KiB for the longest rows
  const size_t lds = align_up((size_t)L.rows * L.rw, 16) + (dynamic ? sizeof(PngDynLds) : 0);
  SWEM_ALLOW_LDS(png_encode_px_kernel, 65536 + sizeof(PngDynLds));
  hipLaunchKernelGGL(png_encode_px_kernel, dim3((unsigned)L.nseg, (unsigned)T), dim3(64), lds, ST, pixels, slots, meta, H, W,
                     channels, dynamic, L.rows, L.slot);
  SWEM_CHECK_LAUNCH("png_encode_px");
  hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(256), 0, ST, meta, offsets, T, L.nseg,
                     PNG_FIXED_HEAD + (has_palette ? PNG_PLTE_BYTES : 0));
  SWEM_CHECK_LAUNCH("png_offsets");
  hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)L.nseg + 1u, (unsigned)T), dim3(64), 0, ST, slots, meta, offsets, blob, pal,
                     has_palette, H, W, channels, L.rows, L.slot);
  SWEM_CHECK_LAUNCH("png_pack");
  return SWEM_OK;
}
