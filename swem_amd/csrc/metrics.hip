// DAVIS J&F on the device (include/swem_hip_metrics.h): the integer sums of evaluation/davis2017/metrics.py:6-37 (db_eval_iou)
// and :57-119 (f_measure with the same-size _seg2bmap, :122-178) for all T frames and N objects of a sequence.
//
// Everything is integer work on binary images, done on 64-pixel words (bit x % 64 of word x / 64 = pixel x of a row; bits at
// x >= W are zero):
//   jf_pack_kernel   the only pass over bytes: 16 bytes per lane and map, every object's `pred == o && !void`, `gt == o && !void`
//                    compared four bytes at a time, four lanes' 16-bit results joined into a word -> bit-planes [T][N][2][H][Wd]
//   jf_match_kernel  one lane per word of a 64-row x 14-word tile: the two boundary maps (three XORs of shifted words and the
//                    last-row / last-column / corner rules) are staged in the LDS with a halo of r rows and one word; the disk
//                    dilation of a (left, centre, right) triple costs r one-pixel spreads and 2r row ORs (not (2r+1)^2 taps):
//                        acc = B(y);  for k = 1..r:  spread acc by one pixel isqrt(r^2-(k-1)^2) - isqrt(r^2-k^2) times;
//                                                    acc |= B(y+k) | B(y-k)
//                    since spread(A, a) | spread(B, b) = spread(spread(A, a-b) | B, b) for a >= b.  A triple is enough while
//                    r <= 64: what is missing left of `left` reaches the centre word only with the 65th spread.
//                    All six counts are popcounts taken here (inter / union from the mask words the boundary was made of: the
//                    pack pass then needs no sums and no atomics), summed per block, one integer atomic per block and count.
// The counts are zeroed by a memset node in front; integer sums: any block order gives the same result.
#include "common.h"
#include "../../include/swem_hip_metrics.h"

namespace {

typedef unsigned long long u64;

#define JF_RS 64     // rows of a tile
#define JF_WS 14     // words of a tile row (896 pixels: the whole row at 854)
#define JF_PITCH 16  // LDS words per staged row: one halo word on either side (128 bytes)

// 0x80 in every byte of x that is zero, 0 elsewhere (exact: the 7-bit sums cannot carry into the next byte)
__host__ __device__ inline unsigned zero_bytes(unsigned x) {
  return ~((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) | 0x7f7f7f7fu);
}
// bits 7, 15, 23, 31 -> bits 0..3 (the four partial products land on distinct bits: no carries)
__host__ __device__ inline unsigned top_bits(unsigned m) { return (((m >> 7) * 0x01020408u) >> 24) & 0xfu; }
// 16 pixels (four little-endian dwords): bit j set where pixel j == o and valid (valid: 0x80 per admissible byte)
__host__ __device__ inline unsigned eq16(const unsigned px[4], const unsigned valid[4], unsigned o) {
  const unsigned pat = o * 0x01010101u;
  unsigned m = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) m |= top_bits(zero_bytes(px[q] ^ pat) & valid[q]) << (4 * q);
  return m;
}

// _seg2bmap (metrics.py:160-178, the same-size branch) on a word: s = the mask word, s_next = the word right of it, d / d_next
// = the same of the row below (zero where the image ends, like the zero-filled e, s, se of the reference).  last_col_bit: the bit
// of pixel W-1 when this is the last word of a row, else 0.
__host__ __device__ inline u64 boundary_word(u64 s, u64 s_next, u64 d, u64 d_next, bool last_row, u64 last_col_bit) {
  const u64 e = (s >> 1) | (s_next << 63);
  const u64 de = (d >> 1) | (d_next << 63);
  u64 b = last_row ? (s ^ e) : ((s ^ e) | (s ^ d) | (s ^ de));                       // b[-1, :] = seg ^ e
  if (last_col_bit) b = (b & ~last_col_bit) | (last_row ? 0ull : ((s ^ d) & last_col_bit));   // b[:, -1] = seg ^ s; b[-1, -1] = 0
  return b;
}

struct Tri {
  u64 l, c, r;
};
// dilate by one pixel to either side, carried across the three words
__host__ __device__ inline void spread1(Tri &a) {
  const u64 l = a.l | (a.l << 1) | (a.l >> 1) | (a.c << 63);
  const u64 c = a.c | (a.c << 1) | (a.c >> 1) | (a.l >> 63) | (a.r << 63);
  const u64 r = a.r | (a.r << 1) | (a.r >> 1) | (a.c >> 63);
  a.l = l;
  a.c = c;
  a.r = r;
}

// 16 bytes of a row from pixel x0 on as four dwords; pixels at x >= W read as 0 (never an object id, never void).
// The rows of a W = 854 map are not 16-byte aligned: the copy leaves the choice of the load to the compiler.
__device__ inline void load16(const unsigned char *__restrict__ row, int x0, int W, unsigned out[4]) {
  if (x0 + 16 <= W) {
    __builtin_memcpy(out, row + x0, 16);
  } else {
    out[0] = out[1] = out[2] = out[3] = 0;
    for (int j = 0; j < 16; ++j)
      if (x0 + j < W) out[j >> 2] |= (unsigned)row[x0 + j] << (8 * (j & 3));
  }
}

// One wave per 1024 pixels of a row (16 words); planes [T][N][2][H][Wd], plane 0 = prediction, 1 = annotation.
__global__ __launch_bounds__(256) void jf_pack_kernel(const unsigned char *__restrict__ gt,
                                                      const unsigned char *__restrict__ pred,
                                                      const unsigned char *__restrict__ vd, u64 *__restrict__ planes, int N,
                                                      int H, int W, int Wd, int chunks, long long items) {
  const int lane = threadIdx.x & 63;
  const long long nwaves = (long long)gridDim.x * 4;
  const size_t plane = (size_t)H * Wd;
  for (long long it = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += nwaves) {   // (wave-uniform)
    const int chunk = (int)(it % chunks);
    const long long row = it / chunks;   // t * H + y
    const int y = (int)(row % H);
    const long long t = row / H;
    const int x0 = chunk * 1024 + lane * 16;
    const size_t off = (size_t)row * W;
    unsigned g[4], p[4], valid[4];
    load16(gt + off, x0, W, g);
    load16(pred + off, x0, W, p);
    if (vd) {
      unsigned v[4];
      load16(vd + off, x0, W, v);
#pragma unroll
      for (int q = 0; q < 4; ++q) valid[q] = zero_bytes(v[q]);
    } else {
      valid[0] = valid[1] = valid[2] = valid[3] = 0x80808080u;
    }
    const int wi = chunk * 16 + (lane >> 2);
    const bool writer = (lane & 3) == 0 && wi < Wd;
    const int sh = 16 * (lane & 3);
    u64 *dst = planes + (size_t)t * N * 2 * plane + (size_t)y * Wd + wi;
    for (int o = 1; o <= N; ++o, dst += 2 * plane) {
      u64 pw = (u64)eq16(p, valid, (unsigned)o) << sh;
      u64 gw = (u64)eq16(g, valid, (unsigned)o) << sh;
      pw |= __shfl_xor(pw, 1);
      gw |= __shfl_xor(gw, 1);
      pw |= __shfl_xor(pw, 2);
      gw |= __shfl_xor(gw, 2);
      if (writer) {
        dst[0] = pw;
        dst[plane] = gw;
      }
    }
  }
}

__device__ inline u64 boundary_at(const u64 *__restrict__ S, int y, int wi, int H, int Wd, u64 colbit) {
  const u64 *p = S + (size_t)y * Wd + wi;
  const bool lastw = wi == Wd - 1, lastr = y == H - 1;
  const u64 s = p[0], sn = lastw ? 0ull : p[1];
  const u64 d = lastr ? 0ull : p[Wd], dn = (lastr || lastw) ? 0ull : p[Wd + 1];
  return boundary_word(s, sn, d, dn, lastr, lastw ? colbit : 0ull);
}

// One block per (frame, object, tile of JF_RS rows x JF_WS words); dynamic LDS: [2][JF_RS + 2r][JF_PITCH] words.
__global__ __launch_bounds__(256) void jf_match_kernel(const u64 *__restrict__ planes, int *__restrict__ counts, int H, int W,
                                                       int Wd, int r, int tiles_x, int tiles_y) {
  extern __shared__ u64 jf_lds[];
  __shared__ int red[4][SWEM_JF_COUNTS];
  const int rows = JF_RS + 2 * r;
  u64 *Bf = jf_lds, *Bg = jf_lds + rows * JF_PITCH;
  long long b = blockIdx.x;
  const int tx = (int)(b % tiles_x);
  b /= tiles_x;
  const int ty = (int)(b % tiles_y);
  const long long to = b / tiles_y;   // t * N + (o - 1)
  const int y0 = ty * JF_RS, w0 = tx * JF_WS;
  const size_t plane = (size_t)H * Wd;
  const u64 *P = planes + (size_t)to * 2 * plane, *G = P + plane;
  const u64 colbit = 1ull << ((W - 1) & 63);

  // boundary words of rows y0-r .. y0+JF_RS+r-1, words w0-1 .. w0+JF_WS; zero outside the image
  for (int i = threadIdx.x; i < rows * JF_PITCH; i += 256) {
    const int y = y0 - r + i / JF_PITCH, wi = w0 - 1 + i % JF_PITCH;
    u64 bf = 0, bg = 0;
    if (y >= 0 && y < H && wi >= 0 && wi < Wd) {
      bf = boundary_at(P, y, wi, H, Wd, colbit);
      bg = boundary_at(G, y, wi, H, Wd, colbit);
    }
    Bf[i] = bf;
    Bg[i] = bg;
  }
  __syncthreads();

  int c[SWEM_JF_COUNTS] = {0, 0, 0, 0, 0, 0};
  const int th = min(JF_RS, H - y0), tw = min(JF_WS, Wd - w0);
  for (int i = threadIdx.x; i < th * tw; i += 256) {
    const int ry = i / tw, rx = i % tw;
    const size_t gi = (size_t)(y0 + ry) * Wd + (w0 + rx);
    const u64 p = P[gi], q = G[gi];
    c[SWEM_JF_INTER] += __popcll(p & q);
    c[SWEM_JF_UNION] += __popcll(p | q);
    const u64 *f = Bf + (ry + r) * JF_PITCH + (rx + 1), *g = Bg + (ry + r) * JF_PITCH + (rx + 1);
    const u64 bf = f[0], bg = g[0];
    if ((bf | bg) == 0) continue;   // no boundary pixel in this word: nothing to match (most words of a frame)
    c[SWEM_JF_N_FG] += __popcll(bf);
    c[SWEM_JF_N_GT] += __popcll(bg);
    Tri af = {f[-1], bf, f[1]}, ag = {g[-1], bg, g[1]};
    int cur = r;   // isqrt(r*r - (k-1)*(k-1)): the half-width of the disk's row k-1
    for (int k = 1; k <= r; ++k) {
      const int lim = r * r - k * k;
      while (cur * cur > lim) {
        spread1(af);
        spread1(ag);
        --cur;
      }
      const u64 *fu = f - k * JF_PITCH, *fd = f + k * JF_PITCH, *gu = g - k * JF_PITCH, *gd = g + k * JF_PITCH;
      af.l |= fu[-1] | fd[-1];
      af.c |= fu[0] | fd[0];
      af.r |= fu[1] | fd[1];
      ag.l |= gu[-1] | gd[-1];
      ag.c |= gu[0] | gd[0];
      ag.r |= gu[1] | gd[1];
    }
    c[SWEM_JF_FG_MATCH] += __popcll(bf & ag.c);
    c[SWEM_JF_GT_MATCH] += __popcll(bg & af.c);
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < SWEM_JF_COUNTS; ++j) {
    int v = c[j];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) red[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < SWEM_JF_COUNTS) {
    const int v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (v) atomicAdd(counts + to * SWEM_JF_COUNTS + threadIdx.x, v);
  }
}

}  // namespace

#define ST static_cast<hipStream_t>(stream)

extern "C" size_t swem_jf_workspace(int T, int N, int H, int W) {
  if (T <= 0 || N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)T * N * 2 * H * ((W + 63) / 64) * sizeof(u64);
}

extern "C" int swem_jf_counts_u8(void *stream, const unsigned char *gt, const unsigned char *pred,
                                 const unsigned char *void_or_null, int *counts, int T, int N, int H, int W, int r, void *ws,
                                 size_t ws_bytes) {
  SWEM_REQUIRE(gt && pred && counts && ws, SWEM_E_ARG, "jf_counts: null pointer");
  SWEM_REQUIRE(((uintptr_t)ws % 8) == 0 && ((uintptr_t)counts % 4) == 0, SWEM_E_ARG,
               "jf_counts: ws must be 8-byte aligned, counts 4-byte aligned");
  SWEM_REQUIRE(T > 0 && N > 0 && N <= 255 && H > 0 && W > 0, SWEM_E_SHAPE,
               "jf_counts: need T, H, W > 0 and 1 <= N <= 255 objects (uint8 ids), got T=%d N=%d H=%d W=%d", T, N, H, W);
  SWEM_REQUIRE(r >= 0 && r <= SWEM_JF_MAX_RADIUS, SWEM_E_SHAPE,
               "jf_counts: disk radius %d outside 0..%d (the dilation works on three 64-pixel words)", r, SWEM_JF_MAX_RADIUS);
  const int Wd = (W + 63) / 64;
  const int tiles_x = cdiv(Wd, JF_WS), tiles_y = cdiv(H, JF_RS);
  const long long blocks = (long long)T * N * tiles_x * tiles_y;
  const int chunks = cdiv(W, 1024);
  const long long items = (long long)T * H * chunks;
  SWEM_REQUIRE(blocks <= 0x7fffffffLL && (long long)T * N * SWEM_JF_COUNTS <= 0x7fffffffLL, SWEM_E_SHAPE,
               "jf_counts: %lld tiles exceed one launch", blocks);
  SWEM_REQUIRE(ws_bytes >= swem_jf_workspace(T, N, H, W), SWEM_E_WORKSPACE, "jf_counts: workspace %zu < %zu bytes", ws_bytes,
               swem_jf_workspace(T, N, H, W));
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)T * N * SWEM_JF_COUNTS * sizeof(int), ST);
  if (e != hipSuccess) {
    swem_set_error("jf_counts: hipMemsetAsync: %s", hipGetErrorString(e));
    return SWEM_E_HIP;
  }
  const long long pack_blocks = (items + 3) / 4;
  hipLaunchKernelGGL(jf_pack_kernel, dim3((unsigned)(pack_blocks < 2048 ? pack_blocks : 2048)), dim3(256), 0, ST, gt, pred,
                     void_or_null, static_cast<u64 *>(ws), N, H, W, Wd, chunks, items);
  SWEM_CHECK_LAUNCH("jf_pack");
  const size_t lds = (size_t)2 * (JF_RS + 2 * r) * JF_PITCH * sizeof(u64);   // <= 48 KiB at r = 64
  hipLaunchKernelGGL(jf_match_kernel, dim3((unsigned)blocks), dim3(256), lds, ST, static_cast<const u64 *>(ws), counts, H, W,
                     Wd, r, tiles_x, tiles_y);
  SWEM_CHECK_LAUNCH("jf_match");
  return SWEM_OK;
}
