// What every convolution unit shares: the launch parameters (ConvP), the launchers' prototypes, and the device helpers of
// all kernel families -- tile order, tap arithmetic, the row-layout epilogue with its output planes.
//   conv.hip           host side: plans, workspace, the C entry points; the split-K reducer and the operand-split kernels
//   conv_f32.hip       the kernels that read fp32 maps (conv_igemm_kernel, _pipe_, _bf3_)
//   conv_presplit.hip  conv_igemm_bf3s_kernel (pre-split operand planes) and its instantiations
//   conv_t256.hip      conv_t256_kernel (the 256-column tiles)
//   conv_mma16.h       what the kernels on the 16-bit matrix cores share
#pragma once
#include "common.h"
#include "lds_dma.h"
#include "bf16_split.h"

constexpr int BK = 32;
constexpr int KQ = BK / 4;  // float4 slots per row per k-block

struct ConvP {
  const float *x[3];
  int c[3];
  long long bs[3];
  int B, H, W, Ho, Wo, Cin, K, M;
  const float *w, *scale, *shift, *res;
  float uscale;  // the scale of every output column where `scale` is NULL (1; matching's readout undoes its operand scaling here)
  long long res_bs, w_bs;  // w_bs: elements between the filter banks of consecutive batch items (0 = shared)
  const unsigned short *wsplit;  // optional [3][Ncols][K] bf16: the filters pre-split into hi/mid/lo planes
  const unsigned short *xs[3];   // pre-split activations (conv_igemm_bf3s_kernel): plane 0 of each source
  long long ps[3];               // ... and the element stride between a source's three planes
  int bsp[3], npx[3];            // pre-split sources: batch stride in pixels, pixels per plane (host-side divisions)
  float *y;
  int Cout, Ncols, KH, KW, stride, pad, flags;
  int nkb, kb_per_split;
  float *partial;
  int nplanes;  // 3 = bf16x6 (hi/mid/lo planes, six products), 2 = three products on (hi, mid), 1 = plain bf16 (hi plane only)
  int f16;      // nplanes == 2 only: the operand planes are fp16 pairs (bf16_split.h, split2h) -- the "f16x3" arithmetic
  int xpn;      // XCD partition of the N tiles (1, 2, 4, 8): see tile_coords
  int mt0;      // first M tile of this launch (the tail launch of a tail-split layer starts further down)
  int part_m0;  // first output row held by `partial` (rows are stored relative to it)
  // Optional: the output's bf16 planes, written by the epilogue itself for the convolutions that will consume this tensor
  // pre-split (the layout swem_split_bf16x3_f32 produces, [plane][Cout/8][M][8]): variant 0 = the planes of y, variant 1 =
  // the planes of relu(y) (a consumer that applies its input ReLU while splitting).  NULL = not wanted.
  // Optional: the residual as operand PLANES instead of an fp32 map (round 4): a block output that only convolutions and the
  // next block's residual add consume is written as planes only, and the add reads it back from them -- hi + mid of the fp16
  // pair (exact in fp32: the value to 22-23 significant bits) or hi + mid + lo of three bf16 planes (exactly the value).
  const unsigned short *res_pl;   // plane 0 of the residual, [C/8][res_npx][8]; NULL = the fp32 map `res`
  long long res_ps;               // elements between its planes
  int res_npx, res_npl;           // pixels per plane; SWEM_PLANES_F16 or 3
  unsigned short *ysp[2];
  int ysp_npl[2];     // planes to write per variant: 2 (hi, mid: all consumers run bf16x3) or 3
  long long ysp_ps;   // elements between the planes (M * Cout)
  // Stream-K (conv_igemm_bf3s_kernel, plan bits 24-27 == 1): sk_workers persistent blocks share the tiles x k-blocks
  // iteration space in equal contiguous ranges; see the kernel
  // n / HoWo and n / Wo for 0 <= n < 2^31 as umulhi(n, mul) >> sh (fast_div; a runtime integer division is ~40 dependent
  // vector instructions, and the row set-up of every block does four of them)
  unsigned fd_howo_mul, fd_howo_sh, fd_wo_mul, fd_wo_sh;
  int sk_workers, sk_mtiles, sk_ntiles;
  float *sk_ws;         // one block tile of fp32 partial sums per worker
  unsigned *sk_flags;   // one word per worker, zero at launch: "my partial tile is in sk_ws"
  int spin_limit;       // polls a block may spend waiting for another block's partial tile (2^24 ~ seconds; SWEM_SPIN_LIMIT)
  unsigned *fault;      // optional sticky fault word (the caller's, one per device: include/swem_hip.h): a bounded wait that expires
                        // or an output that does not fit the fp16 pair it is written as ORs SWEM_FAULT_* into it -- the tile is
                        // then wrong, and the host can know (never cleared on the device)
};

// The launchers, one per kernel unit.  Each picks its instantiation and enqueues it; the caller checks the launch.
// conv_f32.hip: tile wm x wn of 64 rows/columns; emulate = bf16x6 on the bf16 matrix cores, pipe_ok = every source a multiple
// of 32 channels (the buffer-load kernels), single = conv_igemm_kernel without its second LDS buffer
int swem_conv_f32_launch(const ConvP &p, int wm, int wn, bool emulate, bool pipe_ok, bool single, dim3 grid, hipStream_t st);
// conv_presplit.hip: variant = plan bits 20-23.  occ != nullptr: launch nothing, report the resident blocks per CU of the
// instantiation the launch would use (0 = this variant has no stream-K form)
int swem_conv_presplit_launch(const ConvP &p, int wm, int wn, int variant, dim3 grid, hipStream_t st, int *occ);
// conv_t256.hip: trows = rows of a tile (128, 160, 192, 224 or 256)
int swem_conv_t256_launch(const ConvP &p, int trows, dim3 grid, hipStream_t st);

namespace {

// One v_max_f32 per element.  fmaxf() costs two (hipcc first canonicalises the operand with v_max x,x), and in the fp32
// MFMA k-loop every vector instruction is time taken from the matrix pipe.  NaN inputs map to 0 (IEEE maxNum),
// like ATen's clamp-based ReLU on this path's finite activations.
__device__ __forceinline__ float relu1(float x) {
  float y;
  asm("v_max_f32 %0, 0, %1" : "=v"(y) : "v"(x));
  return y;
}
// XCD-aware tile order.  Workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2), so the
// linear id is remapped to give every XCD one contiguous range of tiles, with the N tiles of one M tile adjacent:
// the tiles that share activation rows (same M tile, neighbouring M tiles' 3x3 halo) then hit the same L2.
// With xpn > 1 the N tiles are first cut into xpn groups and the order runs group by group (M tiles outer, the group's
// N tiles inner): 8 / xpn XCDs share one group and split its M tiles, so an XCD fetches 1/xpn of the filters and
// xpn/8 of the activations instead of all filters and 1/8 of the activations -- the cheaper cut where the filters
// outweigh the activations (the 30x54 layers: 60 MB of filter planes against 20 MB of activation planes).
// Placement only changes speed, never results.
__device__ __forceinline__ void tile_coords(int &mt, int &nt, int xpn = 1) {
  const int nwg = gridDim.x * gridDim.y, id = blockIdx.x + blockIdx.y * gridDim.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = id & 7, local = id >> 3;
  const int nid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
  const int ng = (int)gridDim.y / xpn, G = (int)gridDim.x * ng;   // N tiles per group, tiles per group
  const int jn = nid / G, rem = nid - jn * G;
  mt = rem / ng;
  nt = jn * ng + rem - mt * ng;
}

__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)); }

// zero a loaded vector with a bit mask: the value is used unconditionally, so the load itself stays unconditional
__device__ __forceinline__ float4 mask4(float4 v, bool keep) {
  const unsigned m = keep ? 0xffffffffu : 0u;
  return make_float4(__uint_as_float(__float_as_uint(v.x) & m), __uint_as_float(__float_as_uint(v.y) & m),
                     __uint_as_float(__float_as_uint(v.z) & m), __uint_as_float(__float_as_uint(v.w) & m));
}

// floor(n / d) for 0 <= n < 2^31 by a host-made multiplier: mul = floor(2^(31+l) / d) + 1, sh = l - 1 with l = ceil(log2 d)
// (checked exhaustively against // for d < 3000 and on random d < 2^22); d = 1 is mul = 0.
static inline void fast_div_make(unsigned d, unsigned &mul, unsigned &sh) {
  if (d <= 1) {
    mul = 0; sh = 0;
    return;
  }
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  mul = (unsigned)(((1ull << (31 + l)) / d) + 1);
  sh = l - 1;
}
__device__ __forceinline__ int fast_div(int n, unsigned mul, unsigned sh) {
  return mul ? (int)(__umulhi((unsigned)n, mul) >> sh) : n;
}

// Source pixel coordinate of output coordinate o (carried as o0) under tap k.
//   forward:  o0 = o*stride - pad,  i = o0 + k
//   data gradient (SWEM_CONV_DGRAD: x is dY, the output is dX): o0 = o + pad, t = o0 - k must be a multiple of the
//   stride, i = t / stride  (stride 1 or 2).  Evaluated only when the tap changes, never inside the k-loop.
__device__ __forceinline__ bool tap_coord(const ConvP &p, int o0, int k, int lim, int &i) {
  if (p.flags & SWEM_CONV_DGRAD) {
    const int t = o0 - k;
    i = t >> (p.stride - 1);
    return t >= 0 && (t & (p.stride - 1)) == 0 && i < lim;
  }
  i = o0 + k;
  return (unsigned)i < (unsigned)lim;
}
__device__ __forceinline__ int tap_origin(const ConvP &p, int o) {
  return (p.flags & SWEM_CONV_DGRAD) ? o + p.pad : o * p.stride - p.pad;
}

// Position of a k-block in the K order: source, first channel within it, filter tap (block-uniform, advanced with scalars)
struct KPos {
  int src, ci0, ky, kx;
};

// ---- output staging of the epilogues -------------------------------------------------------------------------------
// A wave stages one 32-pixel x 32-channel tile of scaled accumulators in its own slice of the (now idle) operand LDS and
// takes it out in row layout (out_tile32), output planes included.  The split is bf16_split.h's (bit-identical to
// swem_split_bf16x3_f32).
constexpr int PL_STRIDE = 36;                     // dwords per staged row: 16-byte aligned, conflict-free b128 reads
constexpr int PL_BYTES = 32 * PL_STRIDE * 4;      // LDS bytes per wave
__device__ __forceinline__ unsigned *planes_lds() {
  extern __shared__ __attribute__((aligned(16))) char smem_pl[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  return reinterpret_cast<unsigned *>(smem_pl + wave * PL_BYTES);
}

// Four consecutive channels n..n+3 of residual pixel `pix` from its planes (see ConvP::res_pl): 8 bytes per plane.
__device__ __forceinline__ float4 residual_from_planes(const ConvP &p, long long pix, int n) {
  const unsigned short *q = p.res_pl + ((long long)(n >> 3) * p.res_npx + pix) * 8 + (n & 7);
  const uint2 h = *reinterpret_cast<const uint2 *>(q), m = *reinterpret_cast<const uint2 *>(q + p.res_ps);
  if (p.res_npl == SWEM_PLANES_F16)
    return make_float4(lo_f16(h.x) + lo_f16(m.x), hi_f16(h.x) + hi_f16(m.x), lo_f16(h.y) + lo_f16(m.y), hi_f16(h.y) + hi_f16(m.y));
  const uint2 l = *reinterpret_cast<const uint2 *>(q + 2 * p.res_ps);
  return make_float4((lo_f32(h.x) + lo_f32(m.x)) + lo_f32(l.x), (hi_f32(h.x) + hi_f32(m.x)) + hi_f32(l.x),
                     (lo_f32(h.y) + lo_f32(m.y)) + lo_f32(l.y), (hi_f32(h.y) + hi_f32(m.y)) + hi_f32(l.y));
}

// One 32 x 32 tile of SCALED accumulators (acc * scale + shift), staged by the wave in its LDS slice in row order, goes
// out in ROW layout: lane (row id / 8, channel group id % 8) holds four consecutive channels of one pixel, adds the residual
// (or applies the mask) from a 16-byte load, applies the ReLU, stores 16 bytes of y -- an instruction covers 8 rows x 128
// bytes, against 4 rows x 64 bytes (or 2 x 128) of a dword store from the accumulator layout: a quarter of the store
// instructions (the epilogue was store-issue bound: 9.8k cycles of a 128x128 block, 4.6k of a 64x64 one) -- and writes the
// bf16 planes of the final values (an even lane and its odd neighbour hold the 8 channels of one 16-byte run).
__device__ __forceinline__ void out_tile32(const ConvP &p, const unsigned *lds, int m_base, int n_base) {
  const int lane = threadIdx.x & 63;
  const bool relu_out = p.flags & SWEM_CONV_RELU_OUT;
  const int HoWo = p.Ho * p.Wo;
  unsigned bad = 0;   // a value this lane wrote into an fp16 pair was beyond the fp16 range (SWEM_FAULT_RANGE)
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's staging writes have landed
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int id = lane + 64 * c, row = id >> 3, cg = id & 7;
    const int m = m_base + row, n = n_base + 4 * cg;
    const uint4 raw = *reinterpret_cast<const uint4 *>(lds + row * PL_STRIDE + 4 * cg);
    float4 v = make_float4(__uint_as_float(raw.x), __uint_as_float(raw.y), __uint_as_float(raw.z), __uint_as_float(raw.w));
    const bool in = m < p.M && n < p.Cout;
    if (in && (p.res || p.res_pl)) {
      const int b = fast_div(m, p.fd_howo_mul, p.fd_howo_sh);
      // (res_bs: fp32 elements between batch items, 0 = one image for the whole batch; the planes' pixel index follows from it)
      const float4 rv = p.res_pl ? residual_from_planes(p, (long long)b * (p.res_bs / p.Cout) + (m - b * HoWo), n)
                                 : *reinterpret_cast<const float4 *>(p.res + (long long)b * p.res_bs + (long long)(m - b * HoWo) * p.Cout + n);
      if (p.flags & SWEM_CONV_MASK_POS) {
        v = make_float4(rv.x > 0.f ? v.x : 0.f, rv.y > 0.f ? v.y : 0.f, rv.z > 0.f ? v.z : 0.f, rv.w > 0.f ? v.w : 0.f);
      } else {
        v.x += rv.x; v.y += rv.y; v.z += rv.z; v.w += rv.w;
      }
    }
    // (a NaN must not leave through a ReLU as a clean 0 in an fp16 pair without a trace -- fmaxf(NaN, 0) = 0, and the planes of
    // relu(y) may be the only output: the range test below looks at the value BEFORE any ReLU too)
    const unsigned nan_in = f32_nan(v);
    if (relu_out) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
    if (in && p.y) *reinterpret_cast<float4 *>(p.y + (long long)m * p.Cout + n) = v;   // (y = NULL: planes-only output)
#pragma unroll
    for (int var = 0; var < 2; ++var) {
      if (!p.ysp[var]) continue;
      const float4 q = var ? relu4(v) : v;
      uint2 h, mm, l;
      unsigned oor = 0;
      split_as(p.ysp_npl[var], q, h, mm, l, oor);
      if (p.ysp_npl[var] == SWEM_PLANES_F16) oor |= nan_in;
      if (in) bad |= oor;
      const uint2 h2 = make_uint2(__shfl_down(h.x, 1), __shfl_down(h.y, 1));
      const uint2 m2 = make_uint2(__shfl_down(mm.x, 1), __shfl_down(mm.y, 1));
      const uint2 l2 = make_uint2(__shfl_down(l.x, 1), __shfl_down(l.y, 1));
      if (in && (cg & 1) == 0) {
        unsigned short *d = p.ysp[var] + ((long long)(n >> 3) * p.M + m) * 8;
        *reinterpret_cast<uint4 *>(d) = make_uint4(h.x, h.y, h2.x, h2.y);
        *reinterpret_cast<uint4 *>(d + p.ysp_ps) = make_uint4(mm.x, mm.y, m2.x, m2.y);
        if (p.ysp_npl[var] == 3) *reinterpret_cast<uint4 *>(d + 2 * p.ysp_ps) = make_uint4(l.x, l.y, l2.x, l2.y);
      }
    }
  }
  if (p.ysp[0] || p.ysp[1]) range_fault(p.fault, bad);
  __builtin_amdgcn_s_waitcnt(0xc07f);   // the reads are done before the next tile is staged
}

// Epilogue shared by both kernels: raw split-K partials, or scale/shift (+residual, ReLU) / GLU gate, NHWC stores.
template <int WM, int WN>
__device__ __forceinline__ void conv_epilogue(const ConvP &p, f32x16 (&acc)[WM][WN], int m0, int n0, int wm, int wn,
                                              int r, int h) {
  const int mrow0 = m0 + wm * 32 * WM;
  const int ncol0 = n0 + wn * 32 * WN;
  if (p.partial) {  // split-K: raw partial sums, [z][M][Ncols]
    float *dst = p.partial + (long long)blockIdx.z * (p.M - p.part_m0) * p.Ncols - (long long)p.part_m0 * p.Ncols;
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int jn = 0; jn < WN; ++jn) {
        int n = ncol0 + 32 * jn + r;
        if (n >= p.Ncols) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          int m = mrow0 + 32 * i + acc_row(e, h);
          if (m < p.M) dst[(long long)m * p.Ncols + n] = acc[i][jn][e];
        }
      }
    return;
  }
  if constexpr (WN == 2) {
    if (p.flags & SWEM_CONV_GLU) {
      // packed columns [group][f|a][32]: this wave's two N tiles are the f and a banks of one group; the gated values go
      // through the wave's LDS slice and out in row layout like every other output (16-byte stores, bf16 planes)
      const int nf = ncol0 + r, na = ncol0 + 32 + r;
      const bool nin = na < p.Ncols;
      const float scf = (nin && p.scale) ? p.scale[nf] : p.uscale, sca = (nin && p.scale) ? p.scale[na] : p.uscale;
      const float shf = (nin && p.shift) ? p.shift[nf] : 0.f, sha = (nin && p.shift) ? p.shift[na] : 0.f;
      __syncthreads();   // every wave is done with the operand stages
      unsigned *lds = planes_lds();
#pragma unroll
      for (int i = 0; i < WM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float f = acc[i][0][e] * scf + shf, a = acc[i][1][e] * sca + sha;
          lds[acc_row(e, h) * PL_STRIDE + r] = __float_as_uint(f * sigmoidf_(a));
        }
        out_tile32(p, lds, mrow0 + 32 * i, nin ? (ncol0 >> 1) : p.Cout);
      }
      return;
    }
  }
  __syncthreads();   // every wave is done with the operand stages: the LDS is free for the output staging
  unsigned *lds = planes_lds();
#pragma unroll
  for (int jn = 0; jn < WN; ++jn) {
    const int n = ncol0 + 32 * jn + r;
    const bool nin = n < p.Ncols;
    const float sc = (nin && p.scale) ? p.scale[n] : p.uscale, sh = (nin && p.shift) ? p.shift[n] : 0.f;
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) lds[acc_row(e, h) * PL_STRIDE + r] = __float_as_uint(acc[i][jn][e] * sc + sh);
      out_tile32(p, lds, mrow0 + 32 * i, ncol0 + 32 * jn);
    }
  }
}

// dynamic LDS of a launch: the operand stages, or -- where a small tile's stages are smaller -- the plane staging of the
// epilogue (one PL_BYTES slice per wave), when output planes are wanted
static inline size_t lds_with_planes(const ConvP &p, size_t lds, int nwaves) {
  (void)p;
  const size_t need = (size_t)nwaves * PL_BYTES;   // (round 3: every epilogue stages its outputs, planes wanted or not)
  return lds < need ? need : lds;
}

}  // namespace
