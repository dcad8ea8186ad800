// The convolution kernels that read fp32 maps (GEMM view: conv.hip): conv_igemm_kernel on the fp32 matrix cores, its
// buffer-load variant conv_igemm_pipe_kernel, and conv_igemm_bf3_kernel, which splits the operands while staging them.
//
// conv_igemm_kernel: block = 256 threads = 4 waves in a 2x2 grid; wave tile = (32*WM) x (32*WN) outputs built from
// v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fma chain).  K is walked in 32-wide blocks that
// are register-staged (global -> VGPR while the previous block is multiplied, then VGPR -> LDS)
// into a double-buffered LDS image  [k/4][row][4 floats], row stride padded by one 16-byte slot:
//   - the 8 lanes that write one row hit 8 different slots (stride BM+1 is odd),
//   - a ds_read_b128 of 16 consecutive rows is conflict free,
//   - one float4 per operand feeds 4 MFMAs (lane half h owns k = 4*(2j+h)..+3).
// The epilogue applies scale/shift (bias + folded frozen BatchNorm), the residual, ReLU or the GLU gate
// and stores NHWC: 32 consecutive channels per half wave = one 128-byte segment.
#include "conv_mma16.h"

namespace {

template <int WM, int WN, bool DB>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvP p) {
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int SA = BM + 1, SB = BN + 1;  // row strides in float4 slots
  constexpr int RA = BM / 32, RB = BN / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4 *As = reinterpret_cast<float4 *>(smem);  // [2][KQ][SA]
  constexpr int NBUF = DB ? 2 : 1;
  float4 *Bs = As + NBUF * KQ * SA;               // [NBUF][KQ][SB]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  int tm, tn;
  tile_coords(tm, tn);
  tm += p.mt0;
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- per-thread gather coordinates (fixed over the K loop) ----
  const int kq = tid & 7, rbase = tid >> 3;
  int iy0[RA], ix0[RA], bidx[RA];
  bool rowok[RA];
  const int HoWo = p.Ho * p.Wo;
#pragma unroll
  for (int i = 0; i < RA; ++i) {
    int m = m0 + rbase + 32 * i;
    rowok[i] = m < p.M;
    int b = m / HoWo;
    int rem = m - b * HoWo;
    int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    iy0[i] = tap_origin(p, oy);
    ix0[i] = tap_origin(p, ox);
    bidx[i] = b;
  }
  const float *wrow[RB];
  bool colok[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    int n = n0 + rbase + 32 * i;
    colok[i] = n < p.Ncols;
    wrow[i] = p.w + (long long)(m0 / (p.Ho * p.Wo)) * p.w_bs + (long long)(colok[i] ? n : 0) * p.K;
  }
  const bool relu_in = p.flags & SWEM_CONV_RELU_IN;

  float4 ga[RA], gb[RB];
  unsigned okbits = 0;  // validity of the staged vectors: bit i = A row i, bit 8+i = B row i (applied at the LDS store)
  // Loads are unconditional (out-of-image taps read a clamped in-bounds address and are zeroed by a select) so the
  // compiler issues all of them back to back with ONE wait before the LDS stores; the input ReLU is applied at the
  // store, not at the load (a use right behind each load would serialise the L2 round trips).
  auto gload = [&](int kb) {
    const int k = kb * BK + kq * 4;
    const bool kok = k < p.K;
    const int kc = kok ? k : 0;
    unsigned bits = 0;
    int tap = kc / p.Cin;
    int ci = kc - tap * p.Cin;
    int ky = tap / p.KW, kx = tap - ky * p.KW;
    // channel -> (source, local channel) by selects: no runtime-indexed arrays (they would go to scratch)
    const float *src = p.x[0];
    int cs = p.c[0];
    long long sbs = p.bs[0];
    if (ci >= p.c[0]) {
      ci -= p.c[0];
      src = p.x[1];
      cs = p.c[1];
      sbs = p.bs[1];
      if (ci >= p.c[1]) {
        ci -= p.c[1];
        src = p.x[2];
        cs = p.c[2];
        sbs = p.bs[2];
      }
    }
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      int iy = iy0[i] + ky, ix = ix0[i] + kx;
      bool ok = kok && rowok[i] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      long long off = ok ? bidx[i] * sbs + ((long long)iy * p.W + ix) * cs + ci : 0;
      ga[i] = *reinterpret_cast<const float4 *>(src + off);
      bits |= ok ? (1u << i) : 0u;
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      gb[i] = *reinterpret_cast<const float4 *>(wrow[i] + kc);
      bits |= (kok && colok[i]) ? (1u << (8 + i)) : 0u;
    }
    okbits = bits;
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      float4 v = mask4(ga[i], (okbits >> i) & 1u);
      As[(buf * KQ + kq) * SA + rbase + 32 * i] = relu_in ? relu4(v) : v;
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) Bs[(buf * KQ + kq) * SB + rbase + 32 * i] = mask4(gb[i], (okbits >> (8 + i)) & 1u);
  };

  f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int kb_begin = blockIdx.z * p.kb_per_split;
  const int kb_end = min(p.nkb, kb_begin + p.kb_per_split);

  gload(kb_begin);
  lstore(0);
  __syncthreads();
  int buf = 0;
  for (int kb = kb_begin; kb < kb_end; ++kb) {
    const bool more = kb + 1 < kb_end;
    if (more) gload(kb + 1);
    const float4 *Ab = As + buf * KQ * SA + wm * 32 * WM + r + h * SA;
    const float4 *Bb = Bs + buf * KQ * SB + wn * 32 * WN + r + h * SB;
    // operand fragments are fetched one k-group ahead of the MFMAs that use them
    float4 a[2][WM], b[2][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i) a[0][i] = Ab[32 * i];
#pragma unroll
    for (int i = 0; i < WN; ++i) b[0][i] = Bb[32 * i];
#pragma unroll
    for (int j = 0; j < KQ / 2; ++j) {
      if (j + 1 < KQ / 2) {
#pragma unroll
        for (int i = 0; i < WM; ++i) a[(j + 1) & 1][i] = Ab[2 * (j + 1) * SA + 32 * i];
#pragma unroll
        for (int i = 0; i < WN; ++i) b[(j + 1) & 1][i] = Bb[2 * (j + 1) * SB + 32 * i];
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int jn = 0; jn < WN; ++jn) acc[i][jn] = mfma32x4(a[j & 1][i], b[j & 1][jn], acc[i][jn]);
      // keep the LDS reads of group j+1 ahead of the MFMAs of group j (the scheduler otherwise sinks them behind and
      // reuses the fragment registers, exposing the LDS latency: 124 vs 155 TFLOP/s in tools/mfma_lds.hip)
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (DB) {
      if (more) lstore(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    } else {
      // single LDS image: half the LDS, twice the resident blocks; other blocks' MFMAs cover this block's refill
      __syncthreads();
      if (more) lstore(0);
      __syncthreads();
    }
  }

  conv_epilogue<WM, WN>(p, acc, m0, n0, wm, wn, r, h);
}

// ------------------------------------------------------------------------------------------------------------
// Fast variant for the common case (every source width, hence Cin, a multiple of 32).
//
// Measured on gfx950 (profiles/r01_conv_pmc.txt): while v_mfma_f32_32x32x2_f32 runs, NO vector-ALU instruction
// co-executes (SQ_VALU_MFMA_COEXEC_CYCLES = 0: the fp32 MFMA runs at the fp32 vector rate on the same datapath), so
// every VALU instruction in the k-loop is time taken from the matrix pipe.  This kernel therefore keeps the loop free
// of vector arithmetic:
//   - a 32-wide k-block lies inside one tap of one source, so its position (source, tap, channel) is block-uniform
//     and advances with scalar instructions;
//   - operands are fetched with raw buffer loads: per-lane byte offsets are recomputed only when the tap or source
//     changes (every Cin/32 k-blocks), the channel offset travels in the scalar offset, and out-of-image taps /
//     out-of-range rows use an out-of-range offset, which the buffer unit returns as zeros (no masks, no branches);
//   - the only vector op left is the optional input ReLU on the staged values.
__device__ __forceinline__ void kpos_init(KPos &q, const ConvP &p, int kb) {
  int k = kb * BK;
  int tap = k / p.Cin;
  int ci = k - tap * p.Cin;
  q.ky = tap / p.KW;
  q.kx = tap - q.ky * p.KW;
  q.src = 0;
  if (ci >= p.c[0]) {
    ci -= p.c[0];
    q.src = 1;
    if (ci >= p.c[1]) {
      ci -= p.c[1];
      q.src = 2;
    }
  }
  q.ci0 = ci;
}

template <int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv_igemm_pipe_kernel(ConvP p) {
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int SA = BM + 1, SB = BN + 1;
  constexpr int RA = BM / 32, RB = BN / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4 *As = reinterpret_cast<float4 *>(smem);  // [2][KQ][SA]
  float4 *Bs = As + 2 * KQ * SA;                  // [2][KQ][SB]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  int tm, tn;
  tile_coords(tm, tn);
  tm += p.mt0;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kq = tid & 7, rbase = tid >> 3;

  // buffer descriptors (wave-uniform: built from kernel arguments and block-uniform scalars only)
  const long long HWin = (long long)p.H * p.W;
  auto src_rsrc = [&](int sidx) __attribute__((always_inline)) {
    const float *base = sidx == 0 ? p.x[0] : (sidx == 1 ? p.x[1] : p.x[2]);
    const int cs = sidx == 0 ? p.c[0] : (sidx == 1 ? p.c[1] : p.c[2]);
    const long long bs = sidx == 0 ? p.bs[0] : (sidx == 1 ? p.bs[1] : p.bs[2]);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0,
                                             (int)((bs ? (long long)p.B * bs : HWin * cs) * 4), 0x00020000);
  };
  __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(p.w + (long long)(m0 / (p.Ho * p.Wo)) * p.w_bs), 0, (int)((long long)p.Ncols * p.K * 4),
      0x00020000);

  int iy0[RA], ix0[RA], bidx[RA];
  const int HoWo = p.Ho * p.Wo;
#pragma unroll
  for (int i = 0; i < RA; ++i) {
    int m = m0 + rbase + 32 * i;
    int b = m / HoWo;
    int rem = m - b * HoWo;
    int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    iy0[i] = tap_origin(p, oy);
    ix0[i] = tap_origin(p, ox);
    bidx[i] = m < p.M ? b : -1;
  }
  unsigned wvoff[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    int n = n0 + rbase + 32 * i;
    wvoff[i] = n < p.Ncols ? (unsigned)(((long long)n * p.K + kq * 4) * 4) : OOB;
  }
  const bool relu_in = p.flags & SWEM_CONV_RELU_IN;

  // per-lane byte offsets of the A rows for the current (source, tap); recomputed only when that changes
  unsigned avoff[RA];
  auto set_tap = [&](const KPos &q) {
    const int cs = q.src == 0 ? p.c[0] : (q.src == 1 ? p.c[1] : p.c[2]);
    const long long bs = q.src == 0 ? p.bs[0] : (q.src == 1 ? p.bs[1] : p.bs[2]);
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      int iy, ix;
      const bool oky = tap_coord(p, iy0[i], q.ky, p.H, iy), okx = tap_coord(p, ix0[i], q.kx, p.W, ix);
      const bool ok = bidx[i] >= 0 && oky && okx;
      const long long e = bidx[i] * bs + ((long long)iy * p.W + ix) * cs + kq * 4;
      avoff[i] = ok ? (unsigned)(e * 4) : OOB;
    }
  };

  float4 ga[RA], gb[RB];
  __amdgpu_buffer_rsrc_t rsa;
  auto gload = [&](const KPos &q, int kb) {
    const unsigned soff = (unsigned)q.ci0 * 4u;
#pragma unroll
    for (int i = 0; i < RA; ++i) ga[i] = bufload4(rsa, avoff[i], soff);
    const unsigned wsoff = (unsigned)kb * (BK * 4u);
#pragma unroll
    for (int i = 0; i < RB; ++i) gb[i] = bufload4(rsw, wvoff[i], wsoff);
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < RA; ++i) As[(buf * KQ + kq) * SA + rbase + 32 * i] = relu_in ? relu4(ga[i]) : ga[i];
#pragma unroll
    for (int i = 0; i < RB; ++i) Bs[(buf * KQ + kq) * SB + rbase + 32 * i] = gb[i];
  };
  // advance to the next k-block (scalar); refresh the lane offsets when the tap or the source changes
  auto advance = [&](KPos &q) {
    q.ci0 += BK;
    const int cs = q.src == 0 ? p.c[0] : (q.src == 1 ? p.c[1] : p.c[2]);
    if (q.ci0 >= cs) {
      q.ci0 = 0;
      ++q.src;
      const int cn = q.src == 1 ? p.c[1] : (q.src == 2 ? p.c[2] : 0);
      if (cn == 0) {
        q.src = 0;
        if (++q.kx == p.KW) {
          q.kx = 0;
          ++q.ky;
        }
      }
      set_tap(q);
      rsa = src_rsrc(q.src);
    }
  };

  f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int kb_begin = blockIdx.z * p.kb_per_split;
  const int kb_end = min(p.nkb, kb_begin + p.kb_per_split);
  KPos q;
  kpos_init(q, p, kb_begin);
  set_tap(q);
  rsa = src_rsrc(q.src);
  gload(q, kb_begin);
  lstore(0);
  __syncthreads();
  int buf = 0;
  for (int kb = kb_begin; kb < kb_end; ++kb) {
    // the gathers for the next k-block are issued unconditionally (the last iteration re-reads its own block into the
    // idle buffer): a conditional definition of the staging registers costs register copies + early waits here
    const bool more = kb + 1 < kb_end;
    if (more) advance(q);
    gload(q, more ? kb + 1 : kb);
    const float4 *Ab = As + buf * KQ * SA + wm * 32 * WM + r + h * SA;
    const float4 *Bb = Bs + buf * KQ * SB + wn * 32 * WN + r + h * SB;
    float4 a[2][WM], b[2][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i) a[0][i] = Ab[32 * i];
#pragma unroll
    for (int i = 0; i < WN; ++i) b[0][i] = Bb[32 * i];
#pragma unroll
    for (int j = 0; j < KQ / 2; ++j) {
      if (j + 1 < KQ / 2) {
#pragma unroll
        for (int i = 0; i < WM; ++i) a[(j + 1) & 1][i] = Ab[2 * (j + 1) * SA + 32 * i];
#pragma unroll
        for (int i = 0; i < WN; ++i) b[(j + 1) & 1][i] = Bb[2 * (j + 1) * SB + 32 * i];
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int jn = 0; jn < WN; ++jn) acc[i][jn] = mfma32x4(a[j & 1][i], b[j & 1][jn], acc[i][jn]);
      __builtin_amdgcn_sched_barrier(0);
    }
    lstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  conv_epilogue<WM, WN>(p, acc, m0, n0, wm, wn, r, h);
}

// ------------------------------------------------------------------------------------------------------------
// fp32-accurate convolution on the bf16 matrix cores ("bf16x6"): every fp32 operand is split exactly into three bf16
// terms  x = hi + mid + lo  (8 + 8 + 8 significant bits, round-to-nearest residuals) while it is staged into LDS, and
// the product is rebuilt from the six term pairs above 2^-24:  hi*hi + hi*mid + mid*hi + hi*lo + lo*hi + mid*mid,
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16 (each bf16 x bf16 product is exact).  The dropped pairs are <= 2^-24
// relative, i.e. the result carries fp32-level error, at 16/6 = 2.7x the fp32-MFMA rate -- and, unlike the fp32 MFMA,
// the bf16 MFMA co-executes with the vector ALU, so the splitting arithmetic of one wave hides behind another's MFMAs.
// Same tiling, loads, k-block bookkeeping and epilogue as conv_igemm_pipe_kernel; LDS holds three bf16 planes per
// operand,  [plane][k/8][row][8 bf16], one 16-byte MFMA fragment per (row, k/8), plane stride padded by 16 bytes.
template <int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv_igemm_bf3_kernel(ConvP p) {
  constexpr bool PS = false;  // (pre-split filters in this register-staged variant were measured slower: more loads)
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int RA = BM / 32, RB = BN / 32;
  constexpr int SA = BM + 1, SB = BN + 1;          // k/8-group strides in 16-byte slots (+1: conflict-free stores)
  constexpr int PA = 4 * SA, PB = 4 * SB;         // plane strides
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4 *As = reinterpret_cast<uint4 *>(smem);  // [2 buffers][3 planes][PA]
  uint4 *Bs = As + 2 * 3 * PA;                  // [2][3][PB]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  int tm, tn;
  tile_coords(tm, tn);
  tm += p.mt0;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kq = tid & 7, rbase = tid >> 3;

  const long long HWin = (long long)p.H * p.W;
  auto src_rsrc = [&](int sidx) __attribute__((always_inline)) {
    const float *base = sidx == 0 ? p.x[0] : (sidx == 1 ? p.x[1] : p.x[2]);
    const int cs = sidx == 0 ? p.c[0] : (sidx == 1 ? p.c[1] : p.c[2]);
    const long long bs = sidx == 0 ? p.bs[0] : (sidx == 1 ? p.bs[1] : p.bs[2]);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0,
                                             (int)((bs ? (long long)p.B * bs : HWin * cs) * 4), 0x00020000);
  };
  __amdgpu_buffer_rsrc_t rsw =
      PS ? __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(p.wsplit), 0,
                                             (int)((long long)3 * p.Ncols * p.K * 2), 0x00020000)
         : __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w + (long long)(m0 / (p.Ho * p.Wo)) * p.w_bs), 0,
                                             (int)((long long)p.Ncols * p.K * 4), 0x00020000);
  const unsigned wplane = (unsigned)((long long)p.Ncols * p.K * 2);  // bytes per pre-split plane

  int iy0[RA], ix0[RA], bidx[RA];
  const int HoWo = p.Ho * p.Wo;
#pragma unroll
  for (int i = 0; i < RA; ++i) {
    int m = m0 + rbase + 32 * i;
    int b = m / HoWo;
    int rem = m - b * HoWo;
    int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    iy0[i] = tap_origin(p, oy);
    ix0[i] = tap_origin(p, ox);
    bidx[i] = m < p.M ? b : -1;
  }
  unsigned wvoff[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    int n = n0 + rbase + 32 * i;
    wvoff[i] = n < p.Ncols ? (unsigned)(((long long)n * p.K + kq * 4) * (PS ? 2 : 4)) : OOB;
  }
  const bool relu_in = p.flags & SWEM_CONV_RELU_IN;
  unsigned avoff[RA];
  auto set_tap = [&](const KPos &q) {
    const int cs = q.src == 0 ? p.c[0] : (q.src == 1 ? p.c[1] : p.c[2]);
    const long long bs = q.src == 0 ? p.bs[0] : (q.src == 1 ? p.bs[1] : p.bs[2]);
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      int iy, ix;
      const bool oky = tap_coord(p, iy0[i], q.ky, p.H, iy), okx = tap_coord(p, ix0[i], q.kx, p.W, ix);
      const bool ok = bidx[i] >= 0 && oky && okx;
      const long long e = bidx[i] * bs + ((long long)iy * p.W + ix) * cs + kq * 4;
      avoff[i] = ok ? (unsigned)(e * 4) : OOB;
    }
  };
  float4 ga[RA], gb[PS ? 1 : RB];
  uint2 gs[PS ? 3 : 1][RB];
  __amdgpu_buffer_rsrc_t rsa;
  auto gload = [&](const KPos &q, int kb) {
    const unsigned soff = (unsigned)q.ci0 * 4u;
#pragma unroll
    for (int i = 0; i < RA; ++i) ga[i] = bufload4(rsa, avoff[i], soff);
    if constexpr (PS) {
      const unsigned wsoff = (unsigned)kb * (BK * 2u);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int i = 0; i < RB; ++i) gs[pl][i] = bufload2(rsw, wvoff[i], wsoff + pl * wplane);
    } else {
      const unsigned wsoff = (unsigned)kb * (BK * 4u);
#pragma unroll
      for (int i = 0; i < RB; ++i) gb[i] = bufload4(rsw, wvoff[i], wsoff);
    }
  };
  // split + store: 8 bytes per plane at [plane][k8 = kq/2][row] + (kq & 1) * 8
  auto lstore = [&](int buf) {
    char *abase = reinterpret_cast<char *>(As + buf * 3 * PA) + ((kq >> 1) * SA + rbase) * 16 + (kq & 1) * 8;
    char *bbase = reinterpret_cast<char *>(Bs + buf * 3 * PB) + ((kq >> 1) * SB + rbase) * 16 + (kq & 1) * 8;
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      uint2 hh, mm, ll;
      split3(relu_in ? relu4(ga[i]) : ga[i], hh, mm, ll);
      *reinterpret_cast<uint2 *>(abase + 32 * i * 16) = hh;
      *reinterpret_cast<uint2 *>(abase + PA * 16 + 32 * i * 16) = mm;
      *reinterpret_cast<uint2 *>(abase + 2 * PA * 16 + 32 * i * 16) = ll;
    }
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      uint2 hh, mm, ll;
      if constexpr (PS) {
        hh = gs[0][i];
        mm = gs[1][i];
        ll = gs[2][i];
      } else {
        split3(gb[i], hh, mm, ll);
      }
      *reinterpret_cast<uint2 *>(bbase + 32 * i * 16) = hh;
      *reinterpret_cast<uint2 *>(bbase + PB * 16 + 32 * i * 16) = mm;
      *reinterpret_cast<uint2 *>(bbase + 2 * PB * 16 + 32 * i * 16) = ll;
    }
  };
  auto advance = [&](KPos &q) {
    q.ci0 += BK;
    const int cs = q.src == 0 ? p.c[0] : (q.src == 1 ? p.c[1] : p.c[2]);
    if (q.ci0 >= cs) {
      q.ci0 = 0;
      ++q.src;
      const int cn = q.src == 1 ? p.c[1] : (q.src == 2 ? p.c[2] : 0);
      if (cn == 0) {
        q.src = 0;
        if (++q.kx == p.KW) {
          q.kx = 0;
          ++q.ky;
        }
      }
      set_tap(q);
      rsa = src_rsrc(q.src);
    }
  };

  f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int kb_begin = blockIdx.z * p.kb_per_split;
  const int kb_end = min(p.nkb, kb_begin + p.kb_per_split);
  KPos q;
  kpos_init(q, p, kb_begin);
  set_tap(q);
  rsa = src_rsrc(q.src);
  gload(q, kb_begin);
  lstore(0);
  __syncthreads();
  int buf = 0;
  for (int kb = kb_begin; kb < kb_end; ++kb) {
    const bool more = kb + 1 < kb_end;
    if (more) advance(q);
    gload(q, more ? kb + 1 : kb);
    const uint4 *Ab = As + buf * 3 * PA + wm * 32 * WM + r;
    const uint4 *Bb = Bs + buf * 3 * PB + wn * 32 * WN + r;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {  // two 16-wide k-steps; lane half h holds k = 8h..8h+7 of the step
      const int k8 = 2 * s2 + h;
      uint4 a[3][WM], b[3][WN];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
        for (int i = 0; i < WM; ++i) a[pl][i] = Ab[pl * PA + k8 * SA + 32 * i];
#pragma unroll
        for (int i = 0; i < WN; ++i) b[pl][i] = Bb[pl * PB + k8 * SB + 32 * i];
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int jn = 0; jn < WN; ++jn) {
          f32x16 c = acc[i][jn];
          c = mfma_bf16(a[0][i], b[2][jn], c);  // small terms first
          c = mfma_bf16(a[2][i], b[0][jn], c);
          c = mfma_bf16(a[1][i], b[1][jn], c);
          c = mfma_bf16(a[0][i], b[1][jn], c);
          c = mfma_bf16(a[1][i], b[0][jn], c);
          c = mfma_bf16(a[0][i], b[0][jn], c);
          acc[i][jn] = c;
        }
    }
    lstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  conv_epilogue<WM, WN>(p, acc, m0, n0, wm, wn, r, h);
}

template <int WM, int WN>
int launch_pipe(const ConvP &p, dim3 grid, hipStream_t st) {
  constexpr size_t lds = 2 * KQ * (64 * WM + 1 + 64 * WN + 1) * sizeof(float4);
  SWEM_ALLOW_LDS((conv_igemm_pipe_kernel<WM, WN>), lds);
  hipLaunchKernelGGL((conv_igemm_pipe_kernel<WM, WN>), grid, dim3(256), lds, st, p);
  return SWEM_OK;
}

template <int WM, int WN>
int launch_bf3(const ConvP &p, dim3 grid, hipStream_t st) {
  constexpr size_t lds = 2 * 3 * 4 * (64 * WM + 1 + 64 * WN + 1) * 16;
  SWEM_ALLOW_LDS((conv_igemm_bf3_kernel<WM, WN>), lds);
  hipLaunchKernelGGL((conv_igemm_bf3_kernel<WM, WN>), grid, dim3(256), lds, st, p);
  return SWEM_OK;
}

template <int WM, int WN, bool DB>
int launch(const ConvP &p, dim3 grid, hipStream_t st) {
  constexpr size_t lds = (DB ? 2 : 1) * KQ * (64 * WM + 1 + 64 * WN + 1) * sizeof(float4);
  SWEM_ALLOW_LDS((conv_igemm_kernel<WM, WN, DB>), lds);
  hipLaunchKernelGGL((conv_igemm_kernel<WM, WN, DB>), grid, dim3(256), lds_with_planes(p, lds, 4), st, p);
  return SWEM_OK;
}

}  // namespace

int swem_conv_f32_launch(const ConvP &p, int wm, int wn, bool emulate, bool pipe_ok, bool single, dim3 grid, hipStream_t st) {
  if (emulate && wm == 2 && wn == 2) return launch_bf3<2, 2>(p, grid, st);
  if (emulate && wm == 1 && wn == 2) return launch_bf3<1, 2>(p, grid, st);
  if (emulate && wm == 1 && wn == 1) return launch_bf3<1, 1>(p, grid, st);
  if (pipe_ok && wm == 2 && wn == 2) return launch_pipe<2, 2>(p, grid, st);
  if (pipe_ok && wm == 1 && wn == 2) return launch_pipe<1, 2>(p, grid, st);
  if (pipe_ok && wm == 1 && wn == 1) return launch_pipe<1, 1>(p, grid, st);
  if (wm == 2 && wn == 2) return single ? launch<2, 2, false>(p, grid, st) : launch<2, 2, true>(p, grid, st);
  if (wm == 1 && wn == 2) return single ? launch<1, 2, false>(p, grid, st) : launch<1, 2, true>(p, grid, st);
  if (wm == 1 && wn == 1) return single ? launch<1, 1, false>(p, grid, st) : launch<1, 1, true>(p, grid, st);
  swem_set_error("conv2d: unsupported tile plan %dx%d", wm, wn);
  return SWEM_E_ARG;
}
