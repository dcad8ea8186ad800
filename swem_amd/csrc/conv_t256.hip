// conv_t256_kernel: the pre-split convolution on 256-column tiles, one block per CU (a unit of its own: its six
// instantiations compile in a minute beside the five of conv_presplit.hip).
#include <type_traits>

#include "conv_mma16.h"

namespace {

// Epilogue of conv_t256_kernel (round 6).  conv_epilogue16 inlines one copy of out_tile32 -- residual / mask / ReLU / fp32 map / two
// plane variants, all runtime flags -- per 32 x 32 sub-tile of the wave's accumulators, because the accumulators are registers and
// a register array only takes compile-time indices: with this kernel's 128 accumulator registers that was 8 (+ 4 for the GLU form)
// unrolled copies, 294 KB of code for conv_t256_kernel<true, 0>, 68 spilled registers and 72 scratch instructions in the epilogue
// of the one-block-per-CU kernel whose measured weakness IS its epilogue.  Here the accumulators leave the
// registers first: a pass stages up to four scaled sub-tiles (static register indices, ~70 instructions each) into the wave's
// slice of the idle operand LDS (18 KB per wave), and ONE out_tile32 in a loop that is not unrolled takes them out -- the LDS
// address is the only thing that depends on the loop counter.  Same values, same stores, same order per sub-tile.
constexpr int T256_EPI_SUB = 4;                                  // sub-tiles staged per pass
constexpr int T256_EPI_BYTES = T256_EPI_SUB * PL_BYTES;          // LDS bytes per wave (x 8 waves = 144 KB <= the block's 144 KB)
template <int TM2, int TN2>
__device__ __forceinline__ void t256_epilogue(const ConvP &p, f32x4v (&acc)[TM2][TN2], int mrow0, int ncol0, int lane, char *smem) {
  static_assert(TM2 % 2 == 0 && TN2 % 2 == 0, "the output staging works on 32 x 32 sub-tiles");
  const int col = lane & 15, rg = lane >> 4;
  if (p.partial) {   // (a K-split launch whose partial tiles a separate kernel reduces: raw sums, as conv_epilogue16)
    float *dst = p.partial + (long long)blockIdx.z * (p.M - p.part_m0) * p.Ncols - (long long)p.part_m0 * p.Ncols;
#pragma unroll
    for (int i = 0; i < TM2; ++i)
#pragma unroll
      for (int j = 0; j < TN2; ++j) {
        const int n = ncol0 + 16 * j + col;
        if (n >= p.Ncols) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = mrow0 + 16 * i + 4 * rg + e;
          if (m < p.M) dst[(long long)m * p.Ncols + n] = acc[i][j][e];
        }
      }
    return;
  }
  constexpr int NI = TM2 / 2, NJ = TN2 / 2;
  constexpr int SUBW = 32 * PL_STRIDE;                           // dwords per staged sub-tile
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned *lds = reinterpret_cast<unsigned *>(smem + wave * T256_EPI_BYTES);
  const bool glu = TN2 == 4 && (p.flags & SWEM_CONV_GLU);
  // per-column scale / shift of this lane's columns (GLU: tiles 0, 1 are f, tiles 2, 3 the gates of the same 32 channels)
  float sc[TN2], sh[TN2];
  const bool gin = ncol0 + 64 <= p.Ncols;
#pragma unroll
  for (int j = 0; j < TN2; ++j) {
    const int n = ncol0 + 16 * j + col;
    const bool nin = glu ? gin : n < p.Ncols;
    sc[j] = (nin && p.scale) ? p.scale[n] : p.uscale;
    sh[j] = (nin && p.shift) ? p.shift[n] : 0.f;
  }
  __syncthreads();   // every wave is done with the operand stages: the LDS is free for the output staging
  const int nsub = glu ? NI : NI * NJ;                            // sub-tile s: rows 32 (s % NI), column pair s / NI
  // The passes are spelled out (the accumulators a pass stages are dead after it: only the later passes' registers stay live
  // across the output loop); the output loop inside a pass is NOT unrolled.
  constexpr int NPASS = (NI * NJ + T256_EPI_SUB - 1) / T256_EPI_SUB;
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    const int s0 = pass * T256_EPI_SUB;
    // ---- stage sub-tiles s0 .. s0 + 3 (compile-time register indices)
#pragma unroll
    for (int kk = 0; kk < T256_EPI_SUB; ++kk) {
      const int s = s0 + kk;
      if (s >= NI * NJ || s >= nsub) continue;
      const int i0 = 2 * (s % NI), j0 = 2 * (s / NI);
      unsigned *dst = lds + kk * SUBW;
      if (glu) {
        if constexpr (TN2 == 4) {
#pragma unroll
          for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                dst[(16 * ii + 4 * rg + e) * PL_STRIDE + 16 * j + col] = __float_as_uint(
                    (acc[i0 + ii][j][e] * sc[j] + sh[j]) * sigmoidf_(acc[i0 + ii][j + 2][e] * sc[j + 2] + sh[j + 2]));
        }
      } else {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              dst[(16 * ii + 4 * rg + e) * PL_STRIDE + 16 * jj + col] =
                  __float_as_uint(acc[i0 + ii][j0 + jj][e] * sc[j0 + jj] + sh[j0 + jj]);
      }
    }
    // ---- ... and take them out: one out_tile32 per pass, the sub-tile is a runtime index
    const int cnt = min(T256_EPI_SUB, nsub - s0);      // (<= 0 for the second pass of the GLU form: NI sub-tiles in all)
#pragma nounroll
    for (int k = 0; k < cnt; ++k) {
      const int s = s0 + k;
      const int si = s % NI, sj = s / NI;
      out_tile32(p, lds + k * SUBW, mrow0 + 32 * si, glu ? (gin ? (ncol0 >> 1) : p.Cout) : ncol0 + 32 * sj);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// "t256" (round 5): the f16x3 convolution on a 256 x 256 tile, eight waves, ONE block per CU.
// conv_igemm_bf3s_kernel (conv_presplit.hip) is the "128x128 tile, one hand-over per k-block" structure, whose ceiling on this chip is ~900 TFLOP/s of
// MFMA work (cdna_hip_programming.md, "The step-3 structure's ~900 TF ceiling"; this library's f16x3 layers run at 3 x 290-370
// = 870-1100): every k-block a wave requests the next transfers, reads 12 fragments, waits, meets the block at a barrier and
// only then starts 24 MFMAs -- what hides that sequence is the CU's OTHER resident block.  The structure that gets past it keeps
// ONE block per CU busy by itself: a wave tile of 128 x 64 (4 MFMAs per fragment read instead of 2), the transfers of k-block
// kb + 1 requested a full k-block (96 MFMAs per wave, ~3k cycles per SIMD) before anything waits for them, and the fragments of
// the next quarter of the wave tile read from the LDS while the MFMAs of the current quarter run (two fragment register sets).
//   per k-block (32 k = one filter tap x 32 channels, hi + mid planes; stage = kb & 1, 64 KB per stage) eight steps over the
//   eighths (32 rows x 32 columns) of the wave tile in snake order -- consecutive eighths share their A pair or their B pair:
//     steps 0, 1: request the transfers of k-block kb + 1 into the other stage (eight 1 KB transfers per wave);
//     every step: read the ONE new fragment pair of the next step (four ds_read_b128), then the twelve MFMAs of this step
//                 on fragments read one step earlier (two A and two B register pairs, double-buffered: 64 registers);
//     step 7:     vmcnt(0) (requested six steps ago), lgkmcnt(0), ONE s_barrier -- it publishes k-block kb + 1's stage and
//                 releases this one for the transfers of kb + 2 -- read the first pairs of k-block kb + 1; MFMAs of step 7
// Same k order, same three products per (A, B) fragment pair, same epilogue (conv_epilogue16) as that kernel; the
// accumulation order over k is the same, so the results are bit-identical to it.  LDS image per operand and stage:
// [plane][k/8 group][256 rows][16 bytes] (fragment reads conflict-free as above: the group stride is a multiple of 16 slots).
// Each wave transfers ONE 64-row run (run = wave & 3, plane = wave >> 2) of every k/8 group of both operands: one pixel decode
// and one tap mask per lane.  128 accumulator + 64 fragment registers per lane, two waves per SIMD.
// Preconditions (host): fp16 pairs (SWEM_PLAN_F16), no per-batch filters, plan tile 4 x 4, no tail split / stream-K.
// TMW = 0: the layout above (wave grid 2 x 4, BM = 256).  TMW = 8, 10, 12, 14: wave grid 1 x 8 -- every wave owns ALL BM = 16 TMW
// rows x 32 columns -- so that the tile HEIGHT can be chosen per layer: with one block per CU a launch is whole rounds of 256
// tiles, and 203 tiles (2x120x216 rows / 256) leave a fifth of the chip idle where 232 tiles of 224 rows fill it (plan bits
// 20-23 = TMW / 2).  Its k-block: the B pair once, then TMW / 2 steps of one A pair (read one step ahead) x twelve MFMAs.
template <bool F16, int TMW = 0>
__global__ __launch_bounds__(512, 1) void conv_t256_kernel(ConvP p STAMP_ARG) {
  STAMP(0);
  static_assert(TMW == 0 || (TMW >= 4 && TMW <= 14 && TMW % 2 == 0), "1 x 8 layout: an even number of 16-row tiles, below 256 rows");
  // F16 = false: the bf16x6 arithmetic (three bf16 planes per operand, six products: all 24 operand bits) -- 128-row tiles only
  // (TMW = 8): (128 + 256) rows x 64 bytes x 3 planes = 72 KB per stage.
  static_assert(F16 || TMW == 8, "three planes fit the LDS with 128-row tiles only");
  constexpr int NPL = F16 ? 2 : 3, KG = 4, BM = TMW ? 16 * TMW : 256, BN = 256, NW = 8;
  constexpr int NTM = TMW ? TMW : 8, NTN = TMW ? 2 : 4;   // accumulator tiles of a wave
  constexpr int AROWS = F16 ? 256 : BM;        // rows of the A image (fp16 pairs: 256 allocated, BM of them used)
  constexpr int PAA = KG * AROWS, PA = KG * 256;   // 16-byte slots per plane of the A / B image
  constexpr unsigned OPA = NPL * PAA * 16, OPB = NPL * PA * 16;   // bytes of the A / B image of one stage
  constexpr unsigned STAGE = OPA + OPB;        // A image, then B image (fp16 pairs: 64 KB)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // wave tile: rows wr * 128 + [0, 128), columns wc * 64 + [0, 64)  (TMW: all rows, columns wave * 32 + [0, 32))
  const int wr = TMW ? 0 : wave >> 2, wc = TMW ? wave : wave & 3;
  const int r16 = lane & 15, kgl = lane >> 4;
  int tm, tn;
  tile_coords(tm, tn, p.xpn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int dj = wave & 3, dpl = wave >> 2;    // the 64-row run and the plane this wave transfers
  const bool a_run = dj * 64 < BM;             // (a tile lower than 256 rows has fewer runs; rows past BM of the last one are
                                               // the next tile's pixels: transferred, never read)

  auto src_rsrc = [&](int sidx) __attribute__((always_inline)) {
    const unsigned short *base = sidx == 0 ? p.xs[0] : (sidx == 1 ? p.xs[1] : p.xs[2]);
    const long long ps = sidx == 0 ? p.ps[0] : (sidx == 1 ? p.ps[1] : p.ps[2]);
    return raw_rsrc(base, (unsigned)(3 * ps * 2));
  };
  const i32x4 rsw = raw_rsrc(p.wsplit, (unsigned)((long long)3 * p.Ncols * p.K * 2));
  const unsigned wplane = (unsigned)((long long)p.Ncols * p.K * 2);
  const unsigned wgroup = (unsigned)p.Ncols * 16u;
  // ---- the pixel this lane transfers (A image, row dj * 64 + lane) and its valid taps; the filter it transfers (B image)
  int iy0, ix0, bidx;
  {
    const int m = m0 + dj * 64 + lane;
    const int b = fast_div(m, p.fd_howo_mul, p.fd_howo_sh);
    const int rem = m - b * (p.Ho * p.Wo);
    const int oy = fast_div(rem, p.fd_wo_mul, p.fd_wo_sh), ox = rem - oy * p.Wo;
    iy0 = tap_origin(p, oy);
    ix0 = tap_origin(p, ox);
    bidx = m < p.M ? b : -1;
  }
  unsigned bvoff;
  {
    const int n = n0 + dj * 64 + lane;
    bvoff = n < p.Ncols ? (unsigned)n * 16u : OOB;
  }
  const int dsh = (p.flags & SWEM_CONV_DGRAD) ? p.stride - 1 : 0;
  unsigned long long tmask = 0;
  {
    unsigned colv = 0;
    for (int kx = 0; kx < p.KW; ++kx) {
      int ix;
      colv |= (tap_coord(p, ix0, kx, p.W, ix) ? 1u : 0u) << kx;
    }
    for (int ky = 0; ky < p.KH; ++ky) {
      int iy;
      if (tap_coord(p, iy0, ky, p.H, iy)) tmask |= (unsigned long long)colv << (ky * p.KW);
    }
    if (bidx < 0) tmask = 0ull;
  }
  unsigned avoff = OOB, aplane = 0, agroup = 0, a_base = 0, w_base = 0;
  int pix0 = 0;
  i32x4 rsa;
  auto set_src = [&](const KPos &q) __attribute__((always_inline)) {
    const long long ps = q.src == 0 ? p.ps[0] : (q.src == 1 ? p.ps[1] : p.ps[2]);
    const int npx = q.src == 0 ? p.npx[0] : (q.src == 1 ? p.npx[1] : p.npx[2]);
    const int bsp = q.src == 0 ? p.bsp[0] : (q.src == 1 ? p.bsp[1] : p.bsp[2]);
    aplane = (unsigned)(ps * 2);
    agroup = (unsigned)npx * 16u;
    a_base = (unsigned)(q.ci0 / 8) * agroup + (F16 ? (unsigned)dpl * aplane : 0u);
    rsa = src_rsrc(q.src);
    pix0 = (bidx < 0 ? 0 : bidx) * bsp + (iy0 >> dsh) * p.W + (ix0 >> dsh);
  };
  auto set_tap = [&](const KPos &q) __attribute__((always_inline)) {
    const int t = q.ky * p.KW + q.kx;
    const int d = (q.ky >> dsh) * p.W + (q.kx >> dsh);
    const int delta = (p.flags & SWEM_CONV_DGRAD) ? -d : d;
    avoff = ((tmask >> t) & 1ull) ? (unsigned)(pix0 + delta) * 16u : OOB;
  };
  auto advance = [&](KPos &q) __attribute__((always_inline)) {
    w_base += KG * wgroup;
    if (++q.kx == p.KW) {
      q.kx = 0;
      if (++q.ky == p.KH) {
        q.ky = 0;
        q.ci0 += BK;
        a_base += 4 * agroup;
        const int cs = q.src == 0 ? p.c[0] : (q.src == 1 ? p.c[1] : p.c[2]);
        if (q.ci0 >= cs) {
          q.ci0 = 0;
          ++q.src;
          set_src(q);
        }
      }
    }
    set_tap(q);
  };
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
  // fp16 pairs: wave (dj, dpl) moves the four k/8 groups of plane dpl of its run.  Three planes: the twelve (plane, group) cells of
  // a run are shared by the two waves (dj, 0 / 1): cell index = 2 i + (wave >> 2), i < 6.
  const unsigned lds_a = lds0 + (unsigned)((F16 ? dpl * PAA : 0) + dj * 64) * 16u;
  const unsigned lds_b = lds0 + OPA + (unsigned)((F16 ? dpl * PA : 0) + dj * 64) * 16u;
  auto issue_a = [&](int stage) __attribute__((always_inline)) {
    const unsigned sa = lds_a + (unsigned)stage * STAGE;
    if (a_run) {
      if constexpr (F16) {
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) dma16(rsa, sa + (unsigned)kg * (AROWS * 16), avoff, a_base + (unsigned)kg * agroup);
      } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          const int cell = 2 * i + dpl, pl = cell >> 2, kg = cell & 3;
          dma16(rsa, sa + (unsigned)(pl * PAA + kg * AROWS) * 16u, avoff, a_base + (unsigned)kg * agroup + (unsigned)pl * aplane);
        }
      }
    }
  };
  auto issue_b = [&](int stage) __attribute__((always_inline)) {
    const unsigned sb = lds_b + (unsigned)stage * STAGE;
    if constexpr (F16) {
#pragma unroll
      for (int kg = 0; kg < KG; ++kg) dma16(rsw, sb + (unsigned)kg * (BN * 16), bvoff, w_base + (unsigned)kg * wgroup);
    } else {
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const int cell = 2 * i + dpl, pl = cell >> 2, kg = cell & 3;
        dma16(rsw, sb + (unsigned)(pl * PA + kg * BN) * 16u, bvoff, w_base + (unsigned)kg * wgroup + (unsigned)pl * wplane);
      }
    }
  };

  f32x4v acc16[NTM][NTN];
#pragma unroll
  for (int i = 0; i < NTM; ++i)
#pragma unroll
    for (int j = 0; j < NTN; ++j) acc16[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};

  const int kb_begin = blockIdx.z * p.kb_per_split;
  const int kb_end = ((int)blockIdx.z == (int)gridDim.z - 1 && p.sk_flags && p.partial) ? p.nkb : min(p.nkb, kb_begin + p.kb_per_split);
  KPos q;
  {
    const int taps = p.KH * p.KW;
    const int cb = kb_begin / taps, t = kb_begin - cb * taps;
    q.ky = t / p.KW;
    q.kx = t - q.ky * p.KW;
    q.src = 0;
    int ci = cb * BK;
    if (ci >= p.c[0]) {
      ci -= p.c[0];
      q.src = 1;
      if (ci >= p.c[1]) {
        ci -= p.c[1];
        q.src = 2;
      }
    }
    q.ci0 = ci;
    set_src(q);
  }
  w_base = (unsigned)(kb_begin * 4) * wgroup + (F16 ? (unsigned)dpl * wplane : 0u);
  set_tap(q);

  // fragment addresses: the lane's slot inside a plane of the A / B image (tile 0 of the wave, k/8 group kgl)
  const uint4 *As = reinterpret_cast<const uint4 *>(smem) + kgl * AROWS + wr * 128 + r16;
  const uint4 *Bs = reinterpret_cast<const uint4 *>(smem + OPA) + kgl * BN + (TMW ? wc * 32 : wc * 64) + r16;
  constexpr int SSL = STAGE / 16;              // slots per stage
  // eighth (AM, BN) of the wave tile: rows AM * 32 + [0, 32) (two A tiles), columns BN * 32 + [0, 32) (two B tiles)
  auto load_a = [&](int stage, int am, uint4 (&f)[NPL][2]) __attribute__((always_inline)) {
    const uint4 *a = As + stage * SSL + am * 32;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
      for (int i = 0; i < 2; ++i) f[pl][i] = a[pl * PAA + 16 * i];
  };
  auto load_b = [&](int stage, int bn, uint4 (&f)[NPL][2]) __attribute__((always_inline)) {
    const uint4 *b = Bs + stage * SSL + bn * 32;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
      for (int j = 0; j < 2; ++j) f[pl][j] = b[pl * PA + 16 * j];
  };
#define T256_MFMA(AM, BNQ, FA, FB)                                                                          \
  {                                                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
    __builtin_amdgcn_s_setprio(1);                                                                          \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)            \
        acc16[AM * 2 + i][BNQ * 2 + j] = mm16<F16>(FA[0][i], FB[1][j], acc16[AM * 2 + i][BNQ * 2 + j]);     \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)            \
        acc16[AM * 2 + i][BNQ * 2 + j] = mm16<F16>(FA[1][i], FB[0][j], acc16[AM * 2 + i][BNQ * 2 + j]);     \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)            \
        acc16[AM * 2 + i][BNQ * 2 + j] = mm16<F16>(FA[0][i], FB[0][j], acc16[AM * 2 + i][BNQ * 2 + j]);     \
    __builtin_amdgcn_s_setprio(0);                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
  }
  // One k-block = eight steps over the wave tile's eighths in snake order, so that consecutive steps share the A pair or the B
  // pair: every step reads ONE new pair (four ds_read_b128) for the next step while its twelve MFMAs run.  BX holds the B pair
  // of eighth column 0 on entry; the next k-block's first B pair lands in BY (the roles swap from k-block to k-block).
#define T256_KBLOCK(BX, BY)                                                                                 \
  {                                                                                                         \
    const bool more = kb + 1 < kb_end;                                                                      \
    if (more) {                                                                                             \
      advance(q);                                                                                           \
      issue_a(st ^ 1);                                                                                      \
    }                                                                                                       \
    load_b(st, 1, BY);                                                                                      \
    T256_MFMA(0, 0, a0, BX);                                                                                \
    if (more) issue_b(st ^ 1);                                                                              \
    load_a(st, 1, a1);                                                                                      \
    T256_MFMA(0, 1, a0, BY);                                                                                \
    load_b(st, 0, BX);                                                                                      \
    T256_MFMA(1, 1, a1, BY);                                                                                \
    load_a(st, 2, a0);                                                                                      \
    T256_MFMA(1, 0, a1, BX);                                                                                \
    load_b(st, 1, BY);                                                                                      \
    T256_MFMA(2, 0, a0, BX);                                                                                \
    load_a(st, 3, a1);                                                                                      \
    T256_MFMA(2, 1, a0, BY);                                                                                \
    load_b(st, 0, BX);                                                                                      \
    T256_MFMA(3, 1, a1, BY);                                                                                \
    /* hand-over: k-block kb + 1 has landed (requested seven steps ago), this wave's reads of stage st are done */ \
    STAMP_T0(t_vm);                                                                                         \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                        \
    STAMP_ACC(t_vm);                                                                                        \
    STAMP_T0(t_bar);                                                                                        \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                      \
    __builtin_amdgcn_s_barrier();                                                                           \
    STAMP_ACC(t_bar);                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
    if (more) {                                                                                             \
      load_a(st ^ 1, 0, a0);                                                                                \
      load_b(st ^ 1, 0, BY);                                                                                \
    }                                                                                                       \
    T256_MFMA(3, 0, a1, BX);                                                                                \
    st ^= 1;                                                                                                \
  }
  STAMP(1);
  issue_a(0);
  issue_b(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  STAMP(2);
  STAMP_ACC_DECL(t_vm);
  STAMP_ACC_DECL(t_bar);
  int st = 0;
  if constexpr (TMW == 0) {
    uint4 a0[NPL][2], a1[NPL][2], b0[NPL][2], b1[NPL][2];
    load_a(0, 0, a0);
    load_b(0, 0, b0);
    for (int kb = kb_begin; kb < kb_end; ++kb) {
      T256_KBLOCK(b0, b1);
      if (++kb >= kb_end) break;
      T256_KBLOCK(b1, b0);
    }
  } else {
    // 1 x 8 layout: fa[(c + PA_) & 1] holds the A pair of step c (rows 32 c + [0, 32)), fb[PB_] this k-block's B pair.  The
    // buffer parities are compile-time constants (registers, not scratch): the k-loop is unrolled by two k-blocks.
    constexpr int NCH = TMW / 2;
    // (A half-k-block stagger of the two waves that share a SIMD -- waves 4-7 behind one extra barrier, two meetings per k-block
    // -- measured 1-5 % SLOWER on every layer, profiles/r05_kernel_experiments.txt section 8: the ~750 cycles per k-block outside
    // the MFMAs are not an idle SIMD at the hand-over, and the stagger halves the transfers' lead.  Diff: profiles/r06_experiments/.)
    uint4 fa[2][NPL][2], fb[2][NPL][2];
    load_a(0, 0, fa[0]);
    load_b(0, 0, fb[0]);
    int kb = kb_begin;
    auto kblock = [&](auto pa_, auto pb_) __attribute__((always_inline)) {
      constexpr int PA_ = decltype(pa_)::value, PB_ = decltype(pb_)::value;
      const bool more = kb + 1 < kb_end;
      if (more) {
        advance(q);
        issue_a(st ^ 1);
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (c == 1 && more) issue_b(st ^ 1);
        if (c + 1 < NCH) {
          load_a(st, c + 1, fa[(c + 1 + PA_) & 1]);
        } else {
          // hand-over: k-block kb + 1 has landed (requested NCH - 1 steps ago), this wave's reads of stage st are done
          STAMP_T0(t_vm);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          STAMP_ACC(t_vm);
          STAMP_T0(t_bar);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          STAMP_ACC(t_bar);
          __builtin_amdgcn_sched_barrier(0);
          if (more) {
            load_a(st ^ 1, 0, fa[(NCH + PA_) & 1]);
            load_b(st ^ 1, 0, fb[PB_ ^ 1]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        // products in the order of conv_igemm_bf3s_kernel (per accumulator): fp16 pairs a0 b1, a1 b0, a0 b0; three planes
        // a0 b2, a2 b0, a1 b1, a0 b1, a1 b0, a0 b0
        constexpr int NPROD = F16 ? 3 : 6;
        constexpr int PAI[6] = {0, 2, 1, 0, 1, 0}, PBI[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
        for (int prod = 0; prod < NPROD; ++prod)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc16[2 * c + i][j] = mm16<F16>(fa[(c + PA_) & 1][PAI[prod + 6 - NPROD]][i], fb[PB_][PBI[prod + 6 - NPROD]][j],
                                              acc16[2 * c + i][j]);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
      }
      st ^= 1;
    };
    for (; kb < kb_end; ++kb) {
      kblock(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
      if (++kb >= kb_end) break;
      kblock(std::integral_constant<int, NCH & 1>{}, std::integral_constant<int, 1>{});
    }
  }
#undef T256_KBLOCK
#undef T256_MFMA
  STAMP(3);
  STAMP_ACC_OUT(6, t_vm);
  STAMP_ACC_OUT(7, t_bar);
  // ---- K-split reduced inside the launch: conv_igemm_bf3s_kernel's scheme (the last split of a tile is its reducer)
  bool fused_last = false;
  if (p.partial && p.sk_flags) {
    constexpr int NCH = NTM * NTN;   // float4 chunks per lane: the wave's accumulator tiles
    constexpr unsigned TILE_BYTES = BM * BN * 4;
    const int nsp = (int)gridDim.z, tile_lin = tm * (int)gridDim.y + tn;
    float *slots = p.partial + (long long)tile_lin * nsp * (BM * BN);
    if ((int)blockIdx.z != nsp - 1) {
      const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(slots + (long long)blockIdx.z * (BM * BN), 0, TILE_BYTES, 0x00020000);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const f32x4v t = acc16[c / NTN][c % NTN];
        u32x4 v;
        v.x = __float_as_uint(t[0]); v.y = __float_as_uint(t[1]); v.z = __float_as_uint(t[2]); v.w = __float_as_uint(t[3]);
        __builtin_amdgcn_raw_buffer_store_b128(v, rp, (unsigned)((c * 64 * NW + tid) * 16), 0, 0x11);   // sc0 sc1
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) __hip_atomic_fetch_add(p.sk_flags + tile_lin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    fused_last = true;
    if (tid == 0) {
      int spin = 0;
      unsigned seen = __hip_atomic_fetch_add(p.sk_flags + tile_lin, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      while (seen < (unsigned)(nsp - 1) && spin < p.spin_limit) {
        __builtin_amdgcn_s_sleep(8);
        ++spin;
        seen = __hip_atomic_fetch_add(p.sk_flags + tile_lin, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (seen < (unsigned)(nsp - 1) && p.fault)
        __hip_atomic_fetch_or(p.fault, (unsigned)SWEM_FAULT_KSPLIT_WAIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p.sk_flags + tile_lin, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    for (int zz = 0; zz < nsp - 1; ++zz) {
      const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(slots + (long long)zz * (BM * BN), 0, TILE_BYTES, 0x00020000);
      // (sixteen 16-byte loads in flight per lane, not all NCH: beside 128 accumulator registers more would spill; fewer would
      // make the reducer's tail a chain of load latencies)
      constexpr int RCH = 16;
#pragma unroll
      for (int c0 = 0; c0 < NCH; c0 += RCH) {
        u32x4 v[RCH];
#pragma unroll
        for (int cc = 0; cc < RCH; ++cc)
          if (c0 + cc < NCH) v[cc] = __builtin_amdgcn_raw_buffer_load_b128(rp, (unsigned)(((c0 + cc) * 64 * NW + tid) * 16), 0, 0x11);
#pragma unroll
        for (int cc = 0; cc < RCH; ++cc)
          if (c0 + cc < NCH) {
            f32x4v t = acc16[(c0 + cc) / NTN][(c0 + cc) % NTN];
            t[0] += __uint_as_float(v[cc].x); t[1] += __uint_as_float(v[cc].y); t[2] += __uint_as_float(v[cc].z); t[3] += __uint_as_float(v[cc].w);
            acc16[(c0 + cc) / NTN][(c0 + cc) % NTN] = t;
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  if (fused_last) {
    ConvP q2 = p;
    q2.partial = nullptr;
    t256_epilogue<NTM, NTN>(q2, acc16, m0 + wr * 128, n0 + (TMW ? wc * 32 : wc * 64), lane, smem);
  } else {
    t256_epilogue<NTM, NTN>(p, acc16, m0 + wr * 128, n0 + (TMW ? wc * 32 : wc * 64), lane, smem);
  }
  STAMP(4);
}

}  // namespace

int swem_conv_t256_launch(const ConvP &q, int trows, dim3 grid, hipStream_t st) {
  // two stages x (A, B) x two planes x four k/8 groups x 256 rows = 128 KB for the k-loop; the epilogue stages four 32 x 32 sub-tiles
  // per wave (t256_epilogue): 144 KB
  constexpr size_t lds = 8 * T256_EPI_BYTES;
  static_assert(lds >= 2 * 2 * 2 * 4 * 256 * 16 && lds <= 160 * 1024, "LDS of conv_t256_kernel");
  if (!q.f16) {   // bf16x6 (three planes): 128-row tiles, (128 + 256) rows x 3 planes x 4 groups x 16 bytes per stage
    constexpr size_t lds3 = 2 * 3 * 4 * (128 + 256) * 16;
    static_assert(lds3 >= 8 * T256_EPI_BYTES, "the bf16x6 form's operand stages hold the epilogue's staging too");
    SWEM_ALLOW_LDS((conv_t256_kernel<false, 8>), lds3);
    hipLaunchKernelGGL((conv_t256_kernel<false, 8>), grid, dim3(512), lds3, st, q STAMP_PASS);
    return SWEM_OK;
  }
#define T256_LAUNCH(TMW_)                                                                         \
  {                                                                                               \
    SWEM_ALLOW_LDS((conv_t256_kernel<true, TMW_>), lds);                                          \
    hipLaunchKernelGGL((conv_t256_kernel<true, TMW_>), grid, dim3(512), lds, st, q STAMP_PASS);   \
  }
  switch (trows) {
    case 128: T256_LAUNCH(8); break;
    case 160: T256_LAUNCH(10); break;
    case 192: T256_LAUNCH(12); break;
    case 224: T256_LAUNCH(14); break;
    default: T256_LAUNCH(0)
  }
#undef T256_LAUNCH
  return SWEM_OK;
}
