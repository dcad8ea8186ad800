// Implicit-GEMM convolution on the gfx950 matrix cores: the host side.  Plans, workspace sizing and the C entry points are
// here, with the split-K reducer and the operand-split kernels; the convolution kernels are in conv_f32.hip,
// conv_presplit.hip and conv_t256.hip, and conv_common.h holds the launch parameters (ConvP) they all take.
//
//   GEMM view:  Y[m][n] = sum_k A[m][k] * Wt[n][k]
//     m = output pixel (b, oy, ox)            M = B*Ho*Wo
//     n = output filter                       Ncols = Cout (2*Cout for the GLU pair)
//     k = (ky, kx, ci), ci fastest            K = KH*KW*Cin
//   A is never materialised: each thread gathers 16-byte channel groups of the NHWC input
//   (up to three concatenated sources, optional broadcast over the batch, optional input ReLU).
//
// Layers whose grid would not fill the 256 CUs split K over blockIdx.z; the partial sums go to a
// workspace and a second kernel reduces them in a fixed order (deterministic) and runs the epilogue.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "conv_common.h"

namespace {

// Reduce split-K partials in z order and apply the same epilogue.  One thread per 4 output channels.
__global__ __launch_bounds__(256) void conv_splitk_epilogue_kernel(ConvP p, int nsplit) {
  const bool glu = p.flags & SWEM_CONV_GLU;
  const int cq = p.Cout / 4;
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)(p.M - p.part_m0) * cq) return;
  const int mrel = (int)(idx / cq);
  const int m = p.part_m0 + mrel;
  const int co = (int)(idx - (long long)mrel * cq) * 4;
  const long long MN = (long long)(p.M - p.part_m0) * p.Ncols;
  auto sum4 = [&](int col) {
    const float *src = p.partial + (long long)mrel * p.Ncols + col;
    float4 s = *reinterpret_cast<const float4 *>(src);
    for (int z = 1; z < nsplit; ++z) {
      float4 t = *reinterpret_cast<const float4 *>(src + z * MN);
      s.x += t.x;
      s.y += t.y;
      s.z += t.z;
      s.w += t.w;
    }
    return s;
  };
  auto affine4 = [&](float4 s, int col) {
    float4 sc = p.scale ? *reinterpret_cast<const float4 *>(p.scale + col) : make_float4(p.uscale, p.uscale, p.uscale, p.uscale);
    float4 sh = p.shift ? *reinterpret_cast<const float4 *>(p.shift + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(s.x * sc.x + sh.x, s.y * sc.y + sh.y, s.z * sc.z + sh.z, s.w * sc.w + sh.w);
  };
  float4 v;
  if (glu) {
    const int g = co >> 5, rr = co & 31;
    float4 f = affine4(sum4(g * 64 + rr), g * 64 + rr);
    float4 a = affine4(sum4(g * 64 + 32 + rr), g * 64 + 32 + rr);
    v = make_float4(f.x * sigmoidf_(a.x), f.y * sigmoidf_(a.y), f.z * sigmoidf_(a.z), f.w * sigmoidf_(a.w));
  } else {
    v = affine4(sum4(co), co);
    if (p.res || p.res_pl) {
      const int HoWo = p.Ho * p.Wo;
      int b = m / HoWo;
      float4 rv = p.res_pl ? residual_from_planes(p, (long long)b * (p.res_bs / p.Cout) + (m - b * HoWo), co)
                           : *reinterpret_cast<const float4 *>(p.res + (long long)b * p.res_bs +
                                                               (long long)(m - b * HoWo) * p.Cout + co);
      if (p.flags & SWEM_CONV_MASK_POS) {
        v = make_float4(rv.x > 0.f ? v.x : 0.f, rv.y > 0.f ? v.y : 0.f, rv.z > 0.f ? v.z : 0.f, rv.w > 0.f ? v.w : 0.f);
      } else {
        v.x += rv.x;
        v.y += rv.y;
        v.z += rv.z;
        v.w += rv.w;
      }
    }
  }
  const unsigned nan_in = f32_nan(v);   // (before any ReLU: out_tile32)
  if (!glu && (p.flags & SWEM_CONV_RELU_OUT)) v = relu4(v);
  if (p.y) *reinterpret_cast<float4 *>(p.y + (long long)m * p.Cout + co) = v;
  if (!(p.ysp[0] || p.ysp[1])) return;
  // output planes (fused operand split): an even lane and its odd neighbour hold the 8 channels of one 16-byte run
  // (Cout / 4 is even -- Cout % 8 == 0 is the planes' precondition -- so a pair never straddles two pixels)
  unsigned bad = 0;
#pragma unroll
  for (int var = 0; var < 2; ++var) {
    if (!p.ysp[var]) continue;
    const float4 q = var ? relu4(v) : v;
    uint2 h, mm, l;
    split_as(p.ysp_npl[var], q, h, mm, l, bad);
    if (p.ysp_npl[var] == SWEM_PLANES_F16) bad |= nan_in;
    const uint2 h2 = make_uint2(__shfl_down(h.x, 1), __shfl_down(h.y, 1));
    const uint2 m2 = make_uint2(__shfl_down(mm.x, 1), __shfl_down(mm.y, 1));
    const uint2 l2 = make_uint2(__shfl_down(l.x, 1), __shfl_down(l.y, 1));
    if ((co & 4) == 0) {
      unsigned short *d = p.ysp[var] + ((long long)(co >> 3) * p.M + m) * 8;
      *reinterpret_cast<uint4 *>(d) = make_uint4(h.x, h.y, h2.x, h2.y);
      *reinterpret_cast<uint4 *>(d + p.ysp_ps) = make_uint4(mm.x, mm.y, m2.x, m2.y);
      if (p.ysp_npl[var] == 3) *reinterpret_cast<uint4 *>(d + 2 * p.ysp_ps) = make_uint4(l.x, l.y, l2.x, l2.y);
    }
  }
  range_fault(p.fault, bad);
}

struct Plan {
  int wm, wn, nsplit, kb_per_split;
};
constexpr int SWEM_KSPLIT_SKEW_DEFAULT = 0;   // percent (see the fused K-split launch)
constexpr int SK_MAX_WORKERS = 1024;   // stream-K: resident-block slots of the chip (256 CUs x at most 4 blocks)

// Tuning hook (tools/conv_bench.py): SWEM_CONV_PLAN="wm,wn,nsplit" forces one plan for every launch.
bool forced_plan(Plan &pl, int nkb, bool glu) {
  static int state = 0, fwm = 0, fwn = 0, fns = 0;
  if (state == 0) {
    const char *e = getenv("SWEM_CONV_PLAN");
    state = (e && sscanf(e, "%d,%d,%d", &fwm, &fwn, &fns) == 3) ? 1 : -1;
  }
  if (state < 0) return false;
  if (glu && fwn != 2) return false;
  int ns = fns < 1 ? 1 : (fns > nkb ? nkb : fns);
  int per = cdiv(nkb, ns);
  pl = Plan{fwm, fwn, cdiv(nkb, per), per};
  return true;
}

Plan make_plan(int M, int Ncols, int nkb, bool glu) {
  {
    Plan f;
    if (forced_plan(f, nkb, glu)) return f;
  }
  // Candidate wave tiles, largest first.  Take the largest whose grid gives every CU about two blocks
  // (the LDS image allows two resident blocks); if none does, take the smallest and split K until it does.
  static const int cand[3][2] = {{2, 2}, {1, 2}, {1, 1}};
  const long long target = 2 * 256;
  Plan best{1, glu ? 2 : 1, 1, nkb};
  for (int c = 0; c < 3; ++c) {
    const int wm = cand[c][0], wn = cand[c][1];
    if (glu && wn != 2) continue;
    if (!glu && Ncols < 64 * wn && wn > 1) continue;
    best = Plan{wm, wn, 1, nkb};
    if ((long long)cdiv(M, 64 * wm) * cdiv(Ncols, 64 * wn) >= target) return best;
  }
  const long long blocks = (long long)cdiv(M, 64 * best.wm) * cdiv(Ncols, 64 * best.wn);
  int ns = (int)((target + blocks - 1) / blocks);
  const int maxsplit = nkb / 4;  // keep at least 4 k-blocks (128 k) per split
  if (ns > maxsplit) ns = maxsplit;
  if (ns > 16) ns = 16;
  if (ns < 1) ns = 1;
  const int per = cdiv(nkb, ns);
  best.nsplit = cdiv(nkb, per);
  best.kb_per_split = per;
  return best;
}

}  // namespace

// plan hint: 0 = heuristic; else wm | wn << 4 | nsplit << 8 | math << 16 | variant << 20 (swem_hip.h)
Plan resolve_plan(int plan, int M, int Ncols, int nkb, bool glu) {
  const bool presplit_math = ((plan >> 16) & 3) != 0;   // the 128x64 tile (wm 2, wn 1) exists for the pre-split kernels only
  const bool f16x3 = ((plan >> 16) & 7) == 7;           // ... and the 256-column tiles (wm 4, wn 4: conv_t256_kernel) for f16x3,
  const bool bf16x6_128 = ((plan >> 16) & 7) == 1 && ((plan >> 20) & 15) == 4;   // or for bf16x6 with 128-row tiles (bits 20-23 = 4)
  plan &= 0xffff;
  if (plan > 0) {
    int wm = plan & 15, wn = (plan >> 4) & 15, ns = plan >> 8;
    bool ok = (wm == 1 || wm == 2) && (wn == 1 || wn == 2) && !(wm == 2 && wn == 1 && !presplit_math) && !(glu && wn != 2);
    ok = ok || (wm == 4 && wn == 4 && (f16x3 || bf16x6_128));
    if (ok) {
      ns = ns < 1 ? 1 : (ns > nkb ? nkb : ns);
      int per = cdiv(nkb, ns);
      return Plan{wm, wn, cdiv(nkb, per), per};
    }
  }
  return make_plan(M, Ncols, nkb, glu);
}

// Tail split (plan bits 24-27 = K-split factor ts of the LAST, partly filled round of tiles): a grid of T tiles on S
// resident-block slots runs ceil(T/S) rounds however few tiles the last one holds (2x120x216x256->256: 1620 tiles on 512
// slots = 3.16 -> 4 rounds).  The whole rounds are launched as they are; the M-tile rows of the remainder are launched a
// second time split ts ways over K (so they fill the chip) and reduced by the split-K epilogue over those rows only.
struct TailSplit {
  int main_mt, nsplit, kb_per_split;
};
// rows of a conv_t256_kernel tile (plan tile 4 x 4): plan bits 20-23 = TMW / 2 (the 1 x 8 wave layout, 16 TMW rows), 0 = 256
static inline int t256_rows(int plan) {
  const int v = (plan >> 20) & 15;
  return (v >= 4 && v <= 7) ? 32 * v : 256;
}
static inline int tile_rows(int plan, const Plan &pl) { return pl.wm == 4 ? t256_rows(plan) : 64 * pl.wm; }
static TailSplit tail_split(int plan, const Plan &pl, int M, int Ncols, int nkb) {
  TailSplit t{cdiv(M, 64 * pl.wm), 1, nkb};
  const int ts = (plan >> 24) & 15;
  if (ts <= 1 || pl.nsplit != 1 || nkb < 2 * ts) return t;
  const int bpc = (pl.wm == 2 && pl.wn == 2) ? 1 : 2;  // resident blocks per CU (LDS: 98 KB for the 128x128 tile, 74 KB else)
  const long long slots = (long long)swem_device_cus() * bpc;
  const int mt = cdiv(M, 64 * pl.wm), nt = cdiv(Ncols, 64 * pl.wn);
  const long long tiles = (long long)mt * nt, full = tiles / slots * slots;
  if (full == 0 || full == tiles) return t;
  t.main_mt = (int)(full / nt);
  if (t.main_mt >= mt) {
    t.main_mt = mt;
    return t;
  }
  t.kb_per_split = cdiv(nkb, ts);
  t.nsplit = cdiv(nkb, t.kb_per_split);
  return t;
}

// output size: forward floor((H + 2p - K)/s) + 1; data gradient: the forward INPUT size (H-1)*s + K - 2p + e, where
// e = rows/cols of the forward input the strided filter never reached (flag bits EH / EW)
static inline void conv_out_dims(int H, int W, int KH, int KW, int stride, int pad, int flags, int &Ho, int &Wo) {
  if (flags & SWEM_CONV_DGRAD) {
    Ho = (H - 1) * stride + KH - 2 * pad + ((flags & SWEM_CONV_DGRAD_EH) ? 1 : 0);
    Wo = (W - 1) * stride + KW - 2 * pad + ((flags & SWEM_CONV_DGRAD_EW) ? 1 : 0);
  } else {
    Ho = (H + 2 * pad - KH) / stride + 1;
    Wo = (W + 2 * pad - KW) / stride + 1;
  }
}

extern "C" size_t swem_conv2d_workspace(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                        int flags, int plan) {
  if (stride <= 0) return 0;
  int Ho, Wo;
  conv_out_dims(H, W, KH, KW, stride, pad, flags, Ho, Wo);
  long long M = (long long)B * Ho * Wo;
  int Ncols = (flags & SWEM_CONV_GLU) ? 2 * Cout : Cout;
  int nkb = cdiv((long long)KH * KW * Cin, BK);
  Plan pl = resolve_plan(plan, (int)M, Ncols, nkb, flags & SWEM_CONV_GLU);
  if (((plan >> 24) & 15) == 1)   // stream-K: a partial tile and a flag per worker (workers <= resident slots)
    return (size_t)SK_MAX_WORKERS * ((size_t)64 * pl.wm * 64 * pl.wn * sizeof(float) + sizeof(unsigned));
  if (pl.nsplit <= 1) {
    TailSplit t = tail_split(plan, pl, (int)M, Ncols, nkb);
    return t.nsplit > 1 ? (size_t)t.nsplit * (M - (long long)t.main_mt * 64 * pl.wm) * Ncols * sizeof(float) : 0;
  }
  // (the pre-split kernel keeps padded partial TILES and a counter per tile; the fp32 kernels [z][M][Ncols]: the larger)
  const size_t mt = cdiv(M, tile_rows(plan, pl)), nt = cdiv(Ncols, 64 * pl.wn), tile = (size_t)tile_rows(plan, pl) * 64 * pl.wn * sizeof(float);
  return (size_t)pl.nsplit * mt * nt * tile + mt * nt * sizeof(unsigned);
}

namespace {
struct PlaneOut {
  void *planes[2];
  int npl[2];
  unsigned *counters = nullptr;   // optional: caller-owned tile counters, ALL ZERO between calls (swem_conv2d_nhwc_bf16x3_planes_ctr)
  size_t ncounters = 0;
  const void *res_planes = nullptr;   // optional: the residual as planes (swem_conv2d_nhwc_bf16x3_planes_res)
  long long res_ps = 0, res_npx = 0;
  int res_npl = 0;
  unsigned *fault = nullptr;          // optional: the caller's sticky fault word (SWEM_FAULT_*)
};
// validate the optional output planes and put them into the launch parameters (after p.M / p.Cout are set)
int set_planes(ConvP &p, const PlaneOut *po, bool glu, const char *who) {
  p.ysp[0] = p.ysp[1] = nullptr;
  p.ysp_npl[0] = p.ysp_npl[1] = 3;
  p.ysp_ps = (long long)p.M * p.Cout;
  if (!po || (!po->planes[0] && !po->planes[1])) return SWEM_OK;
  (void)glu;   // the gated output goes through the same row-layout stores as any other
  SWEM_REQUIRE(p.Cout % 8 == 0, SWEM_E_SHAPE, "%s: output planes need Cout %% 8 == 0", who);
  for (int v = 0; v < 2; ++v) {
    SWEM_REQUIRE(!po->planes[v] || po->npl[v] == 2 || po->npl[v] == 3 || po->npl[v] == SWEM_PLANES_F16, SWEM_E_ARG,
                 "%s: 2 or 3 bf16 output planes, or SWEM_PLANES_F16 (an fp16 pair)", who);
    p.ysp[v] = static_cast<unsigned short *>(po->planes[v]);
    p.ysp_npl[v] = po->npl[v];
  }
  return SWEM_OK;
}
// The launch parameters both operand formats fill alike: geometry, epilogue operands, and the defaults of one plain launch.
// Everything else is zero (value-initialised: a field added later cannot reach a kernel uninitialised); the caller adds its
// sources and filters.  Wants stride > 0; the caller checks Ho, Wo and M before it uses them.
ConvP conv_params(int c0, long long bs0, int c1, long long bs1, int c2, long long bs2, int B, int H, int W, long long w_bs,
                  const float *scale, float uscale, const float *shift, const float *res, long long res_bs, float *y, int Cout,
                  int KH, int KW, int stride, int pad, int flags) {
  ConvP p{};
  p.c[0] = c0; p.c[1] = c1; p.c[2] = c2;
  p.bs[0] = bs0; p.bs[1] = bs1; p.bs[2] = bs2;
  p.B = B; p.H = H; p.W = W;
  conv_out_dims(H, W, KH, KW, stride, pad, flags, p.Ho, p.Wo);
  const long long HoWo = (long long)p.Ho * p.Wo;
  p.Cin = c0 + c1 + c2;
  p.K = KH * KW * p.Cin;
  p.M = (int)(B * HoWo);
  p.scale = scale; p.uscale = uscale; p.shift = shift; p.res = res; p.res_bs = res_bs; p.w_bs = w_bs; p.y = y;
  p.Cout = Cout; p.Ncols = (flags & SWEM_CONV_GLU) ? 2 * Cout : Cout;
  p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad; p.flags = flags;
  p.nkb = cdiv(p.K, BK);
  fast_div_make((unsigned)HoWo, p.fd_howo_mul, p.fd_howo_sh);
  fast_div_make((unsigned)p.Wo, p.fd_wo_mul, p.fd_wo_sh);
  p.nplanes = 3; p.xpn = 1;
  p.spin_limit = 1 << 24;
  return p;
}
int conv2d_f32_impl(void *stream, const float *x0, int c0, long long bs0, const float *x1, int c1, long long bs1,
                    const float *x2, int c2, long long bs2, int B, int H, int W,
                    const float *w, long long w_bs, const float *scale, const float *shift, const float *res,
                    long long res_bs, float *y, int Cout, int KH, int KW, int stride, int pad, int flags, int plan, void *ws,
                    size_t ws_bytes, const PlaneOut *po) {
  SWEM_REQUIRE(x0 && w && (y || (po && (po->planes[0] || po->planes[1]))), SWEM_E_ARG,
               "conv2d: null pointer (y may be NULL only when output planes are given)");
  if (!x1) c1 = 0;
  if (!x2) c2 = 0;
  SWEM_REQUIRE(!(x2 && !x1), SWEM_E_ARG, "conv2d: source 2 without source 1");
  SWEM_REQUIRE(c0 > 0 && c0 % 4 == 0 && c1 % 4 == 0 && c2 % 4 == 0, SWEM_E_SHAPE,
               "conv2d: every source needs a channel count that is a multiple of 4 (got %d,%d,%d)", c0, c1, c2);
  SWEM_REQUIRE(B > 0 && H > 0 && W > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0, SWEM_E_SHAPE,
               "conv2d: bad geometry");
  SWEM_REQUIRE(Cout > 0 && Cout % 4 == 0, SWEM_E_SHAPE, "conv2d: Cout must be a multiple of 4 (got %d)", Cout);
  const bool glu = flags & SWEM_CONV_GLU;
  SWEM_REQUIRE(!glu || (Cout % 32 == 0 && !res), SWEM_E_SHAPE, "conv2d: GLU needs Cout %% 32 == 0 and no residual");
  ConvP p = conv_params(c0, bs0, c1, bs1, c2, bs2, B, H, W, w_bs, scale, 1.f, shift, res, res_bs, y, Cout, KH, KW, stride, pad, flags);
  p.x[0] = x0; p.x[1] = x1 ? x1 : x0; p.x[2] = x2 ? x2 : x0;
  p.w = w;
  SWEM_REQUIRE(p.Ho > 0 && p.Wo > 0, SWEM_E_SHAPE, "conv2d: empty output");
  SWEM_REQUIRE(!(flags & SWEM_CONV_DGRAD) || ((stride == 1 || stride == 2) && c0 % 32 == 0 && c1 % 32 == 0 && c2 % 32 == 0),
               SWEM_E_SHAPE, "conv2d: the data-gradient mode needs stride 1 or 2 and sources that are multiples of 32 channels");
  SWEM_REQUIRE(!(flags & SWEM_CONV_MASK_POS) || res, SWEM_E_ARG, "conv2d: SWEM_CONV_MASK_POS needs the mask in res");
  const long long M = (long long)B * p.Ho * p.Wo;
  SWEM_REQUIRE(M < (1ll << 31) && M * (glu ? 2 * Cout : Cout) < (1ll << 40), SWEM_E_SHAPE, "conv2d: too large");
  Plan pl = resolve_plan(plan, p.M, p.Ncols, p.nkb, glu);
  if (pl.wm == 4) pl = make_plan(p.M, p.Ncols, p.nkb, glu);   // (the 256-column tiles belong to the pre-split kernel: heuristic tile here)
  if (pl.wm == 2 && pl.wn == 1) pl.wm = 1;   // (a 128x64 plan on inputs that are not pre-split: the kernels here have no such tile)
  p.kb_per_split = pl.kb_per_split;
  if (int prc = set_planes(p, po, glu, "conv2d")) return prc;
  p.fault = po ? po->fault : nullptr;
  if (pl.nsplit > 1) {
    size_t need = (size_t)pl.nsplit * M * p.Ncols * sizeof(float);
    SWEM_REQUIRE(ws && ws_bytes >= need, SWEM_E_WORKSPACE, "conv2d: workspace %zu < %zu bytes", ws_bytes, need);
    p.partial = static_cast<float *>(ws);
  }
  SWEM_REQUIRE(w_bs == 0 || (p.Ho * p.Wo) % (64 * pl.wm) == 0, SWEM_E_SHAPE,
               "conv2d: per-batch filters need Ho*Wo (%d) to be a multiple of the %d-row tile", p.Ho * p.Wo, 64 * pl.wm);
  hipStream_t st = static_cast<hipStream_t>(stream);
  dim3 grid(cdiv(p.M, 64 * pl.wm), cdiv(p.Ncols, 64 * pl.wn), pl.nsplit);
  static int single = -1;
  if (single < 0) {
    const char *e = getenv("SWEM_CONV_SINGLE");
    single = e ? atoi(e) : 0;
  }
  static int nopipe = -1;
  if (nopipe < 0) {
    const char *e = getenv("SWEM_CONV_NOPIPE");
    nopipe = e ? atoi(e) : 0;
  }
  const bool pipe_ok = !nopipe && c0 % 32 == 0 && c1 % 32 == 0 && c2 % 32 == 0;
  static int math_env = -1;
  if (math_env < 0) {
    const char *e = getenv("SWEM_CONV_MATH");  // tuning/debug override: "bf16x6" or "f32"
    math_env = !e ? 0 : (strcmp(e, "bf16x6") == 0 ? 1 : 2);
  }
  const bool emulate = pipe_ok && (math_env == 1 || (math_env == 0 && ((plan >> 16) & 1)));
  if (int rc = swem_conv_f32_launch(p, pl.wm, pl.wn, emulate, pipe_ok, single != 0, grid, st)) return rc;
  SWEM_CHECK_LAUNCH("conv_igemm_kernel");
  if (pl.nsplit > 1) {
    long long work = M * (Cout / 4);
    hipLaunchKernelGGL(conv_splitk_epilogue_kernel, dim3(cdiv(work, 256)), dim3(256), 0, st, p, pl.nsplit);
    SWEM_CHECK_LAUNCH("conv_splitk_epilogue_kernel");
  }
  return SWEM_OK;
}
}  // namespace

extern "C" int swem_conv2d_nhwc_f32(void *stream, const float *x0, int c0, long long bs0, const float *x1, int c1,
                                    long long bs1, const float *x2, int c2, long long bs2, int B, int H, int W,
                                    const float *w, long long w_bs, const float *scale, const float *shift,
                                    const float *res, long long res_bs, float *y, int Cout, int KH, int KW, int stride,
                                    int pad, int flags, int plan, void *ws, size_t ws_bytes) {
  return conv2d_f32_impl(stream, x0, c0, bs0, x1, c1, bs1, x2, c2, bs2, B, H, W, w, w_bs, scale, shift, res, res_bs, y, Cout,
                         KH, KW, stride, pad, flags, plan, ws, ws_bytes, nullptr);
}

extern "C" int swem_conv2d_nhwc_f32_planes(void *stream, const float *x0, int c0, long long bs0, const float *x1, int c1,
                                           long long bs1, const float *x2, int c2, long long bs2, int B, int H, int W,
                                           const float *w, long long w_bs, const float *scale, const float *shift,
                                           const float *res, long long res_bs, float *y, int Cout, int KH, int KW,
                                           int stride, int pad, int flags, int plan, void *ws, size_t ws_bytes,
                                           void *planes, int nplanes, void *planes_relu, int nplanes_relu, void *fault) {
  PlaneOut po{{planes, planes_relu}, {nplanes, nplanes_relu}};
  po.fault = static_cast<unsigned *>(fault);
  return conv2d_f32_impl(stream, x0, c0, bs0, x1, c1, bs1, x2, c2, bs2, B, H, W, w, w_bs, scale, shift, res, res_bs, y, Cout,
                         KH, KW, stride, pad, flags, plan, ws, ws_bytes, &po);
}

// ---------------------------------------------------------------------------------------------------------------
namespace {
// x [npix][C] fp32 -> three bf16 planes [C/8][npix][8] with x = hi + mid + lo (optionally of relu(x)).
// Block = 32 pixels x 8 channel groups; thread (pixel p, group g) = (tid / 8, tid % 8): the 8 threads of a pixel read 256
// contiguous bytes of its row (full cache lines; with the pixel on the fast thread index every thread read 32 bytes of
// its own line), and per channel group 8 consecutive pixels store one 128-byte run of every plane.
__global__ __launch_bounds__(256) void split_bf16x3_kernel(const float *__restrict__ x, unsigned short *__restrict__ out,
                                                           long long npix, int C, int relu) {
  const long long pix = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int cg = blockIdx.y * 8 + (threadIdx.x & 7);
  if (pix >= npix || cg >= C / 8) return;
  const float *src = x + pix * C + cg * 8;
  float4 v0 = *reinterpret_cast<const float4 *>(src), v1 = *reinterpret_cast<const float4 *>(src + 4);
  if (relu) {
    v0 = relu4(v0);
    v1 = relu4(v1);
  }
  uint2 h0, m0, l0, h1, m1, l1;
  split3(v0, h0, m0, l0);
  split3(v1, h1, m1, l1);
  const long long plane = npix * C, i = (long long)cg * npix + pix;
  *reinterpret_cast<uint4 *>(out + i * 8) = make_uint4(h0.x, h0.y, h1.x, h1.y);
  *reinterpret_cast<uint4 *>(out + plane + i * 8) = make_uint4(m0.x, m0.y, m1.x, m1.y);
  *reinterpret_cast<uint4 *>(out + 2 * plane + i * 8) = make_uint4(l0.x, l0.y, l1.x, l1.y);
}
}  // namespace

namespace {
// ... -> two fp16 planes [C/8][npix][8] with x = hi + mid (bf16_split.h, split2h): the operand format of the f16x3 arithmetic
__global__ __launch_bounds__(256) void split_f16x2_kernel(const float *__restrict__ x, unsigned short *__restrict__ out,
                                                          long long npix, int C, int relu, unsigned *fault) {
  const long long pix = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int cg = blockIdx.y * 8 + (threadIdx.x & 7);
  if (pix >= npix || cg >= C / 8) return;
  const float *src = x + pix * C + cg * 8;
  float4 v0 = *reinterpret_cast<const float4 *>(src), v1 = *reinterpret_cast<const float4 *>(src + 4);
  // (a NaN in the map is a fault whatever follows: relu1 would turn it into a clean 0 before the range test sees it)
  const unsigned nan_in = relu ? (f32_nan(v0) | f32_nan(v1)) : 0u;
  if (relu) {
    v0 = relu4(v0);
    v1 = relu4(v1);
  }
  uint2 h0, m0, h1, m1;
  split2h(v0, h0, m0);
  split2h(v1, h1, m1);
  const long long plane = npix * C, i = (long long)cg * npix + pix;
  *reinterpret_cast<uint4 *>(out + i * 8) = make_uint4(h0.x, h0.y, h1.x, h1.y);
  *reinterpret_cast<uint4 *>(out + plane + i * 8) = make_uint4(m0.x, m0.y, m1.x, m1.y);
  range_fault(fault, f16_oor(v0) | f16_oor(v1) | nan_in);   // (behind the input ReLU: a large NEGATIVE value under a ReLU is a plain 0)
}
}  // namespace

extern "C" int swem_split_f16x2_f32(void *stream, const float *x, void *out, long long npix, int C, int relu, void *fault) {
  SWEM_REQUIRE(x && out && npix > 0 && C > 0 && C % 8 == 0, SWEM_E_ARG, "split_f16x2: need C %% 8 == 0");
  hipLaunchKernelGGL(split_f16x2_kernel, dim3((unsigned)cdiv(npix, 32), (unsigned)cdiv(C / 8, 8)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, static_cast<unsigned short *>(out), npix, C, relu,
                     static_cast<unsigned *>(fault));
  SWEM_CHECK_LAUNCH("split_f16x2");
  return SWEM_OK;
}

extern "C" int swem_split_bf16x3_f32(void *stream, const float *x, void *out, long long npix, int C, int relu) {
  SWEM_REQUIRE(x && out && npix > 0 && C > 0 && C % 8 == 0, SWEM_E_ARG, "split_bf16x3: need C %% 8 == 0");
  hipLaunchKernelGGL(split_bf16x3_kernel, dim3((unsigned)cdiv(npix, 32), (unsigned)cdiv(C / 8, 8)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, static_cast<unsigned short *>(out), npix, C, relu);
  SWEM_CHECK_LAUNCH("split_bf16x3");
  return SWEM_OK;
}

namespace {
int conv2d_bf16x3_impl(void *stream, const void *x0, int c0, long long bs0, long long ps0, const void *x1, int c1,
                       long long bs1, long long ps1, const void *x2, int c2, long long bs2, long long ps2, int B, int H, int W,
                       const void *w_bf16x3, const float *scale, const float *shift, const float *res, long long res_bs,
                       float *y, int Cout, int KH, int KW, int stride, int pad, int flags, int plan, void *ws, size_t ws_bytes,
                       const PlaneOut *po, long long w_bs = 0, float uscale = 1.f) {
  SWEM_REQUIRE(x0 && w_bf16x3 && (y || (po && (po->planes[0] || po->planes[1]))), SWEM_E_ARG,
               "conv2d_bf16x3: null pointer (y may be NULL only when output planes are given)");
  if (!x1) c1 = 0;
  if (!x2) c2 = 0;
  SWEM_REQUIRE(!(x2 && !x1), SWEM_E_ARG, "conv2d_bf16x3: source 2 without source 1");
  SWEM_REQUIRE(c0 > 0 && c0 % 32 == 0 && c1 % 32 == 0 && c2 % 32 == 0, SWEM_E_SHAPE,
               "conv2d_bf16x3: every source needs a channel count that is a multiple of 32 (got %d,%d,%d)", c0, c1, c2);
  SWEM_REQUIRE(B > 0 && H > 0 && W > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0, SWEM_E_SHAPE,
               "conv2d_bf16x3: bad geometry");
  SWEM_REQUIRE(Cout > 0 && Cout % 4 == 0 && !(flags & SWEM_CONV_RELU_IN), SWEM_E_SHAPE,
               "conv2d_bf16x3: Cout %% 4 != 0, or RELU_IN (apply the ReLU when splitting the input)");
  const bool glu = flags & SWEM_CONV_GLU;
  SWEM_REQUIRE(!glu || (Cout % 32 == 0 && !res), SWEM_E_SHAPE, "conv2d_bf16x3: GLU needs Cout %% 32 == 0, no residual");
  ConvP p = conv_params(c0, bs0, c1, bs1, c2, bs2, B, H, W, w_bs, scale, uscale, shift, res, res_bs, y, Cout, KH, KW, stride, pad, flags);
  p.wsplit = static_cast<const unsigned short *>(w_bf16x3);
  p.xs[0] = static_cast<const unsigned short *>(x0);
  p.xs[1] = static_cast<const unsigned short *>(x1 ? x1 : x0);
  p.xs[2] = static_cast<const unsigned short *>(x2 ? x2 : x0);
  p.ps[0] = ps0; p.ps[1] = x1 ? ps1 : ps0; p.ps[2] = x2 ? ps2 : ps0;
  for (int i = 0; i < 3; ++i) {
    p.bsp[i] = p.c[i] > 0 ? (int)(p.bs[i] / p.c[i]) : 0;
    p.npx[i] = p.c[i] > 0 ? (int)(p.ps[i] / p.c[i]) : 0;
  }
  SWEM_REQUIRE(ps0 * 6 < (1ll << 31) && p.ps[1] * 6 < (1ll << 31) && p.ps[2] * 6 < (1ll << 31), SWEM_E_SHAPE,
               "conv2d_bf16x3: a source exceeds the 2 GiB buffer-descriptor range");
  SWEM_REQUIRE(p.Ho > 0 && p.Wo > 0, SWEM_E_SHAPE, "conv2d_bf16x3: empty output");
  SWEM_REQUIRE(!(flags & SWEM_CONV_DGRAD) || stride == 1 || stride == 2, SWEM_E_SHAPE,
               "conv2d_bf16x3: the data-gradient mode needs stride 1 or 2");
  const long long M = (long long)B * p.Ho * p.Wo;
  SWEM_REQUIRE(M < (1ll << 31), SWEM_E_SHAPE, "conv2d_bf16x3: too large");
  Plan pl = resolve_plan(plan, p.M, p.Ncols, p.nkb, glu);
  SWEM_REQUIRE(w_bs == 0 || (p.Ho * p.Wo) % 128 == 0, SWEM_E_SHAPE,
               "conv2d_bf16x3: per-batch filters need Ho*Wo (%d) to be a multiple of the 128-row tile", p.Ho * p.Wo);
  p.kb_per_split = pl.kb_per_split;
  if (int prc = set_planes(p, po, glu, "conv2d_bf16x3")) return prc;
  // caller-owned counters: tile counters / stream-K flags (all zero between calls); the sticky fault word is the caller's too
  if (po && po->res_planes) {
    SWEM_REQUIRE(!res && !glu && !(flags & SWEM_CONV_MASK_POS) && Cout % 8 == 0, SWEM_E_ARG,
                 "conv2d_bf16x3: a plane residual replaces `res` (no GLU, no mask; Cout %% 8 == 0)");
    SWEM_REQUIRE(po->res_npl == SWEM_PLANES_F16 || po->res_npl == 3, SWEM_E_ARG,
                 "conv2d_bf16x3: a plane residual is an fp16 pair or three bf16 planes (two bf16 planes carry 16 bits only)");
    SWEM_REQUIRE(po->res_npx > 0 && po->res_ps >= po->res_npx * (long long)Cout && res_bs % Cout == 0, SWEM_E_ARG,
                 "conv2d_bf16x3: plane residual geometry");
    p.res_pl = static_cast<const unsigned short *>(po->res_planes);
    p.res_ps = po->res_ps; p.res_npx = (int)po->res_npx; p.res_npl = po->res_npl;
  }
  const size_t nctr = (po && po->counters) ? po->ncounters : 0;
  p.fault = po ? po->fault : nullptr;
  {
    static int limit = -1;   // (tests shorten the wait to see the fault path: tests/test_gpu_ops.py)
    if (limit < 0) {
      const char *e = getenv("SWEM_SPIN_LIMIT");
      limit = e ? atoi(e) : (1 << 24);
      if (limit < 0) limit = 0;
    }
    p.spin_limit = limit;
  }
  if (pl.nsplit > 1) {
    size_t need = (size_t)pl.nsplit * M * p.Ncols * sizeof(float);
    SWEM_REQUIRE(ws && ws_bytes >= need, SWEM_E_WORKSPACE, "conv2d_bf16x3: workspace %zu < %zu bytes", ws_bytes, need);
    p.partial = static_cast<float *>(ws);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  SWEM_REQUIRE(KH * KW <= 64, SWEM_E_SHAPE, "conv2d_bf16x3: at most 64 filter taps (one validity bit per tap and pixel)");
  const int variant = (plan >> 20) & 15;
  // math 2 = plain bf16 (mixed-precision training), 3 = "bf16x3" (hi + mid planes, three products: 16 significant bits per
  // operand, ~2^-16 relative error per product), else bf16x6
  p.nplanes = ((plan >> 16) & 3) == 2 ? 1 : (((plan >> 16) & 3) == 3 ? 2 : 3);
  // plan bit 18 (SWEM_PLAN_F16) with math 3: "f16x3" -- the planes of every source and of the filters are fp16 pairs
  // (swem_split_f16x2_f32; the filters scaled per output column by a power of two that the caller folds into `scale`)
  p.f16 = (p.nplanes == 2 && ((plan >> 18) & 1)) ? 1 : 0;
  SWEM_REQUIRE(!((plan >> 18) & 1) || p.nplanes == 2, SWEM_E_ARG, "conv2d_bf16x3: plan bit 18 (fp16 planes) needs math mode 3");
  SWEM_REQUIRE(pl.wm != 4 || ((p.f16 || (p.nplanes == 3 && variant == 4 && !glu)) && w_bs == 0 && ((plan >> 24) & 15) == 0), SWEM_E_ARG,
               "conv2d_bf16x3: the 256-column tiles run f16x3 plans (or bf16x6 with 128-row tiles, no GLU) without per-batch filters, tail split or stream-K");
  const int trows = tile_rows(plan, pl);
  SWEM_REQUIRE(pl.wm != 4 || (trows == 256 && variant == 0) || (trows >= 128 && trows < 256 && trows % 32 == 0 && !glu), SWEM_E_ARG,
               "conv2d_bf16x3: 256-column tile heights are 128, 160, 192, 224 (plan bits 20-23 = rows / 32; no GLU) or 256 (bits 0)");
  const int mtiles = cdiv(p.M, trows), ntiles = cdiv(p.Ncols, 64 * pl.wn);
  // XCD partition of the N tiles: plan bits 28-29 force 2 / 4 / 8 groups; 0 = the cut with the least fetch traffic by
  // the model  groups * activations + (8 / groups) * filters  (each XCD reads its groups' filters and its share of the
  // M tiles' activations once: measured 533 -> 166 MB on 2x30x54x1280 -> 512 together with the channel-block K order)
  p.xpn = 1 << ((plan >> 28) & 3);
  if (((plan >> 28) & 3) == 0) {
    static int forced = -1;
    if (forced < 0) {
      const char *e = getenv("SWEM_CONV_XPN");
      forced = e ? atoi(e) : 0;
    }
    if (forced > 0) {
      p.xpn = forced;
    } else {
      const double abytes = (double)B * H * W * p.Cin, wbytes = (double)p.Ncols * p.K;
      double best = abytes + 8.0 * wbytes;
      for (int pn = 2; pn <= 8; pn *= 2) {
        if (ntiles % pn) continue;
        const double cost = pn * abytes + (8.0 / pn) * wbytes;
        if (cost < 0.9 * best) {
          best = cost;
          p.xpn = pn;
        }
      }
    }
  }
  if (p.xpn != 1 && p.xpn != 2 && p.xpn != 4 && p.xpn != 8) p.xpn = 1;
  if (ntiles % p.xpn) p.xpn = 1;
  auto run = [&](const ConvP &q, dim3 grid, int *occ = nullptr) -> int {
    if (pl.wm == 4) {   // the 256 x 256 tile: its own kernel (f16x3 only), one block per CU
      if (occ) {
        *occ = 1;
        return SWEM_OK;
      }
      return swem_conv_t256_launch(q, trows, grid, st);
    }
    return swem_conv_presplit_launch(q, pl.wm, pl.wn, variant, grid, st, occ);
  };
  int rc;
  if (((plan >> 24) & 15) == 1 && w_bs == 0) {
    // stream-K (see the kernel): persistent workers, one per resident-block slot, equal shares of the tiles x k-blocks
    int nb = 1;
    p.sk_workers = -1;                           // (query the stream-K instantiation)
    if ((rc = run(p, dim3(1, 1, 1), &nb))) return rc;
    p.sk_workers = 0;
    const long long iters = (long long)mtiles * ntiles * p.nkb;
    long long W = (long long)nb * swem_device_cus();
    if (W > iters / 4) W = iters / 4;            // at least four k-blocks per worker
    if (W > SK_MAX_WORKERS) W = SK_MAX_WORKERS;
    if (W >= 2) {
      const size_t tile = (size_t)64 * pl.wm * 64 * pl.wn * sizeof(float);
      const size_t need = (size_t)W * tile + (size_t)W * sizeof(unsigned);
      SWEM_REQUIRE(ws && ws_bytes >= need, SWEM_E_WORKSPACE, "conv2d_bf16x3: workspace %zu < %zu bytes (stream-K)", ws_bytes, need);
      p.kb_per_split = p.nkb;
      p.partial = nullptr;
      p.sk_workers = (int)W; p.sk_mtiles = mtiles; p.sk_ntiles = ntiles;
      p.sk_ws = static_cast<float *>(ws);
      if (nctr >= (size_t)W) {
        p.sk_flags = po->counters;     // zero on entry, reset by the workers that consume them: no memset launch
      } else {
        p.sk_flags = reinterpret_cast<unsigned *>(static_cast<char *>(ws) + (size_t)W * tile);
        if (hipMemsetAsync(p.sk_flags, 0, (size_t)W * sizeof(unsigned), st) != hipSuccess) {
          swem_set_error("conv2d_bf16x3: hipMemsetAsync of the stream-K flags failed");
          return SWEM_E_HIP;
        }
      }
      static int dbg = -1;
      if (dbg < 0) dbg = getenv("SWEM_SK_DEBUG") ? 1 : 0;
      if (dbg) fprintf(stderr, "stream-K: %d x %d tiles x %d k-blocks on %lld workers (%d blocks per CU)\n", mtiles, ntiles, p.nkb, W, nb);
      if ((rc = run(p, dim3((unsigned)W, 1, 1)))) return rc;
      SWEM_CHECK_LAUNCH("conv_igemm_bf3s_kernel");
      return SWEM_OK;
    }
  }
  const TailSplit tl = tail_split(plan, pl, p.M, p.Ncols, p.nkb);
  if (tl.nsplit > 1) {
    if ((rc = run(p, dim3(tl.main_mt, ntiles, 1)))) return rc;      // the whole rounds
    ConvP t = p;                                                    // the last round's tile rows, split over K
    t.mt0 = tl.main_mt;
    t.part_m0 = tl.main_mt * 64 * pl.wm;
    t.kb_per_split = tl.kb_per_split;
    const size_t need = (size_t)tl.nsplit * (M - t.part_m0) * p.Ncols * sizeof(float);
    SWEM_REQUIRE(ws && ws_bytes >= need, SWEM_E_WORKSPACE, "conv2d_bf16x3: workspace %zu < %zu bytes", ws_bytes, need);
    t.partial = static_cast<float *>(ws);
    if ((rc = run(t, dim3(mtiles - tl.main_mt, ntiles, tl.nsplit)))) return rc;
    SWEM_CHECK_LAUNCH("conv_igemm_bf3s_kernel");
    const long long work = (M - t.part_m0) * (Cout / 4);
    hipLaunchKernelGGL(conv_splitk_epilogue_kernel, dim3(cdiv(work, 256)), dim3(256), 0, st, t, tl.nsplit);
    SWEM_CHECK_LAUNCH("conv_splitk_epilogue_kernel");
    return SWEM_OK;
  }
  if (pl.nsplit > 1) {
    // K-split reduced by the last split (z = nsplit - 1) of every tile (see the kernel): partial TILES (padded), one counter per tile
    const size_t tile = (size_t)trows * 64 * pl.wn * sizeof(float);
    const size_t ntile = (size_t)mtiles * ntiles;
    const size_t need = (size_t)pl.nsplit * ntile * tile + ntile * sizeof(unsigned);
    SWEM_REQUIRE(ws && ws_bytes >= need, SWEM_E_WORKSPACE, "conv2d_bf16x3: workspace %zu < %zu bytes (fused K-split)", ws_bytes, need);
    p.partial = static_cast<float *>(ws);
    if (nctr >= ntile) {
      p.sk_flags = po->counters;       // zero on entry; the reducing split of a tile resets its counter: no memset launch
    } else {
      p.sk_flags = reinterpret_cast<unsigned *>(static_cast<char *>(ws) + (size_t)pl.nsplit * ntile * tile);
      if (hipMemsetAsync(p.sk_flags, 0, ntile * sizeof(unsigned), st) != hipSuccess) {
        swem_set_error("conv2d_bf16x3: hipMemsetAsync of the K-split counters failed");
        return SWEM_E_HIP;
      }
    }
    {
      // Staggered shares (round 4): equal shares make all splits of a tile finish together -- the producers' stores and the
      // reducer's loads are then a burst nothing hides (13 of 54 us on 2x30x54 k3 512->512 at nsp = 4, HISTORY.md).  The
      // producers get `skew` percent less than an equal share each, the reducer the rest: their tiles land while it still
      // multiplies.  SWEM_KSPLIT_SKEW overrides the default (0 = equal shares).
      static int skew = -1;
      if (skew < 0) {
        const char *e = getenv("SWEM_KSPLIT_SKEW");
        skew = e ? atoi(e) : SWEM_KSPLIT_SKEW_DEFAULT;
        if (skew < 0 || skew > 50) skew = 0;
      }
      int per = (int)((long long)p.nkb * (100 - skew) / (100LL * pl.nsplit));
      if (per < 1) per = 1;
      if ((long long)per * (pl.nsplit - 1) >= p.nkb) per = pl.kb_per_split;   // (too few k-blocks to skew)
      if (skew > 0 && per <= pl.kb_per_split) p.kb_per_split = per;
    }
    if ((rc = run(p, dim3(mtiles, ntiles, pl.nsplit)))) return rc;
    SWEM_CHECK_LAUNCH("conv_igemm_bf3s_kernel");
    return SWEM_OK;
  }
  if ((rc = run(p, dim3(mtiles, ntiles, pl.nsplit)))) return rc;   // (nsplit == 1: every K split has returned above)
  SWEM_CHECK_LAUNCH("conv_igemm_bf3s_kernel");
  return SWEM_OK;
}
}  // namespace

extern "C" int swem_conv2d_nhwc_bf16x3(void *stream, const void *x0, int c0, long long bs0, long long ps0,
                                       const void *x1, int c1, long long bs1, long long ps1, const void *x2, int c2,
                                       long long bs2, long long ps2, int B, int H, int W, const void *w_bf16x3,
                                       const float *scale, const float *shift, const float *res, long long res_bs,
                                       float *y, int Cout, int KH, int KW, int stride, int pad, int flags, int plan,
                                       void *ws, size_t ws_bytes) {
  return conv2d_bf16x3_impl(stream, x0, c0, bs0, ps0, x1, c1, bs1, ps1, x2, c2, bs2, ps2, B, H, W, w_bf16x3, scale, shift, res,
                            res_bs, y, Cout, KH, KW, stride, pad, flags, plan, ws, ws_bytes, nullptr);
}
extern "C" int swem_conv2d_nhwc_bf16x3_planes(void *stream, const void *x0, int c0, long long bs0, long long ps0,
                                              const void *x1, int c1, long long bs1, long long ps1, const void *x2, int c2,
                                              long long bs2, long long ps2, int B, int H, int W, const void *w_bf16x3,
                                              const float *scale, const float *shift, const float *res, long long res_bs,
                                              float *y, int Cout, int KH, int KW, int stride, int pad, int flags, int plan,
                                              void *ws, size_t ws_bytes, void *planes, int nplanes, void *planes_relu,
                                              int nplanes_relu) {
  PlaneOut po{{planes, planes_relu}, {nplanes, nplanes_relu}};
  return conv2d_bf16x3_impl(stream, x0, c0, bs0, ps0, x1, c1, bs1, ps1, x2, c2, bs2, ps2, B, H, W, w_bf16x3, scale, shift, res,
                            res_bs, y, Cout, KH, KW, stride, pad, flags, plan, ws, ws_bytes, &po);
}
// ... with caller-owned tile counters: `counters` (ncounters words) must be ALL ZERO when the call is enqueued and must not be
// used by another stream at the same time; the kernels leave it all zero again.  K-split and stream-K launches then need no
// memset launch for their counters / flags (4.7 us each on this chip, as many as K-split layers per frame).
extern "C" int swem_conv2d_nhwc_bf16x3_planes_ctr(void *stream, const void *x0, int c0, long long bs0, long long ps0,
                                                  const void *x1, int c1, long long bs1, long long ps1, const void *x2, int c2,
                                                  long long bs2, long long ps2, int B, int H, int W, const void *w_bf16x3,
                                                  const float *scale, const float *shift, const float *res, long long res_bs,
                                                  float *y, int Cout, int KH, int KW, int stride, int pad, int flags, int plan,
                                                  void *ws, size_t ws_bytes, void *planes, int nplanes, void *planes_relu,
                                                  int nplanes_relu, void *counters, size_t ncounters, void *fault) {
  PlaneOut po{{planes, planes_relu}, {nplanes, nplanes_relu}, static_cast<unsigned *>(counters), ncounters};
  po.fault = static_cast<unsigned *>(fault);
  return conv2d_bf16x3_impl(stream, x0, c0, bs0, ps0, x1, c1, bs1, ps1, x2, c2, bs2, ps2, B, H, W, w_bf16x3, scale, shift, res,
                            res_bs, y, Cout, KH, KW, stride, pad, flags, plan, ws, ws_bytes, &po);
}
// ... and with the RESIDUAL given as operand planes (see include/swem_hip.h)
extern "C" int swem_conv2d_nhwc_bf16x3_planes_res(void *stream, const void *x0, int c0, long long bs0, long long ps0,
                                                  const void *x1, int c1, long long bs1, long long ps1, const void *x2, int c2,
                                                  long long bs2, long long ps2, int B, int H, int W, const void *w_bf16x3,
                                                  const float *scale, const float *shift, const void *res_planes,
                                                  long long res_ps, long long res_npx, int res_nplanes, long long res_bs,
                                                  float *y, int Cout, int KH, int KW, int stride, int pad, int flags, int plan,
                                                  void *ws, size_t ws_bytes, void *planes, int nplanes, void *planes_relu,
                                                  int nplanes_relu, void *counters, size_t ncounters, void *fault) {
  PlaneOut po{{planes, planes_relu}, {nplanes, nplanes_relu}, static_cast<unsigned *>(counters), ncounters};
  po.fault = static_cast<unsigned *>(fault);
  po.res_planes = res_planes; po.res_ps = res_ps; po.res_npx = res_npx; po.res_npl = res_nplanes;
  SWEM_REQUIRE(res_planes, SWEM_E_ARG, "conv2d_bf16x3_planes_res: null residual planes");
  return conv2d_bf16x3_impl(stream, x0, c0, bs0, ps0, x1, c1, bs1, ps1, x2, c2, bs2, ps2, B, H, W, w_bf16x3, scale, shift, nullptr,
                            res_bs, y, Cout, KH, KW, stride, pad, flags, plan, ws, ws_bytes, &po);
}
// batched GEMM on pre-split planes (common.h): y[b] = x[b] . w[b]^T with per-batch filter planes, w_bs bf16 elements apart
int swem_gemm_bf16x3_batched(void *stream, const void *x, int K, long long bs, long long ps, int B, int M, const void *w,
                             long long w_bs, float *y, int Ncols, int plan, void *ws, size_t ws_bytes, void *y_planes,
                             int y_nplanes, float out_scale, void *fault) {
  PlaneOut po{{y_planes, nullptr}, {y_nplanes, 3}};
  po.fault = static_cast<unsigned *>(fault);
  return conv2d_bf16x3_impl(stream, x, K, bs, ps, nullptr, 0, 0, 0, nullptr, 0, 0, 0, B, M, 1, w, nullptr, nullptr, nullptr, 0, y,
                            Ncols, 1, 1, 1, 0, 0, plan, ws, ws_bytes, y_planes ? &po : nullptr, w_bs, out_scale);
}
