// Lovasz-softmax auxiliary loss of the training step on gfx950 (losses/lovasz_losses.py:19-31, 155-220 with the defaults
// classes='present', per_image=True, ignore=None that losses/__init__.py:34-63 calls it with).  C ABI: include/swem_hip_train.h.
//
// Per frame, clip b and valid channel c the reference sorts the HW errors e = |fg - p| in descending order and dots them with the
// differenced Jaccard index along that order.  Here: a STABLE segmented least-significant-digit radix sort of (key, payload)
// pairs over all B*N1 segments of the frame at once, then a prefix count of foreground pixels along the order and the closed form
// of the Jaccard difference on INTEGER counts.
//   key     = bits(e): e lies in [0, 1], so the unsigned order is the float order and key <= 0x3F800000 (30 significant bits)
//   payload = pixel | fg << 31
//   order   : descending error, ties by ascending pixel -- an ascending stable sort of  0x3F800000 - key  from the pixel order
//   digits  : 3 passes of 10 bits = the 30 bits exactly
// Every pass is three ordinary launches (per-tile digit histogram, scan of the histograms, scatter); a block never waits for
// another block.  Sums that feed a scalar are fp64 in a fixed order, counts are integers: same inputs, same bits.
#include <math.h>

#include "../../include/swem_hip_train.h"
#include "common.h"
#include "loss_common.h"

namespace {

constexpr unsigned LV_KMAX = 0x3F800000u;     // bits(1.0f)
constexpr int LV_BITS = 10, LV_BINS = 1 << LV_BITS, LV_PASSES = 3;
constexpr int LV_THREADS = 256, LV_WAVES = LV_THREADS / 64, LV_ITEMS = 8;
constexpr int LV_TILE = LV_THREADS * LV_ITEMS;   // keys of one block: wave w owns keys [w*512, w*512 + 512) of the tile, in order

__device__ __forceinline__ unsigned lv_digit(unsigned key, int shift) { return ((LV_KMAX - key) >> shift) & (LV_BINS - 1); }

// lanes of the wave that hold the same digit (among the lanes with ok)
__device__ __forceinline__ unsigned long long lv_match(unsigned d, bool ok) {
  unsigned long long m = __ballot(ok);
#pragma unroll
  for (int b = 0; b < LV_BITS; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long bb = __ballot(ok && bit);
    m &= bit ? bb : ~bb;
  }
  return m;
}

__device__ __forceinline__ unsigned long long lv_lanemask_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// exclusive scan of one int per thread over a block of `nw` waves; *total (may be NULL) = the block's sum.  sh: nw + 1 ints.
__device__ __forceinline__ int block_excl_scan(int v, int *sh, int nw, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int w = 0; w < nw; ++w) {
      const int t = sh[w];
      sh[w] = run;
      run += t;
    }
    sh[nw] = run;
  }
  __syncthreads();
  if (total) *total = sh[nw];
  return sh[wave] + inc - v;
}

// rank of channel c among the valid channels of clip b, -1 if c is not valid
__device__ __forceinline__ int lv_rank(const float *__restrict__ valid, int b, int c, int N1) {
  if (!valid) return c;
  if (!(valid[b * N1 + c] > 0.5f)) return -1;
  int r = 0;
  for (int j = 0; j < c; ++j) r += valid[b * N1 + j] > 0.5f ? 1 : 0;
  return r;
}

// block-wide digit histogram of ITEMS rounds of keys: match-and-count per wave, so that keys sharing a digit (loss-like values
// share their top bits almost everywhere) cost one LDS update per wave and round, not one per lane
__device__ __forceinline__ void lv_count(unsigned *bh, unsigned d, bool ok) {
  const unsigned long long m = lv_match(d, ok);
  if (ok && (m & lv_lanemask_lt()) == 0ull) atomicAdd(&bh[d], (unsigned)__popcll(m));   // (integer counts: any order, same sum)
}

// keys / payloads of every valid segment, its first-digit histogram per tile and its foreground count per tile
__global__ __launch_bounds__(LV_THREADS) void lovasz_keys_kernel(const float *__restrict__ prob,
                                                                  const long long *__restrict__ label, long long label_bs,
                                                                  const float *__restrict__ valid, unsigned *__restrict__ keys,
                                                                  unsigned *__restrict__ pay, unsigned *__restrict__ hist,
                                                                  int *__restrict__ gpart, int N1, long long HW, int ntiles) {
  __shared__ unsigned bh[LV_BINS];
  __shared__ int sh[LV_WAVES + 1];
  const int seg = blockIdx.y, tile = blockIdx.x;
  const int b = seg / N1, c = seg - b * N1;
  const int rank = lv_rank(valid, b, c, N1);
  if (rank < 0) return;                              // (the whole block: an invalid channel is not sorted)
  for (int d = threadIdx.x; d < LV_BINS; d += LV_THREADS) bh[d] = 0u;
  __syncthreads();
  int nfg = 0;
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long long i = (long long)tile * LV_TILE + r * LV_THREADS + threadIdx.x;
    const bool ok = i < HW;
    unsigned key = 0u;
    if (ok) {
      const bool fg = label[(long long)b * label_bs + i] == (long long)rank;
      const float e = fabsf((fg ? 1.f : 0.f) - prob[(long long)seg * HW + i]);
      key = __float_as_uint(e);
      keys[(long long)seg * HW + i] = key;
      pay[(long long)seg * HW + i] = (unsigned)i | (fg ? 0x80000000u : 0u);
      nfg += fg ? 1 : 0;
    }
    lv_count(bh, lv_digit(key, 0), ok);
  }
  int total;
  block_excl_scan(nfg, sh, LV_WAVES, &total);        // (also the barrier behind the histogram's updates)
  if (threadIdx.x == 0) gpart[(long long)seg * ntiles + tile] = total;
  unsigned *dst = hist + ((long long)seg * ntiles + tile) * LV_BINS;
  for (int d = threadIdx.x; d < LV_BINS; d += LV_THREADS) dst[d] = bh[d];
}

// per-tile digit histogram of a later pass; seginfo[seg] = G, 0 for a segment that is skipped
__global__ __launch_bounds__(LV_THREADS) void lovasz_hist_kernel(const unsigned *__restrict__ keys,
                                                                  const int *__restrict__ seginfo, unsigned *__restrict__ hist,
                                                                  long long HW, int ntiles, int shift) {
  __shared__ unsigned bh[LV_BINS];
  const int seg = blockIdx.y, tile = blockIdx.x;
  if (seginfo[seg] <= 0) return;
  for (int d = threadIdx.x; d < LV_BINS; d += LV_THREADS) bh[d] = 0u;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long long i = (long long)tile * LV_TILE + r * LV_THREADS + threadIdx.x;
    const bool ok = i < HW;
    const unsigned key = ok ? keys[(long long)seg * HW + i] : 0u;
    lv_count(bh, lv_digit(key, shift), ok);
  }
  __syncthreads();
  unsigned *dst = hist + ((long long)seg * ntiles + tile) * LV_BINS;
  for (int d = threadIdx.x; d < LV_BINS; d += LV_THREADS) dst[d] = bh[d];
}

// hist[seg][tile][d] (counts) -> the first output position of digit d of that tile: digits ascending, tiles ascending within a
// digit.  One block per segment, thread d owns digit d.  first != 0: also seginfo[seg] = G from the tiles' foreground counts
// (0 for an invalid channel -- and for an absent class, which is then skipped by every later launch)
__global__ __launch_bounds__(LV_BINS) void lovasz_scan_kernel(unsigned *__restrict__ hist, int *__restrict__ seginfo,
                                                               const int *__restrict__ gpart, const float *__restrict__ valid,
                                                               int N1, int ntiles, int first) {
  __shared__ int sh[LV_BINS / 64 + 1];
  const int seg = blockIdx.x;
  if (first) {
    const int b = seg / N1, c = seg - b * N1;
    const bool ok = !valid || valid[b * N1 + c] > 0.5f;      // (uniform over the block)
    int g = 0;
    if (ok)
      for (int t = threadIdx.x; t < ntiles; t += LV_BINS) g += gpart[(long long)seg * ntiles + t];
    int G;
    block_excl_scan(g, sh, LV_BINS / 64, &G);
    if (threadIdx.x == 0) seginfo[seg] = ok ? G : 0;
    if (!ok || G <= 0) return;
  } else if (seginfo[seg] <= 0) {
    return;
  }
  unsigned *h = hist + (long long)seg * ntiles * LV_BINS + threadIdx.x;
  // (eight tiles' counts in flight at a time: the walk over the tiles is a chain of L2 round trips otherwise)
  constexpr int U = 8;
  int tot = 0;
  for (int t0 = 0; t0 < ntiles; t0 += U) {
    unsigned n[U];
#pragma unroll
    for (int j = 0; j < U; ++j) n[j] = t0 + j < ntiles ? h[(long long)(t0 + j) * LV_BINS] : 0u;
#pragma unroll
    for (int j = 0; j < U; ++j) tot += (int)n[j];
  }
  unsigned run = (unsigned)block_excl_scan(tot, sh, LV_BINS / 64, nullptr);
  for (int t0 = 0; t0 < ntiles; t0 += U) {
    unsigned n[U];
#pragma unroll
    for (int j = 0; j < U; ++j) n[j] = t0 + j < ntiles ? h[(long long)(t0 + j) * LV_BINS] : 0u;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      if (t0 + j < ntiles) h[(long long)(t0 + j) * LV_BINS] = run;
      run += n[j];
    }
  }
}

// stable scatter of one tile by one digit.  Wave w owns the keys [w*ITEMS*64, (w+1)*ITEMS*64) of the tile, 64 consecutive keys a
// round: a key's position among the tile's keys of its digit = those of earlier waves + those of earlier rounds of its wave +
// those of lower lanes.  The output index is checked against HW before the store.
__global__ __launch_bounds__(LV_THREADS) void lovasz_scatter_kernel(const unsigned *__restrict__ kin,
                                                                     const unsigned *__restrict__ pin,
                                                                     unsigned *__restrict__ kout, unsigned *__restrict__ pout,
                                                                     const unsigned *__restrict__ hist,
                                                                     const int *__restrict__ seginfo, long long HW, int ntiles,
                                                                     int shift) {
  __shared__ unsigned wh[LV_WAVES][LV_BINS];
  const int seg = blockIdx.y, tile = blockIdx.x;
  if (seginfo[seg] <= 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = threadIdx.x; d < LV_WAVES * LV_BINS; d += LV_THREADS) (&wh[0][0])[d] = 0u;
  __syncthreads();
  const long long base = (long long)seg * HW;
  unsigned key[LV_ITEMS], pl[LV_ITEMS], pos[LV_ITEMS];
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long long i = (long long)tile * LV_TILE + (wave * LV_ITEMS + r) * 64 + lane;
    const bool ok = i < HW;
    key[r] = ok ? kin[base + i] : 0u;
    pl[r] = ok ? pin[base + i] : 0u;
    const unsigned d = lv_digit(key[r], shift);
    const unsigned long long m = lv_match(d, ok);
    const int leader = ok ? __ffsll((long long)m) - 1 : lane;
    unsigned before = 0u;
    if (ok && lane == leader) {
      before = wh[wave][d];
      wh[wave][d] = before + (unsigned)__popcll(m);
    }
    before = __shfl(before, leader);
    pos[r] = before + (unsigned)__popcll(m & lv_lanemask_lt());
    __syncthreads();                                  // (the next round reads what this round's leaders wrote)
  }
  // counts per (wave, digit) -> first output position of (tile, wave, digit)
  const unsigned *off = hist + ((long long)seg * ntiles + tile) * LV_BINS;
  for (int d = threadIdx.x; d < LV_BINS; d += LV_THREADS) {
    unsigned run = off[d];
#pragma unroll
    for (int w = 0; w < LV_WAVES; ++w) {
      const unsigned n = wh[w][d];
      wh[w][d] = run;
      run += n;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long long i = (long long)tile * LV_TILE + (wave * LV_ITEMS + r) * 64 + lane;
    if (i >= HW) continue;
    const long long o = (long long)wh[wave][lv_digit(key[r], shift)] + pos[r];
    if (o < HW) {
      kout[base + o] = key[r];
      pout[base + o] = pl[r];
    }
  }
}

// foreground pixels per tile of the sorted order
__global__ __launch_bounds__(LV_THREADS) void lovasz_fgcount_kernel(const unsigned *__restrict__ pay,
                                                                     const int *__restrict__ seginfo, int *__restrict__ fpart,
                                                                     long long HW, int ntiles) {
  __shared__ int sh[LV_WAVES + 1];
  const int seg = blockIdx.y, tile = blockIdx.x;
  if (seginfo[seg] <= 0) return;
  int n = 0;
#pragma unroll
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long long i = (long long)tile * LV_TILE + r * LV_THREADS + threadIdx.x;
    if (i < HW) n += (int)(pay[(long long)seg * HW + i] >> 31);
  }
  int total;
  block_excl_scan(n, sh, LV_WAVES, &total);
  if (threadIdx.x == 0) fpart[(long long)seg * ntiles + tile] = total;
}

// fpart[seg][tile] -> foreground pixels before the tile (exclusive scan over the tiles, in chunks of one block)
__global__ __launch_bounds__(LV_BINS) void lovasz_fgscan_kernel(int *__restrict__ fpart, const int *__restrict__ seginfo,
                                                                 int ntiles) {
  __shared__ int sh[LV_BINS / 64 + 1];
  const int seg = blockIdx.x;
  if (seginfo[seg] <= 0) return;
  int carry = 0;
  for (int t0 = 0; t0 < ntiles; t0 += LV_BINS) {
    const int t = t0 + threadIdx.x;
    const int v = t < ntiles ? fpart[(long long)seg * ntiles + t] : 0;
    int total;
    const int ex = block_excl_scan(v, sh, LV_BINS / 64, &total);
    if (t < ntiles) fpart[(long long)seg * ntiles + t] = carry + ex;
    carry += total;
    __syncthreads();
  }
}

// lovasz_losses.py:19-31 along the sorted order, in closed form on integer counts.  Position k of a segment with G foreground
// pixels, cf of them before k, U = G + (k - cf):  g = 1/U for a foreground pixel, (G - cf) / (U (U + 1)) for a background pixel
// (= jaccard[k] - jaccard[k-1], jaccard[0] undifferenced).  g goes to the pixel's place in glov, e*g into the tile's fp64 partial.
// A skipped segment gets glov = 0.
__global__ __launch_bounds__(LV_THREADS) void lovasz_grad_kernel(const unsigned *__restrict__ keys,
                                                                  const unsigned *__restrict__ pay,
                                                                  const int *__restrict__ seginfo, const int *__restrict__ fbase,
                                                                  float *__restrict__ glov, double *__restrict__ lpart,
                                                                  unsigned *__restrict__ keys_out, unsigned *__restrict__ pay_out,
                                                                  long long HW, int ntiles) {
  __shared__ int sh[LV_WAVES + 1];
  __shared__ double shd[LV_WAVES];
  const int seg = blockIdx.y, tile = blockIdx.x;
  const long long base = (long long)seg * HW;
  const int G = seginfo[seg];
  if (G <= 0) {
    if (glov)
      for (int r = 0; r < LV_ITEMS; ++r) {
        const long long i = (long long)tile * LV_TILE + r * LV_THREADS + threadIdx.x;
        if (i < HW) glov[base + i] = 0.f;
      }
    return;
  }
  int carry = fbase[(long long)seg * ntiles + tile];
  double acc = 0.0;
  for (int r = 0; r < LV_ITEMS; ++r) {
    const long long k = (long long)tile * LV_TILE + r * LV_THREADS + threadIdx.x;
    const bool ok = k < HW;
    const unsigned key = ok ? keys[base + k] : 0u;
    const unsigned p = ok ? pay[base + k] : 0u;
    const int fg = (int)(p >> 31);
    int total;
    const long long cf = (long long)carry + block_excl_scan(fg, sh, LV_WAVES, &total);
    carry += total;
    if (ok) {
      const double U = (double)((long long)G + (k - cf));
      const double g = fg ? 1.0 / U : (double)((long long)G - cf) / (U * (U + 1.0));
      acc += (double)__uint_as_float(key) * g;
      const long long px = (long long)(p & 0x7fffffffu);
      if (glov && px < HW) glov[base + px] = (float)g;
      if (keys_out) keys_out[base + k] = key;
      if (pay_out) pay_out[base + k] = p;
    }
  }
  acc = block_sum(acc, shd);
  if (threadIdx.x == 0) lpart[(long long)seg * ntiles + tile] = acc;
}

// lov[seg] = {loss_c, G}: the tiles' partials summed in index order
__global__ __launch_bounds__(LV_THREADS) void lovasz_segsum_kernel(const double *__restrict__ lpart,
                                                                    const int *__restrict__ seginfo, float *__restrict__ lov,
                                                                    int ntiles) {
  __shared__ double shd[LV_WAVES];
  const int seg = blockIdx.x;
  const int G = seginfo[seg];
  double a = 0.0;
  if (G > 0)
    for (int t = threadIdx.x; t < ntiles; t += LV_THREADS) a += lpart[(long long)seg * ntiles + t];
  a = block_sum(a, shd);
  if (threadIdx.x == 0) {
    lov[seg * 2] = (float)a;
    lov[seg * 2 + 1] = (float)G;
  }
}

// losses/__init__.py:57-61 with aux = lovasz_softmax: main as loss_reduce_kernel (train.hip), aux = mean over clips of the mean
// over frames of the mean over the frame's present classes (0 for a frame without one)
__global__ void lovasz_reduce_kernel(const float *__restrict__ rowstat, const float *__restrict__ lov,
                                     float *__restrict__ losses, int B, int N1, int T, long long HW, long long k_arg,
                                     const long long *__restrict__ k_dev, float aux_ratio) {
  if (threadIdx.x != 0) return;
  const long long k = k_dev ? *k_dev : k_arg;
  const double keff = k > 0 ? (double)k : (double)HW;
  double main = 0.0;
  for (int r = 0; r < T * B; ++r) {
    const float *s = rowstat + r * 4;
    main += ((double)s[2] + (keff - (double)s[1]) * (double)s[0]) / keff;
  }
  main /= (double)(T * B);
  double aux = 0.0;
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t) {
      int np = 0;
      double acc = 0.0;
      for (int c = 0; c < N1; ++c) {
        const float *q = lov + (((long long)t * B + b) * N1 + c) * 2;
        if (q[1] > 0.f) {
          ++np;
          acc += (double)q[0];
        }
      }
      if (np) aux += acc / (double)np;
    }
  aux /= (double)(T * B);
  losses[0] = (float)(main + (double)aux_ratio * aux);
  losses[1] = (float)main;
  losses[2] = (float)aux;
}

// d total / d logits of one frame: the cross-entropy term exactly as loss_pixel_bwd_kernel (train.hip) forms it, the Lovasz term
// d_c = sign(p_c - fg_c) * glov_c / (n_present T B) (sign(0) = 0, as torch.abs) through the softmax Jacobian
__global__ __launch_bounds__(256) void lovasz_pixel_bwd_kernel(const float *__restrict__ prob, const float *__restrict__ raw,
                                                               const long long *__restrict__ label,
                                                               const float *__restrict__ valid,
                                                               const float *__restrict__ rowstat, const float *__restrict__ lov,
                                                               const float *__restrict__ glov, float *__restrict__ dlogits,
                                                               int B, int N1, int T, long long HW, long long k_arg,
                                                               float aux_ratio, const float *__restrict__ gout,
                                                               long long label_bs, const long long *__restrict__ k_dev) {
  const long long k = k_dev ? *k_dev : k_arg;
  const float gscale = gout ? gout[0] : 1.f;
  const int b = blockIdx.y;
  const long long px = (long long)blockIdx.x * 256 + threadIdx.x;
  if (px >= HW) return;
  const float *rs = rowstat + b * 4;
  const float keff = k > 0 ? (float)k : (float)HW;
  const float x = raw[(long long)b * HW + px];
  float w;
  if (k == 0 || x > rs[0]) w = 1.f;
  else if (x == rs[0]) w = (keff - rs[1]) / rs[3];
  else w = 0.f;
  w /= keff * (float)(B * T);
  const int tgt = (int)label[(long long)b * label_bs + px];
  float p[LOSS_MAXC], d[LOSS_MAXC], oh[LOSS_MAXC];
  bool ok[LOSS_MAXC];
  int nv = 0, np = 0;
#pragma unroll
  for (int c = 0; c < LOSS_MAXC; ++c) {
    ok[c] = c < N1 && (!valid || valid[b * N1 + c] > 0.5f);
    oh[c] = (ok[c] && nv == tgt) ? 1.f : 0.f;
    nv += ok[c] ? 1 : 0;
    p[c] = ok[c] ? prob[((long long)b * N1 + c) * HW + px] : 0.f;
    np += (ok[c] && lov[(b * N1 + c) * 2 + 1] > 0.f) ? 1 : 0;
  }
  const float s = np ? 1.f / ((float)np * (float)(B * T)) : 0.f;
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < LOSS_MAXC; ++c) {
    d[c] = 0.f;
    if (!ok[c] || !(lov[(b * N1 + c) * 2 + 1] > 0.f)) continue;
    const float df = p[c] - oh[c];
    const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
    d[c] = sg * glov[((long long)b * N1 + c) * HW + px] * s;
    dot += p[c] * d[c];
  }
#pragma unroll
  for (int c = 0; c < LOSS_MAXC; ++c) {
    if (c >= N1) continue;
    const float g = ok[c] ? w * (p[c] - oh[c]) + aux_ratio * (p[c] * (d[c] - dot)) : 0.f;
    dlogits[((long long)b * N1 + c) * HW + px] = g * gscale;
  }
}

// workspace layout of one frame call (every array 256-byte aligned)
struct LvLayout {
  size_t keys[2], pay[2], hist, gpart, fpart, seginfo, lpart, total;
  int ntiles;
};
inline LvLayout lv_layout(int B, int N1, long long HW) {
  LvLayout L;
  const size_t S = (size_t)B * N1;
  L.ntiles = cdiv(HW, LV_TILE);
  size_t o = 0;
  auto take = [&o](size_t bytes) {
    const size_t at = o;
    o += align_up(bytes, 256);
    return at;
  };
  for (int i = 0; i < 2; ++i) L.keys[i] = take(S * (size_t)HW * 4);
  for (int i = 0; i < 2; ++i) L.pay[i] = take(S * (size_t)HW * 4);
  L.hist = take(S * L.ntiles * LV_BINS * 4);
  L.gpart = take(S * L.ntiles * 4);
  L.fpart = take(S * L.ntiles * 4);
  L.seginfo = take(S * 4);
  L.lpart = take(S * L.ntiles * 8);
  L.total = o;
  return L;
}
inline bool lv_shape_ok(int B, int N1, long long HW) {
  // (B*N1 is a grid's y extent; HW < 2^31: the payload keeps the pixel in 31 bits)
  return B > 0 && N1 >= 2 && N1 <= LOSS_MAXC && HW > 0 && HW < (1ll << 31) && (long long)B * N1 <= 65535;
}

}  // namespace

extern "C" size_t swem_lovasz_workspace(int B, int N1, long long HW) {
  if (!lv_shape_ok(B, N1, HW)) return 0;
  return lv_layout(B, N1, HW).total;
}

extern "C" int swem_lovasz_frame_fwd_f32(void *stream, const float *prob, const long long *label, long long label_bs,
                                         const float *valid, float *glov, float *lov, unsigned *keys_out,
                                         unsigned *payload_out, int B, int N1, long long HW, void *ws, size_t ws_bytes) {
  SWEM_REQUIRE(prob && label && lov, SWEM_E_ARG, "lovasz_fwd: null pointer");
  SWEM_REQUIRE(lv_shape_ok(B, N1, HW), SWEM_E_SHAPE, "lovasz_fwd: B=%d N1=%d (2..%d) HW=%lld (< 2^31), B*N1 <= 65535", B, N1,
               LOSS_MAXC, HW);
  const LvLayout L = lv_layout(B, N1, HW);
  SWEM_REQUIRE(ws && ws_bytes >= L.total, SWEM_E_WORKSPACE, "lovasz_fwd: workspace %zu < %zu bytes", ws_bytes, L.total);
  SWEM_REQUIRE((uintptr_t)ws % 8 == 0, SWEM_E_ARG, "lovasz_fwd: workspace must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *w = static_cast<char *>(ws);
  unsigned *keys[2] = {reinterpret_cast<unsigned *>(w + L.keys[0]), reinterpret_cast<unsigned *>(w + L.keys[1])};
  unsigned *pay[2] = {reinterpret_cast<unsigned *>(w + L.pay[0]), reinterpret_cast<unsigned *>(w + L.pay[1])};
  unsigned *hist = reinterpret_cast<unsigned *>(w + L.hist);
  int *gpart = reinterpret_cast<int *>(w + L.gpart), *fpart = reinterpret_cast<int *>(w + L.fpart);
  int *seginfo = reinterpret_cast<int *>(w + L.seginfo);
  double *lpart = reinterpret_cast<double *>(w + L.lpart);
  const int S = B * N1, nt = L.ntiles;
  const dim3 tiles(nt, S);
  hipLaunchKernelGGL(lovasz_keys_kernel, tiles, dim3(LV_THREADS), 0, st, prob, label, label_bs, valid, keys[0], pay[0], hist,
                     gpart, N1, HW, nt);
  SWEM_CHECK_LAUNCH("lovasz_keys_kernel");
  int cur = 0;
  for (int pass = 0; pass < LV_PASSES; ++pass) {
    const int shift = pass * LV_BITS;
    if (pass > 0) {
      hipLaunchKernelGGL(lovasz_hist_kernel, tiles, dim3(LV_THREADS), 0, st, keys[cur], seginfo, hist, HW, nt, shift);
      SWEM_CHECK_LAUNCH("lovasz_hist_kernel");
    }
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3(S), dim3(LV_BINS), 0, st, hist, seginfo, gpart, valid, N1, nt, pass == 0);
    SWEM_CHECK_LAUNCH("lovasz_scan_kernel");
    hipLaunchKernelGGL(lovasz_scatter_kernel, tiles, dim3(LV_THREADS), 0, st, keys[cur], pay[cur], keys[cur ^ 1], pay[cur ^ 1],
                       hist, seginfo, HW, nt, shift);
    SWEM_CHECK_LAUNCH("lovasz_scatter_kernel");
    cur ^= 1;
  }
  hipLaunchKernelGGL(lovasz_fgcount_kernel, tiles, dim3(LV_THREADS), 0, st, pay[cur], seginfo, fpart, HW, nt);
  SWEM_CHECK_LAUNCH("lovasz_fgcount_kernel");
  hipLaunchKernelGGL(lovasz_fgscan_kernel, dim3(S), dim3(LV_BINS), 0, st, fpart, seginfo, nt);
  SWEM_CHECK_LAUNCH("lovasz_fgscan_kernel");
  hipLaunchKernelGGL(lovasz_grad_kernel, tiles, dim3(LV_THREADS), 0, st, keys[cur], pay[cur], seginfo, fpart, glov, lpart,
                     keys_out, payload_out, HW, nt);
  SWEM_CHECK_LAUNCH("lovasz_grad_kernel");
  hipLaunchKernelGGL(lovasz_segsum_kernel, dim3(S), dim3(LV_THREADS), 0, st, lpart, seginfo, lov, nt);
  SWEM_CHECK_LAUNCH("lovasz_segsum_kernel");
  return SWEM_OK;
}

extern "C" int swem_lovasz_reduce_f32(void *stream, const float *rowstat, const float *lov, float *losses, int B, int N1, int T,
                                      long long HW, long long k, const long long *k_dev, float aux_ratio) {
  SWEM_REQUIRE(rowstat && lov && losses, SWEM_E_ARG, "lovasz_reduce: null pointer");
  SWEM_REQUIRE(B > 0 && N1 >= 2 && N1 <= LOSS_MAXC && T > 0 && HW > 0, SWEM_E_SHAPE, "lovasz_reduce: bad shape");
  hipLaunchKernelGGL(lovasz_reduce_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), rowstat, lov, losses, B, N1,
                     T, HW, k, k_dev, aux_ratio);
  SWEM_CHECK_LAUNCH("lovasz_reduce_kernel");
  return SWEM_OK;
}

extern "C" int swem_lovasz_frame_bwd_f32(void *stream, const float *prob, const float *raw, const long long *label,
                                         long long label_bs, const float *valid, const float *rowstat, const float *lov,
                                         const float *glov, float *dlogits, int B, int N1, int T, long long HW, long long k,
                                         const long long *k_dev, float aux_ratio, const float *gout) {
  SWEM_REQUIRE(prob && raw && label && rowstat && lov && glov && dlogits, SWEM_E_ARG, "lovasz_bwd: null pointer");
  SWEM_REQUIRE(B > 0 && B <= 65535 && N1 >= 2 && N1 <= LOSS_MAXC && T > 0 && HW > 0 && HW < (1ll << 31), SWEM_E_SHAPE,
               "lovasz_bwd: bad shape");
  hipLaunchKernelGGL(lovasz_pixel_bwd_kernel, dim3(cdiv(HW, 256), B), dim3(256), 0, static_cast<hipStream_t>(stream), prob, raw,
                     label, valid, rowstat, lov, glov, dlogits, B, N1, T, HW, k, aux_ratio, gout, label_bs, k_dev);
  SWEM_CHECK_LAUNCH("lovasz_pixel_bwd_kernel");
  return SWEM_OK;
}
