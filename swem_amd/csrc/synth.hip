// Stage-0 training clips from static images: synthesis_frames of the reference (datasets/static_dataset.py:82-147) on the device
// (include/swem_hip_data.h; DESIGN.md section 9 defines the arithmetic).
//
//   clear_words_kernel      (image_sample.h) zeroes the statistics.  A launch, not a memset node: in a replay of the captured stage-0 call the
//                           memset node left the buffer filled with a stale 8-byte pattern instead of zeros (B = 4, N = 2, 480x640
//                           slots), and these words become addresses.  The static chain's entry clears its
//                           presence set the same way: a captured stage-0 call holds no memset node.
//   synth_stats_kernel      one block per (clip, image, 32x8 tile of the slot): the foreground's bounding box, pixel count and colour
//                           sums.  Lanes by shuffles, waves through the LDS, one global integer max / add per word and block on the
//                           cleared words: any block order gives the same words.
//   synth_plan_kernel       one thread per (clip, frame, object): random_resize and place_object in float64 -> the placement table.
//   synth_composite_kernel  one block per (clip, frame, 32x8 tile): per output pixel the objects from the last pasted to the first;
//                           a hit is a nearest mask sample (integer arithmetic: exact) inside the box, its colour the project's cubic
//                           of the boxed image, taps clamped to the box; no hit: image 0, its own object painted with its mean colour.
// Every size and index that comes from the parameter block is clamped on the device: a wrong block gives wrong pictures, no fault.
#include "common.h"
#include "image_sample.h"
#include "../../include/swem_hip_data.h"

namespace {

#define SYN_TW 32
#define SYN_TH 8

struct SynthLayout {
  size_t stats, plan, total;
};
inline SynthLayout synth_layout(int B, int T, int N) {
  SynthLayout l;
  l.stats = 0;
  l.plan = align_up((size_t)B * N * SWEM_SYNTH_STAT_WORDS * sizeof(unsigned), 256);
  l.total = l.plan + align_up((size_t)B * T * N * SWEM_SYNTH_PLAN_WORDS * sizeof(int), 256);
  return l;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(256) void synth_stats_kernel(const unsigned char *__restrict__ imgs,
                                                          const unsigned char *__restrict__ masks,
                                                          const int *__restrict__ params, unsigned *__restrict__ stats, int N,
                                                          int Hmax, int Wmax, int tiles_x) {
  __shared__ unsigned red[4][SWEM_SYNTH_STAT_WORDS];
  const int tile = blockIdx.x, k = blockIdx.y, b = blockIdx.z;
  const int *C = params + (size_t)b * SWEM_SYNTH_CLIP_WORDS;
  const int n_img = clampi(C[SWEM_SYNTH_N_IMG], 1, N);
  if (k >= n_img) return;                                   // (the whole block)
  const int h = clampi(C[SWEM_SYNTH_SIZES + 2 * k], 1, Hmax), w = clampi(C[SWEM_SYNTH_SIZES + 2 * k + 1], 1, Wmax);
  const int x = (tile % tiles_x) * SYN_TW + (threadIdx.x & (SYN_TW - 1));
  const int y = (tile / tiles_x) * SYN_TH + (threadIdx.x / SYN_TW);
  unsigned v[SWEM_SYNTH_STAT_WORDS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (x < w && y < h) {
    const size_t px = (((size_t)b * N + k) * Hmax + y) * Wmax + x;
    if (masks[px] != 0) {
      const unsigned char *p = imgs + px * 3;
      v[SWEM_SYNTH_STAT_NOT_HMIN] = ~(unsigned)y;
      v[SWEM_SYNTH_STAT_NOT_WMIN] = ~(unsigned)x;
      v[SWEM_SYNTH_STAT_HMAX1] = (unsigned)y + 1u;
      v[SWEM_SYNTH_STAT_WMAX1] = (unsigned)x + 1u;
      v[SWEM_SYNTH_STAT_COUNT] = 1u;
      v[SWEM_SYNTH_STAT_SUM_R] = p[0];
      v[SWEM_SYNTH_STAT_SUM_G] = p[1];
      v[SWEM_SYNTH_STAT_SUM_B] = p[2];
    }
  }
  // the words before COUNT are built by max, COUNT and the sums by add
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < SWEM_SYNTH_STAT_COUNT; ++q) v[q] = max(v[q], (unsigned)__shfl_down((int)v[q], off));
#pragma unroll
    for (int q = SWEM_SYNTH_STAT_COUNT; q < SWEM_SYNTH_STAT_WORDS; ++q) v[q] += (unsigned)__shfl_down((int)v[q], off);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < SWEM_SYNTH_STAT_WORDS; ++q) red[threadIdx.x >> 6][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < SWEM_SYNTH_STAT_WORDS) {
    const int q = threadIdx.x;
    unsigned *S = stats + ((size_t)b * N + k) * SWEM_SYNTH_STAT_WORDS + q;
    if (q < SWEM_SYNTH_STAT_COUNT) {
      const unsigned m = max(max(red[0][q], red[1][q]), max(red[2][q], red[3][q]));
      if (m) atomicMax(S, m);
    } else {
      const unsigned s = red[0][q] + red[1][q] + red[2][q] + red[3][q];
      if (s) atomicAdd(S, s);
    }
  }
}

__global__ __launch_bounds__(64) void synth_plan_kernel(const int *__restrict__ params, const unsigned *__restrict__ stats,
                                                        int *__restrict__ plan, int B, int T, int N, int Hmax, int Wmax) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= B * T * N) return;
  const int k = idx % N, t = (idx / N) % T, b = idx / (N * T);
  const int *C = params + (size_t)b * SWEM_SYNTH_CLIP_WORDS;
  const int *F = params + (size_t)B * SWEM_SYNTH_CLIP_WORDS + ((size_t)b * T + t) * SWEM_SYNTH_FRAME_WORDS;
  const float *O = reinterpret_cast<const float *>(F) + SWEM_SYNTH_OBJECTS + 4 * k;   // area, aspect, ux, uy
  const unsigned *S = stats + ((size_t)b * N + k) * SWEM_SYNTH_STAT_WORDS;
  int *P = plan + (size_t)idx * SWEM_SYNTH_PLAN_WORDS;
  const int n_img = clampi(C[SWEM_SYNTH_N_IMG], 1, N);
  const int h0 = clampi(C[SWEM_SYNTH_SIZES], 1, Hmax), w0 = clampi(C[SWEM_SYNTH_SIZES + 1], 1, Wmax);
  int rh = 0, rw = 0, tx = 0, ty = 0, present = 0;
  if (k < n_img && S[SWEM_SYNTH_STAT_COUNT] != 0u) {
    present = 1;
    const double hc = (double)(S[SWEM_SYNTH_STAT_HMAX1] - ~S[SWEM_SYNTH_STAT_NOT_HMIN]);
    const double wc = (double)(S[SWEM_SYNTH_STAT_WMAX1] - ~S[SWEM_SYNTH_STAT_NOT_WMIN]);
    const double area = (double)O[0] * hc * wc, aspect = (double)O[1];
    const double ux = (double)O[2], uy = (double)O[3];
    // (a NaN or a huge value from a wrong block must not reach the cast: sizes stay within 4 slots)
    const double dh = fmin(fmax(rint(sqrt(area / aspect)), 1.0), 4.0 * Hmax), dw = fmin(fmax(rint(sqrt(area * aspect)), 1.0), 4.0 * Wmax);
    rh = dh == dh ? (int)dh : 1;
    rw = dw == dw ? (int)dw : 1;
    const int lox = rw / 2, hix = max(w0 - rw / 2, rw / 2), loy = rh / 2, hiy = max(h0 - rh / 2, rh / 2);
    const double sx = fmin(fmax(floor(ux * (double)(hix - lox + 1)), 0.0), (double)(hix - lox));
    const double sy = fmin(fmax(floor(uy * (double)(hiy - loy + 1)), 0.0), (double)(hiy - loy));
    tx = sx == sx ? (int)sx : 0;      // cx - rw/2 with cx = lo + ...
    ty = sy == sy ? (int)sy : 0;
  }
  P[SWEM_SYNTH_PLAN_RH] = rh;
  P[SWEM_SYNTH_PLAN_RW] = rw;
  P[SWEM_SYNTH_PLAN_TX] = tx;
  P[SWEM_SYNTH_PLAN_TY] = ty;
  P[SWEM_SYNTH_PLAN_ID] = k < n_img ? (C[SWEM_SYNTH_IDS + k] & 255) : 0;
  P[SWEM_SYNTH_PLAN_PRESENT] = present;
  for (int q = SWEM_SYNTH_PLAN_PRESENT + 1; q < SWEM_SYNTH_PLAN_WORDS; ++q) P[q] = 0;
}

struct SynObj {
  int k, rh, rw, tx, ty, id, hmin, wmin, hc, wc;
};

__global__ __launch_bounds__(256) void synth_composite_kernel(const unsigned char *__restrict__ imgs,
                                                              const unsigned char *__restrict__ masks,
                                                              const int *__restrict__ params, const unsigned *__restrict__ stats,
                                                              const int *__restrict__ plan, unsigned char *__restrict__ comp,
                                                              unsigned char *__restrict__ comp_lab, int B, int T, int N,
                                                              int Hmax, int Wmax, int tiles_x) {
  __shared__ SynObj obj[SWEM_SYNTH_MAX_IMAGES];   // in the order of the walk: the last pasted first
  __shared__ int nobj;
  __shared__ unsigned char mean_fg[4];
  const int tile = blockIdx.x, t = blockIdx.y, b = blockIdx.z;
  const int *C = params + (size_t)b * SWEM_SYNTH_CLIP_WORDS;
  const int *F = params + (size_t)B * SWEM_SYNTH_CLIP_WORDS + ((size_t)b * T + t) * SWEM_SYNTH_FRAME_WORDS;
  const int n_img = clampi(C[SWEM_SYNTH_N_IMG], 1, N);
  const int h0 = clampi(C[SWEM_SYNTH_SIZES], 1, Hmax), w0 = clampi(C[SWEM_SYNTH_SIZES + 1], 1, Wmax);
  if (threadIdx.x == 0) {
    int n = 0;
    for (int p = n_img - 1; p >= 0; --p) {
      const int k = F[SWEM_SYNTH_PASTE + p];
      if (k < 0 || k >= n_img) continue;
      const int *P = plan + (((size_t)b * T + t) * N + k) * SWEM_SYNTH_PLAN_WORDS;
      if (!P[SWEM_SYNTH_PLAN_PRESENT]) continue;
      const unsigned *S = stats + ((size_t)b * N + k) * SWEM_SYNTH_STAT_WORDS;
      // The box and the placement become addresses below.  They are this call's own words, but the workspace is the caller's memory:
      // whatever it holds when this block reads it (a second call on another stream sharing it, a stale or half-built table), the
      // box stays inside the slot and the sizes positive -- wrong words give a wrong picture, never an access outside the slot.
      SynObj o;
      o.k = k;
      o.rh = P[SWEM_SYNTH_PLAN_RH];
      o.rw = P[SWEM_SYNTH_PLAN_RW];
      if (o.rh < 1 || o.rw < 1) continue;
      o.tx = clampi(P[SWEM_SYNTH_PLAN_TX], 0, Wmax);
      o.ty = clampi(P[SWEM_SYNTH_PLAN_TY], 0, Hmax);
      o.id = P[SWEM_SYNTH_PLAN_ID];
      o.hmin = clampi((int)~S[SWEM_SYNTH_STAT_NOT_HMIN], 0, Hmax - 1);
      o.wmin = clampi((int)~S[SWEM_SYNTH_STAT_NOT_WMIN], 0, Wmax - 1);
      o.hc = clampi((int)S[SWEM_SYNTH_STAT_HMAX1] - o.hmin, 1, Hmax - o.hmin);
      o.wc = clampi((int)S[SWEM_SYNTH_STAT_WMAX1] - o.wmin, 1, Wmax - o.wmin);
      obj[n++] = o;
    }
    nobj = n;
  }
  if (threadIdx.x < 3) {
    const unsigned *S = stats + (size_t)b * N * SWEM_SYNTH_STAT_WORDS;
    const double m = (double)S[SWEM_SYNTH_STAT_SUM_R + threadIdx.x] / ((double)S[SWEM_SYNTH_STAT_COUNT] + 1e-8);
    mean_fg[threadIdx.x] = (unsigned char)floor(fmin(fmax(m, 0.0), 255.0) + 0.5);
  }
  __syncthreads();
  const int x = (tile % tiles_x) * SYN_TW + (threadIdx.x & (SYN_TW - 1));
  const int y = (tile / tiles_x) * SYN_TH + (threadIdx.x / SYN_TW);
  if (x >= w0 || y >= h0) return;
  const size_t px0 = ((size_t)b * N * Hmax + y) * Wmax + x;                 // image 0 of the clip
  const size_t out = (((size_t)b * T + t) * Hmax + y) * Wmax + x;
  const unsigned char m0 = masks[px0];
  if (n_img == 1) {                                                          // static_dataset.py:91-94
    comp[out * 3 + 0] = imgs[px0 * 3 + 0];
    comp[out * 3 + 1] = imgs[px0 * 3 + 1];
    comp[out * 3 + 2] = imgs[px0 * 3 + 2];
    comp_lab[out] = m0;
    return;
  }
  for (int q = 0; q < nobj; ++q) {
    const SynObj o = obj[q];
    const int dx = x - o.tx, dy = y - o.ty;
    if (dx < 0 || dx >= o.rw || dy < 0 || dy >= o.rh) continue;
    const int k_mx = min((int)(((long long)dx * o.wc) / o.rw), o.wc - 1), k_my = min((int)(((long long)dy * o.hc) / o.rh), o.hc - 1);
    const size_t base = ((size_t)b * N + o.k) * Hmax;
    if (masks[(base + o.hmin + k_my) * Wmax + o.wmin + k_mx] == 0) continue;
    const double bx = ((double)dx + 0.5) * (double)o.wc / (double)o.rw - 0.5, by = ((double)dy + 0.5) * (double)o.hc / (double)o.rh - 0.5;
    const double fx = floor(bx), fy = floor(by);
    float wx[4], wy[4], acc[3];
    cubic_weights((float)(bx - fx), wx);
    cubic_weights((float)(by - fy), wy);
    cubic_accumulate<3, 0>((int)fx, (int)fy, o.wc, o.hc, wx, wy, [&](int yy, int xx, float tap[3]) {
      rgb_bytes(imgs + (base + o.hmin + yy) * Wmax * 3 + 3 * (o.wmin + xx), tap);
    }, acc);
#pragma unroll
    for (int c = 0; c < 3; ++c) comp[out * 3 + c] = (unsigned char)floorf(fminf(fmaxf(acc[c], 0.f), 255.f) + 0.5f);
    comp_lab[out] = (unsigned char)o.id;
    return;
  }
  comp[out * 3 + 0] = m0 ? mean_fg[0] : imgs[px0 * 3 + 0];
  comp[out * 3 + 1] = m0 ? mean_fg[1] : imgs[px0 * 3 + 1];
  comp[out * 3 + 2] = m0 ? mean_fg[2] : imgs[px0 * 3 + 2];
  comp_lab[out] = 0;
}

}  // namespace

#define ST static_cast<hipStream_t>(stream)

extern "C" size_t swem_synth_workspace(int B, int T, int N) {
  if (B <= 0 || T <= 0 || N <= 0) return 0;
  return synth_layout(B, T, N).total;
}

extern "C" int swem_synth_frames_u8(void *stream, const unsigned char *imgs, const unsigned char *masks, const void *params,
                                    unsigned char *comp, unsigned char *comp_lab, int B, int T, int N, int Hmax, int Wmax,
                                    void *ws, size_t ws_bytes) {
  SWEM_REQUIRE(imgs && masks && params && comp && comp_lab && ws, SWEM_E_ARG, "synth_frames: null pointer");
  SWEM_REQUIRE(((uintptr_t)params % 4) == 0 && ((uintptr_t)ws % 4) == 0, SWEM_E_ARG,
               "synth_frames: params and ws must be 4-byte aligned");
  SWEM_REQUIRE(B > 0 && T > 0 && Hmax > 0 && Wmax > 0, SWEM_E_SHAPE,
               "synth_frames: need B, T, Hmax, Wmax > 0, got B=%d T=%d Hmax=%d Wmax=%d", B, T, Hmax, Wmax);
  SWEM_REQUIRE(N >= 1 && N <= SWEM_SYNTH_MAX_IMAGES, SWEM_E_SHAPE, "synth_frames: need 1 <= N <= %d images, got N=%d",
               SWEM_SYNTH_MAX_IMAGES, N);
  SWEM_REQUIRE(Hmax <= 4096 && Wmax <= 4096, SWEM_E_SHAPE,
               "synth_frames: a slot of %dx%d exceeds 4096x4096 (the 32-bit colour sums)", Hmax, Wmax);
  SWEM_REQUIRE(B <= 65535 && T <= 65535 && (long long)B * T * N <= 0x7fffffffLL / 64, SWEM_E_SHAPE,
               "synth_frames: B=%d, T=%d exceed one launch (65535 each)", B, T);
  const SynthLayout L = synth_layout(B, T, N);
  SWEM_REQUIRE(ws_bytes >= L.total, SWEM_E_WORKSPACE, "synth_frames: workspace %zu < %zu bytes", ws_bytes, L.total);
  unsigned char *w = static_cast<unsigned char *>(ws);
  unsigned *stats = reinterpret_cast<unsigned *>(w + L.stats);
  int *plan = reinterpret_cast<int *>(w + L.plan);
  const int nstat = B * N * SWEM_SYNTH_STAT_WORDS;
  hipLaunchKernelGGL(clear_words_kernel, dim3((unsigned)cdiv(nstat, 256)), dim3(256), 0, ST, stats, nstat);
  SWEM_CHECK_LAUNCH("synth_clear");
  const int tiles_x = cdiv(Wmax, SYN_TW), tiles = tiles_x * cdiv(Hmax, SYN_TH);
  const int *par = static_cast<const int *>(params);
  hipLaunchKernelGGL(synth_stats_kernel, dim3((unsigned)tiles, (unsigned)N, (unsigned)B), dim3(256), 0, ST, imgs, masks, par, stats,
                     N, Hmax, Wmax, tiles_x);
  SWEM_CHECK_LAUNCH("synth_stats");
  hipLaunchKernelGGL(synth_plan_kernel, dim3((unsigned)cdiv((long long)B * T * N, 64)), dim3(64), 0, ST, par, stats, plan, B, T, N,
                     Hmax, Wmax);
  SWEM_CHECK_LAUNCH("synth_plan");
  hipLaunchKernelGGL(synth_composite_kernel, dim3((unsigned)tiles, (unsigned)T, (unsigned)B), dim3(256), 0, ST, imgs, masks, par,
                     stats, plan, comp, comp_lab, B, T, N, Hmax, Wmax, tiles_x);
  SWEM_CHECK_LAUNCH("synth_composite");
  return SWEM_OK;
}
