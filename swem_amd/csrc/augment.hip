// Augmentation of decoded training clips on the device (include/swem_hip_data.h; DESIGN.md section 8 defines the arithmetic).
//
//   aug_warp_kernel    one block per (clip, frame, 32x8 tile of the output): per pixel the TPS map (16 logs), the two affine forms
//                      M_aff (fill test) and M_src (source coordinate), a nearest label and a 4x4 bicubic of the HWC uint8 source
//                      (byte loads: a 53-pixel row is 159 bytes, nothing is aligned).  Writes the pre-colour planes into `frames`,
//                      label and region code into the workspace, the block's gray sum into ITS slot, and ORs frame 0's labels
//                      into the clip's 256-bit presence set (integer OR: any block order gives the same set).
//   aug_finish_kernel  same grid: the gray mean as a fixed-order sum of the slots, the colour chain in place, the object choice
//                      (every block repeats the clip's 256-entry scan: a ballot and a prefix count), masks, label, valid, found.
// No float atomics: two runs give the same bits.
#include "common.h"
#include "image_sample.h"
#include "../../include/swem_hip_data.h"

// Both forms of the two kernels (the clips' and the static chain's) must give the same bits where their parameters agree.  hipcc's
// default lets the back end fuse a multiply and an add wherever it finds them, which it decided differently in the two
// instantiations; `on` fuses exactly the a * b + c of one expression, so the arithmetic is what the source lines say.
#pragma clang fp contract(on)

namespace {

#define AUG_TW 32   // tile width  (a wave covers two rows of 32 pixels)
#define AUG_TH 8    // tile height

struct AugLayout {
  size_t wlab, wreg, presence, partial, total;
  int tiles_x, tiles;
};
inline AugLayout aug_layout(int B, int T, int Ho, int Wo) {
  AugLayout l;
  const size_t px = (size_t)B * T * Ho * Wo;
  l.tiles_x = cdiv(Wo, AUG_TW);
  l.tiles = l.tiles_x * cdiv(Ho, AUG_TH);
  l.wlab = 0;
  l.wreg = px;
  l.presence = align_up(2 * px, 256);
  l.partial = l.presence + align_up((size_t)B * 8 * sizeof(unsigned), 256);
  l.total = l.partial + align_up((size_t)B * T * l.tiles * sizeof(float), 256);
  return l;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

// one jitter: three ops in the order of `code` (2 bits each: 0 brightness, 1 contrast, 2 saturation, 3 none); m = the frame's
// gray mean before any colour op
__device__ __forceinline__ void jitter(float &r, float &g, float &b, int code, const float *__restrict__ f, float m) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int op = (code >> (2 * k)) & 3;
    if (op == 3) continue;
    const float fac = f[op];
    float add = 0.f;
    if (op == 1) add = (1.f - fac) * m;
    if (op == 2) add = (1.f - fac) * gray_of(r, g, b);
    r = clamp01(fac * r + add);
    g = clamp01(fac * g + add);
    b = clamp01(fac * b + add);
  }
}

// torchvision's adjust_hue on floats in [0,1] (_rgb2hsv / _hsv2rgb, the vector form of colorsys): h <- fmod(h + shift + 1, 1)
__device__ __forceinline__ void hue_shift(float &r, float &g, float &b, float shift) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.f : maxc), crd = eqc ? 1.f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  float h = maxc == r ? bc - gc : (maxc == g ? 2.f + rc - bc : 4.f + gc - rc);
  h = fmodf(h / 6.f + 1.f, 1.f);
  h = fmodf(h + shift + 1.f, 1.f);
  const float h6 = h * 6.f, fi = floorf(h6), f = h6 - fi;
  const int i = ((int)fi) % 6;
  const float v = maxc;
  const float p = clamp01(v * (1.f - s)), q = clamp01(v * (1.f - s * f)), t = clamp01(v * (1.f - s * (1.f - f)));
  r = i == 0 || i == 5 ? v : (i == 1 ? q : (i == 4 ? t : p));
  g = i == 1 || i == 2 ? v : (i == 3 ? q : (i == 0 ? t : p));
  b = i == 3 || i == 4 ? v : (i == 5 ? q : (i == 2 ? t : p));
}

// fixed-order sum over the block: lanes by shuffles, the four waves in order.  Every thread returns the same value.
__device__ __forceinline__ float block_sum(float v, float *red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// STATIC: the static chain's form (swem_augment_static_u8), which reads the frame record's last four words
template <bool STATIC>
__global__ __launch_bounds__(256) void aug_warp_kernel(const unsigned char *__restrict__ src, const unsigned char *__restrict__ lab,
                                                       const float *__restrict__ params, float *__restrict__ frames,
                                                       unsigned char *__restrict__ wlab, unsigned char *__restrict__ wreg,
                                                       float *__restrict__ partial, unsigned *__restrict__ presence, int T,
                                                       int Hs, int Ws, int Ho, int Wo, int tiles_x, int tiles) {
  __shared__ float red[4];
  __shared__ unsigned pres[8];
  const int tile = blockIdx.x, t = blockIdx.y, b = blockIdx.z;
  const size_t bt = (size_t)b * T + t;
  const float *P = params + bt * SWEM_AUG_FRAME_WORDS;
  const int *PI = reinterpret_cast<const int *>(P);
  if (threadIdx.x < 8) pres[threadIdx.x] = 0u;
  __syncthreads();
  // the source inside its slot: Hs, Ws stay the strides
  int hs = Hs, ws = Ws;
  bool src_fill = false;
  if constexpr (STATIC) {
    if (PI[SWEM_AUG_SRC_H] >= 1 && PI[SWEM_AUG_SRC_H] <= Hs) hs = PI[SWEM_AUG_SRC_H];
    if (PI[SWEM_AUG_SRC_W] >= 1 && PI[SWEM_AUG_SRC_W] <= Ws) ws = PI[SWEM_AUG_SRC_W];
    src_fill = (PI[SWEM_AUG_STATIC_FLAGS] & SWEM_AUG_FLAG_SRC_FILL) != 0;
  }

  const int i = (tile % tiles_x) * AUG_TW + (threadIdx.x & (AUG_TW - 1));
  const int j = (tile / tiles_x) * AUG_TH + (threadIdx.x / AUG_TW);
  const bool active = i < Wo && j < Ho;
  float gsum = 0.f;
  if (active) {
    // 1. thin-plate spline (thinplatespline/batch.py:115-133: a linspace grid, read back as grid_sample, align_corners=False)
    float u = (float)i, v = (float)j;
    if (PI[SWEM_AUG_TPS_ON]) {
      const float *Q = P + SWEM_AUG_TPS_AFFINE, *WX = P + SWEM_AUG_TPS_WX, *WY = P + SWEM_AUG_TPS_WY;
      const float xn = -1.f + (2.f * (float)i) / (float)(Wo - 1), yn = -1.f + (2.f * (float)j) / (float)(Ho - 1);
      float qx = Q[0] + Q[1] * xn + Q[2] * yn, qy = Q[3] + Q[4] * xn + Q[5] * yn;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const float ax = (float)(-1.0 + 2.0 * (k & 3) / 3.0), ay = (float)(-1.0 + 2.0 * (k >> 2) / 3.0);
        const float dx = xn - ax, dy = yn - ay;
        const float d = dx * dx + dy * dy;
        const float U = d * logf(d + 1e-9f);
        qx += WX[k] * U;
        qy += WY[k] * U;
      }
      u = ((qx + 1.f) * (float)Wo - 1.f) * 0.5f;
      v = ((qy + 1.f) * (float)Ho - 1.f) * 0.5f;
    }
    const bool outside = u <= -1.f || u >= (float)Wo || v <= -1.f || v >= (float)Ho;
    // 2. affine, 3. crop and flip: two affine forms of the centred coordinate
    const float xc = u + 0.5f - 0.5f * (float)Wo, yc = v + 0.5f - 0.5f * (float)Ho;
    const float *MA = P + SWEM_AUG_M_AFF, *MS = P + SWEM_AUG_M_SRC;
    const float xa = MA[0] * xc + MA[1] * yc + MA[2], ya = MA[3] * xc + MA[4] * yc + MA[5];
    bool fill = xa < 0.f || xa >= (float)Wo || ya < 0.f || ya >= (float)Ho;
    const float sx = MS[0] * xc + MS[1] * yc + MS[2], sy = MS[3] * xc + MS[4] * yc + MS[5];
    if constexpr (STATIC) fill = fill || (src_fill && (sx < 0.f || sx >= (float)ws || sy < 0.f || sy >= (float)hs));
    // 4. sample
    float r = 0.f, g = 0.f, bl = 0.f;
    int l = 0, region = SWEM_AUG_REGION_IMAGE;
    if (outside) {
      region = SWEM_AUG_REGION_OUTSIDE_TPS;
    } else if (fill) {
      region = SWEM_AUG_REGION_FILL;
      r = 124.f / 255.f;
      g = 116.f / 255.f;
      bl = 104.f / 255.f;
    } else {
      const size_t frame_px = bt * Hs * Ws;
      const int lx = min(max((int)floorf(sx), 0), ws - 1), ly = min(max((int)floorf(sy), 0), hs - 1);
      l = lab[frame_px + (size_t)ly * Ws + lx];
      const unsigned char *S = src + frame_px * 3;
      const float bx = sx - 0.5f, by = sy - 0.5f;
      const float fx = floorf(bx), fy = floorf(by);
      float wx[4], wy[4], acc[3];
      cubic_weights(bx - fx, wx);
      cubic_weights(by - fy, wy);
      cubic_accumulate<3, 0>((int)fx, (int)fy, ws, hs, wx, wy,
                          [&](int yy, int xx, float tap[3]) { rgb_bytes(S + (size_t)yy * Ws * 3 + 3 * xx, tap); }, acc);
      r = acc[0] / 255.f;
      g = acc[1] / 255.f;
      bl = acc[2] / 255.f;
    }
    const size_t plane = (size_t)Ho * Wo, pix = (size_t)j * Wo + i;
    float *F = frames + bt * 3 * plane + pix;
    F[0] = r;
    F[plane] = g;
    F[2 * plane] = bl;
    wlab[bt * plane + pix] = (unsigned char)l;
    wreg[bt * plane + pix] = (unsigned char)region;
    gsum = gray_of(r, g, bl);
    if (t == 0 && l != 0 && l != 255) atomicOr(&pres[l >> 5], 1u << (l & 31));
  }
  const float s = block_sum(gsum, red);   // (its barrier also orders the LDS ORs above)
  if (threadIdx.x == 0) partial[bt * tiles + tile] = s;
  if (t == 0 && threadIdx.x < 8 && pres[threadIdx.x]) atomicOr(presence + (size_t)b * 8 + threadIdx.x, pres[threadIdx.x]);
}

template <bool STATIC>
__global__ __launch_bounds__(256) void aug_finish_kernel(const float *__restrict__ params, float *__restrict__ frames,
                                                         float *__restrict__ masks, float *__restrict__ valid,
                                                         long long *__restrict__ label, int *__restrict__ found,
                                                         const unsigned char *__restrict__ wlab,
                                                         const unsigned char *__restrict__ wreg,
                                                         const float *__restrict__ partial, const unsigned *__restrict__ presence,
                                                         int B, int T, int Ho, int Wo, int N, int tiles_x, int tiles) {
  __shared__ float red[4];
  __shared__ int wcnt[4];
  __shared__ int chosen[SWEM_AUG_MAX_CHANNELS];
  const int tile = blockIdx.x, t = blockIdx.y, b = blockIdx.z;
  const size_t bt = (size_t)b * T + t;
  const float *P = params + bt * SWEM_AUG_FRAME_WORDS;
  const int *PI = reinterpret_cast<const int *>(P);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  // the frame's gray mean: slot k goes to thread k % 256, in ascending k; then the block's fixed-order sum
  float s = 0.f;
  for (int k = threadIdx.x; k < tiles; k += 256) s += partial[bt * tiles + k];
  if (threadIdx.x < SWEM_AUG_MAX_CHANNELS) chosen[threadIdx.x] = -1;
  const float mean = block_sum(s, red) / (float)((long long)Ho * Wo);

  // object choice: thread k looks at the label of priority k; the first N present ones, in that order
  const int *order = reinterpret_cast<const int *>(params + (size_t)B * T * SWEM_AUG_FRAME_WORDS) + (size_t)b * SWEM_AUG_CLIP_WORDS;
  const int cand = order[threadIdx.x] & 255;
  const bool present = cand != 0 && cand != 255 && ((presence[(size_t)b * 8 + (cand >> 5)] >> (cand & 31)) & 1u);
  const unsigned long long bal = __ballot(present);
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int before = __popcll(bal & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) before += wcnt[w];
  const int total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  if (present && before < N) chosen[before] = cand;
  __syncthreads();
  const int n = min(N, total);

  if (tile == 0 && t == 0) {
    if (threadIdx.x <= N) valid[(size_t)b * (N + 1) + threadIdx.x] = (int)threadIdx.x <= max(n, 1) ? 1.f : 0.f;
    if (threadIdx.x == 0) found[b] = total;
  }

  const int i = (tile % tiles_x) * AUG_TW + (threadIdx.x & (AUG_TW - 1));
  const int j = (tile / tiles_x) * AUG_TH + (threadIdx.x / AUG_TW);
  if (i >= Wo || j >= Ho) return;
  const size_t plane = (size_t)Ho * Wo, pix = (size_t)j * Wo + i;
  const int l = wlab[bt * plane + pix], region = wreg[bt * plane + pix];

  int ch = 0;
  for (int o = 0; o < n; ++o)
    if (l == chosen[o]) ch = o + 1;
  float *M = masks + bt * (N + 1) * plane + pix;
  for (int c = 0; c <= N; ++c) M[(size_t)c * plane] = c == ch ? 1.f : 0.f;
  label[bt * plane + pix] = ch;

  if (region == SWEM_AUG_REGION_OUTSIDE_TPS) return;   // stays 0, takes no colour op
  float *F = frames + bt * 3 * plane + pix;
  float r = F[0], g = F[plane], bl = F[2 * plane];
  if (region == SWEM_AUG_REGION_IMAGE) {   // (the fill enters after the clip-level ops)
    bool hue = false;
    if constexpr (STATIC) hue = P[SWEM_AUG_HUE] != 0.f;
    if (hue) {   // the clip-level jitter's four ops: `before` of the three, the hue op, the rest
      const int before = (PI[SWEM_AUG_STATIC_FLAGS] >> SWEM_AUG_FLAG_HUE_BEFORE_SHIFT) & SWEM_AUG_FLAG_HUE_BEFORE_MASK;
      jitter(r, g, bl, PI[SWEM_AUG_CLIP_ORDER] | (0x3f << (2 * before)), P + SWEM_AUG_CLIP_FACTORS, mean);
      hue_shift(r, g, bl, P[SWEM_AUG_HUE]);
      jitter(r, g, bl, PI[SWEM_AUG_CLIP_ORDER] | ((1 << (2 * before)) - 1), P + SWEM_AUG_CLIP_FACTORS, mean);
    } else {
      jitter(r, g, bl, PI[SWEM_AUG_CLIP_ORDER], P + SWEM_AUG_CLIP_FACTORS, mean);
    }
    if (PI[SWEM_AUG_GRAY]) r = g = bl = gray_of(r, g, bl);
  }
  jitter(r, g, bl, PI[SWEM_AUG_FRAME_ORDER], P + SWEM_AUG_FRAME_FACTORS, mean);
  F[0] = r;
  F[plane] = g;
  F[2 * plane] = bl;
}

}  // namespace

#define ST static_cast<hipStream_t>(stream)

extern "C" size_t swem_augment_workspace(int B, int T, int Ho, int Wo) {
  if (B <= 0 || T <= 0 || Ho <= 0 || Wo <= 0) return 0;
  return aug_layout(B, T, Ho, Wo).total;
}

namespace {
template <bool STATIC>
int augment_launch(const char *who, void *stream, const unsigned char *src, const unsigned char *lab, const void *params,
                   float *frames, float *masks, float *valid, long long *label, int *found, int B, int T, int Hs, int Ws, int Ho,
                   int Wo, int N, void *ws, size_t ws_bytes) {
  SWEM_REQUIRE(src && lab && params && frames && masks && valid && label && found && ws, SWEM_E_ARG, "%s: null pointer", who);
  SWEM_REQUIRE(((uintptr_t)params % 4) == 0 && ((uintptr_t)ws % 4) == 0 && ((uintptr_t)label % 8) == 0, SWEM_E_ARG,
               "%s: params and ws must be 4-byte aligned, label 8-byte aligned", who);
  SWEM_REQUIRE(B > 0 && T > 0 && Hs > 0 && Ws > 0, SWEM_E_SHAPE, "%s: need B, T, Hs, Ws > 0, got B=%d T=%d Hs=%d Ws=%d", who, B, T,
               Hs, Ws);
  SWEM_REQUIRE(Ho >= 2 && Wo >= 2, SWEM_E_SHAPE, "%s: need an output of at least 2x2 (the TPS grid divides by Ho-1, Wo-1), got %dx%d",
               who, Ho, Wo);
  SWEM_REQUIRE(N >= 1 && N + 1 <= SWEM_AUG_MAX_CHANNELS, SWEM_E_SHAPE, "%s: need 1 <= N and N + 1 <= %d mask channels, got N=%d", who,
               SWEM_AUG_MAX_CHANNELS, N);
  SWEM_REQUIRE(B <= 65535 && T <= 65535, SWEM_E_SHAPE, "%s: B=%d, T=%d exceed one launch (65535 each)", who, B, T);
  SWEM_REQUIRE((long long)Hs * Ws <= 0x7fffffffLL / 3 && (long long)Ho * Wo <= 0x7fffffffLL, SWEM_E_SHAPE,
               "%s: a frame of %dx%d -> %dx%d exceeds 32-bit pixel offsets", who, Hs, Ws, Ho, Wo);
  const AugLayout L = aug_layout(B, T, Ho, Wo);
  SWEM_REQUIRE(ws_bytes >= L.total, SWEM_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, L.total);
  unsigned char *w = static_cast<unsigned char *>(ws);
  unsigned *presence = reinterpret_cast<unsigned *>(w + L.presence);
  float *partial = reinterpret_cast<float *>(w + L.partial);
  if constexpr (STATIC) {
    // a launch, not a memset node: replayed back to back, a captured call's memset node was seen to leave a stale pattern in
    // the presence set; the clips' entry keeps its memset node, as it always had
    hipLaunchKernelGGL(clear_words_kernel, dim3((unsigned)cdiv((long long)B * 8, 256)), dim3(256), 0, ST, presence, B * 8);
    SWEM_CHECK_LAUNCH("aug_clear");
  } else {
    hipError_t e = hipMemsetAsync(presence, 0, (size_t)B * 8 * sizeof(unsigned), ST);
    if (e != hipSuccess) {
      swem_set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
      return SWEM_E_HIP;
    }
  }
  const dim3 grid((unsigned)L.tiles, (unsigned)T, (unsigned)B);
  const float *par = static_cast<const float *>(params);
  hipLaunchKernelGGL(aug_warp_kernel<STATIC>, grid, dim3(256), 0, ST, src, lab, par, frames, w + L.wlab, w + L.wreg, partial,
                     presence, T, Hs, Ws, Ho, Wo, L.tiles_x, L.tiles);
  SWEM_CHECK_LAUNCH("aug_warp");
  hipLaunchKernelGGL(aug_finish_kernel<STATIC>, grid, dim3(256), 0, ST, par, frames, masks, valid, label, found, w + L.wlab,
                     w + L.wreg, partial, presence, B, T, Ho, Wo, N, L.tiles_x, L.tiles);
  SWEM_CHECK_LAUNCH("aug_finish");
  return SWEM_OK;
}
}  // namespace

extern "C" int swem_augment_clips_u8(void *stream, const unsigned char *src, const unsigned char *lab, const void *params,
                                     float *frames, float *masks, float *valid, long long *label, int *found, int B, int T,
                                     int Hs, int Ws, int Ho, int Wo, int N, void *ws, size_t ws_bytes) {
  return augment_launch<false>("augment_clips", stream, src, lab, params, frames, masks, valid, label, found, B, T, Hs, Ws, Ho, Wo,
                               N, ws, ws_bytes);
}

extern "C" int swem_augment_static_u8(void *stream, const unsigned char *src, const unsigned char *lab, const void *params,
                                      float *frames, float *masks, float *valid, long long *label, int *found, int B, int T,
                                      int Hs, int Ws, int Ho, int Wo, int N, void *ws, size_t ws_bytes) {
  return augment_launch<true>("augment_static", stream, src, lab, params, frames, masks, valid, label, found, B, T, Hs, Ws, Ho, Wo,
                              N, ws, ws_bytes);
}
