// Evaluation staging from decoded bytes (include/swem_hip_io.h): four pointwise, memory-bound kernels either side of the
// timed loop.  Bytes come in (RGB frames, palette-PNG index maps), fp32 inputs / result bytes go out; the host touches no
// pixel.
//   stage_frames_kernel   uint8 HWC -> fp32 CHW in [0,1], bicubic-resized: b / 255 correctly rounded, then the cubic of
//                         image_sample.h in resize_bicubic_kernel's operation order, every step fused; one thread per output
//                         pixel forms the taps and weights once for the three channels
//   onehot_kernel         index map + 256-entry channel table -> (C,H,W) fp32 one-hot; four pixels per thread
//   pack_lut_kernel       int64 index maps -> uint8 object ids through a table (map_mask fused with pack_u8); 16 per thread;
//                         a table of up to 32 ids is four 64-bit words in registers, a longer one is read from the arguments
//   overlay_min_kernel /  add_overlay's sequential loop over object ids as a per-pixel closed form; the
//   overlay_kernel        pre-pass finds each frame's smallest label, which the loop's `ids[1:]` skips
// The 256-entry tables travel in the launch itself (kernel arguments by value): no device allocation, no copy to wait for.
// The only LDS is the four words that join a block's wave minima in overlay_min_kernel.
#include "common.h"
#include "image_sample.h"
#include "../../include/swem_hip_io.h"

namespace {

struct Table256 {
  unsigned char v[256];
};
struct Palette {
  unsigned char rgb[768];
};

// src [T][Hi][Wi][3] uint8 -> dst [T][3][Ho][Wo] fp32
__global__ __launch_bounds__(256) void stage_frames_kernel(const unsigned char *__restrict__ src, float *__restrict__ dst,
                                                           int T, int Hi, int Wi, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long plane = (long long)Ho * Wo;
  if (i >= (long long)T * plane) return;
  const int ox = (int)(i % Wo);
  const long long r = i / Wo;
  const int oy = (int)(r % Ho);
  const long long t = r / Ho;
  const unsigned char *img = src + t * Hi * Wi * 3;
  const float sy = (float)Hi / (float)Ho * (oy + 0.5f) - 0.5f, sx = (float)Wi / (float)Wo * (ox + 0.5f) - 0.5f;
  const float fy = floorf(sy), fx = floorf(sx);
  float wy[4], wx[4], acc[3];
  cubic_weights(sy - fy, wy);
  cubic_weights(sx - fx, wx);
  cubic_accumulate<3, 0>((int)fx, (int)fy, Wi, Hi, wx, wy, [&](int yy, int xx, float v[3]) {
    const unsigned char *p = img + (long long)yy * Wi * 3 + xx * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn((float)p[c], 255.0f);
  }, acc);
  float *o = dst + t * 3 * plane + (long long)oy * Wo + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c * plane] = acc[c];
}

// lab [n] uint8, out [C][n] fp32: out[c][i] = (chan[lab[i]] == c).  VEC: lab is 4-byte aligned, out 16-byte aligned, n % 4 == 0
// (every channel plane then starts aligned); otherwise everything goes the scalar way.
template <bool VEC>
__global__ __launch_bounds__(256) void onehot_kernel(const unsigned char *__restrict__ lab, float *__restrict__ out,
                                                     const Table256 chan, int C, long long n) {
  const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= n) return;
  if (VEC) {
    const unsigned w = *reinterpret_cast<const unsigned *>(lab + i0);
    const int c0 = chan.v[w & 0xff], c1 = chan.v[(w >> 8) & 0xff], c2 = chan.v[(w >> 16) & 0xff], c3 = chan.v[w >> 24];
    for (int c = 0; c < C; ++c)
      *reinterpret_cast<float4 *>(out + (long long)c * n + i0) =
          make_float4(c0 == c ? 1.f : 0.f, c1 == c ? 1.f : 0.f, c2 == c ? 1.f : 0.f, c3 == c ? 1.f : 0.f);
  } else {
    const long long i1 = i0 + 4 < n ? i0 + 4 : n;
    for (long long i = i0; i < i1; ++i) {
      const int ci = chan.v[lab[i]];
      for (int c = 0; c < C; ++c) out[(long long)c * n + i] = ci == c ? 1.f : 0.f;
    }
  }
}

// basic_evaluator.py:202-206 fused with pack_u8_kernel: y[i] = ids[x[i]], 0 where x[i] is outside the table
// Both lookups are branch-free (an index outside the table reads entry 0 and is masked to 0), so that the sixteen loads of x
// are issued together and nothing waits between them.
__device__ __forceinline__ unsigned lut_id(const Table256 &ids, int n_ids, long long idx) {
  const bool ok = (unsigned long long)idx < (unsigned long long)n_ids;
  return ids.v[ok ? (unsigned)idx : 0u] & (ok ? 0xffu : 0u);
}
// up to 32 ids (every real sequence: YouTube-VOS has at most a handful of objects) as four 64-bit words that stay in scalar
// registers: the lookup is three selects and a shift, no load behind the load of x.  Entries from n_ids on are zero.
struct Table32 {
  unsigned long long w[4];
};
__device__ __forceinline__ unsigned lut_id(const Table32 &ids, int, long long idx) {
  const unsigned i = (unsigned)idx;
  const unsigned long long lo = (i & 8u) ? ids.w[1] : ids.w[0], hi = (i & 8u) ? ids.w[3] : ids.w[2];
  const unsigned long long w = (i & 16u) ? hi : lo;
  const unsigned ok = (unsigned long long)idx < 32ull ? 0xffu : 0u;
  return (unsigned)(w >> ((i & 7u) * 8u)) & ok;
}
template <class Table>
__global__ __launch_bounds__(256) void pack_lut_kernel(const long long *__restrict__ x, unsigned char *__restrict__ y,
                                                       long long n, const Table ids, int n_ids) {
  const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (i0 >= n) return;
  if (i0 + 16 <= n) {
    long long v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = x[i0 + k];
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k >> 2] |= lut_id(ids, n_ids, v[k]) << (8 * (k & 3));
    *reinterpret_cast<uint4 *>(y + i0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    for (long long i = i0; i < n; ++i) y[i] = (unsigned char)lut_id(ids, n_ids, x[i]);
  }
}

// The smallest label of every frame (np.unique(mask)[0], visualization.py:47,54) into smin[t] (preset to 0xffffffff).
// grid (blocks per frame, T); VEC: frame starts are 4-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void overlay_min_kernel(const unsigned char *__restrict__ lab, unsigned *__restrict__ smin,
                                                          long long hw) {
  __shared__ unsigned red[4];
  const unsigned char *f = lab + (long long)blockIdx.y * hw;
  const long long stride = (long long)gridDim.x * 256 * 4;
  unsigned m = 0xffu;
  for (long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i0 < hw; i0 += stride) {
    if (VEC && i0 + 4 <= hw) {
      const unsigned w = *reinterpret_cast<const unsigned *>(f + i0);
      m = min(min(m, w & 0xff), min((w >> 8) & 0xff, min((w >> 16) & 0xff, w >> 24)));
    } else {
      const long long i1 = i0 + 4 < hw ? i0 + 4 : hw;
      for (long long i = i0; i < i1; ++i) m = min(m, (unsigned)f[i]);
    }
  }
  for (int off = 32; off > 0; off >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMin(smin + blockIdx.y, min(min(red[0], red[1]), min(red[2], red[3])));
}

// visualization.py:46-64 per pixel.  S = the frame's labels without the smallest; M = the largest label
// of S, other than the pixel's own L, among the four edge neighbours inside the image.
//   L in S and L > M (or no M)  -> trunc(img * alpha + (1 - alpha) * palette[L])   float64, every product and the sum rounded
//   else, M exists              -> 0                                                (the contour of object M)
//   else                        -> img
__device__ __forceinline__ int overlay_m(const unsigned char *__restrict__ f, int y, int x, int H, int W, int L, int s0) {
  int M = -1;
  const long long p = (long long)y * W + x;
  if (x > 0) {
    const int v = f[p - 1];
    if (v != L && v != s0) M = max(M, v);
  }
  if (x < W - 1) {
    const int v = f[p + 1];
    if (v != L && v != s0) M = max(M, v);
  }
  if (y > 0) {
    const int v = f[p - W];
    if (v != L && v != s0) M = max(M, v);
  }
  if (y < H - 1) {
    const int v = f[p + W];
    if (v != L && v != s0) M = max(M, v);
  }
  return M;
}
__device__ __forceinline__ unsigned overlay_blend(unsigned b, unsigned c, double alpha, double one_minus_alpha) {
  // numpy rounds both products and the sum.  hipcc contracts a * b + c into an fma by default, and HIP's __dmul_rn / __dadd_rn
  // are plain operators that it contracts just the same: contraction is switched off for this function
#pragma clang fp contract(off)
  const double from_img = (double)b * alpha;
  const double from_colour = one_minus_alpha * (double)c;
  return (unsigned)(int)(from_img + from_colour);
}
// 4 pixels (12 bytes of RGB) per thread; grid (blocks per frame, T).  VEC: frame starts of img / out / lab are 4-byte aligned,
// so that the label word and the three RGB words of a group are aligned loads and stores.
template <bool VEC>
__global__ __launch_bounds__(256) void overlay_kernel(const unsigned char *__restrict__ img, const unsigned char *__restrict__ lab,
                                                      const unsigned *__restrict__ smin, unsigned char *__restrict__ out,
                                                      const Palette pal, double alpha, double one_minus_alpha, int H, int W) {
  const long long hw = (long long)H * W;
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= hw) return;
  const long long t = blockIdx.y;
  const unsigned char *f = lab + t * hw;
  const unsigned char *src = img + t * hw * 3;
  unsigned char *dst = out + t * hw * 3;
  const int s0 = (int)smin[t];
  const int cnt = (int)(hw - p0 < 4 ? hw - p0 : 4);
  // the group lives in four words (labels, then RGB bytes 0..11, little-endian): constant shifts only, so it stays in registers
  unsigned lw = 0, w[3] = {0, 0, 0};
  if (VEC && cnt == 4) {
    lw = *reinterpret_cast<const unsigned *>(f + p0);
    const unsigned *s = reinterpret_cast<const unsigned *>(src + p0 * 3);
    w[0] = s[0];
    w[1] = s[1];
    w[2] = s[2];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) lw |= (unsigned)f[p0 + j] << (8 * j);
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < cnt * 3) w[k >> 2] |= (unsigned)src[p0 * 3 + k] << (8 * (k & 3));
  }
  int y = (int)(p0 / W), x = (int)(p0 - (long long)y * W);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < cnt) {
      const int L = (int)((lw >> (8 * j)) & 0xff);
      const int M = overlay_m(f, y, x, H, W, L, s0);
      const bool blend = L != s0 && L > M;
      if (blend || M >= 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int k = j * 3 + c, sh = 8 * (k & 3);
          const unsigned v = blend ? overlay_blend((w[k >> 2] >> sh) & 0xff, pal.rgb[L * 3 + c], alpha, one_minus_alpha) : 0u;
          w[k >> 2] = (w[k >> 2] & ~(0xffu << sh)) | ((v & 0xff) << sh);
        }
      }
      if (++x == W) {
        x = 0;
        ++y;
      }
    }
  }
  if (VEC && cnt == 4) {
    unsigned *d = reinterpret_cast<unsigned *>(dst + p0 * 3);
    d[0] = w[0];
    d[1] = w[1];
    d[2] = w[2];
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < cnt * 3) dst[p0 * 3 + k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
  }
}

inline bool aligned_to(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace

#define ST static_cast<hipStream_t>(stream)

extern "C" int swem_stage_frames_u8(void *stream, const unsigned char *src, float *dst, int T, int Hs, int Ws, int Ho, int Wo) {
  SWEM_REQUIRE(src && dst, SWEM_E_ARG, "stage_frames: null pointer");
  SWEM_REQUIRE(T > 0 && Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, SWEM_E_SHAPE,
               "stage_frames: need T, Hs, Ws, Ho, Wo > 0, got T=%d %dx%d -> %dx%d", T, Hs, Ws, Ho, Wo);
  const long long n = (long long)T * Ho * Wo;
  SWEM_REQUIRE((n + 255) / 256 <= 0x7fffffffLL && (long long)Hs * Ws <= 0x7fffffffLL / 3, SWEM_E_SHAPE,
               "stage_frames: %lld output pixels / a %dx%d source exceed one launch", n, Hs, Ws);
  hipLaunchKernelGGL(stage_frames_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, src, dst, T, Hs, Ws, Ho, Wo);
  SWEM_CHECK_LAUNCH("stage_frames");
  return SWEM_OK;
}

extern "C" int swem_labels_onehot_u8(void *stream, const unsigned char *lab, const unsigned char *chan256, float *out, int C,
                                     int H, int W) {
  SWEM_REQUIRE(lab && chan256 && out, SWEM_E_ARG, "labels_onehot: null pointer");
  SWEM_REQUIRE(aligned_to(out, 4), SWEM_E_ARG, "labels_onehot: out must be 4-byte aligned");
  SWEM_REQUIRE(C >= 1 && C <= 255 && H > 0 && W > 0, SWEM_E_SHAPE,
               "labels_onehot: need 1 <= C <= 255 channels (255 = no channel) and H, W > 0, got C=%d %dx%d", C, H, W);
  Table256 tab;
  __builtin_memcpy(tab.v, chan256, 256);
  const long long n = (long long)H * W;
  const dim3 grid((unsigned)((n + 1023) / 1024));
  if (n % 4 == 0 && aligned_to(lab, 4) && aligned_to(out, 16))
    hipLaunchKernelGGL(onehot_kernel<true>, grid, dim3(256), 0, ST, lab, out, tab, C, n);
  else
    hipLaunchKernelGGL(onehot_kernel<false>, grid, dim3(256), 0, ST, lab, out, tab, C, n);
  SWEM_CHECK_LAUNCH("labels_onehot");
  return SWEM_OK;
}

extern "C" int swem_pack_u8_lut_i64(void *stream, const long long *x, unsigned char *y, long long n, const unsigned char *ids,
                                    int n_ids) {
  SWEM_REQUIRE(x && y && ids, SWEM_E_ARG, "pack_u8_lut: null pointer");
  SWEM_REQUIRE(aligned_to(y, 16) && aligned_to(x, 8), SWEM_E_ARG, "pack_u8_lut: y must be 16-byte aligned, x 8-byte aligned");
  SWEM_REQUIRE(n > 0 && n_ids >= 1 && n_ids <= 256 && (n + 4095) / 4096 <= 0x7fffffffLL, SWEM_E_SHAPE,
               "pack_u8_lut: need n > 0 and a table of 1..256 object ids, got n=%lld n_ids=%d", n, n_ids);
  Table256 tab;
  __builtin_memset(tab.v, 0, 256);
  __builtin_memcpy(tab.v, ids, (size_t)n_ids);
  const dim3 grid((unsigned)((n + 4095) / 4096));
  if (n_ids <= 32) {
    Table32 small;
    __builtin_memcpy(small.w, tab.v, sizeof(small.w));   // (little-endian: byte k of word j is entry 8 * j + k)
    hipLaunchKernelGGL(pack_lut_kernel<Table32>, grid, dim3(256), 0, ST, x, y, n, small, n_ids);
  } else {
    hipLaunchKernelGGL(pack_lut_kernel<Table256>, grid, dim3(256), 0, ST, x, y, n, tab, n_ids);
  }
  SWEM_CHECK_LAUNCH("pack_u8_lut");
  return SWEM_OK;
}

extern "C" size_t swem_overlay_workspace(int T) { return T > 0 ? (size_t)T * sizeof(unsigned) : 0; }

extern "C" int swem_overlay_u8(void *stream, const unsigned char *frames, const unsigned char *labels,
                               const unsigned char *palette768, double alpha, double one_minus_alpha, unsigned char *out, int T,
                               int H, int W, void *ws, size_t ws_bytes) {
  SWEM_REQUIRE(frames && labels && palette768 && out && ws, SWEM_E_ARG, "overlay: null pointer");
  SWEM_REQUIRE(aligned_to(ws, 4), SWEM_E_ARG, "overlay: ws must be 4-byte aligned");
  SWEM_REQUIRE(alpha >= 0.0 && alpha <= 1.0 && one_minus_alpha >= 0.0 && one_minus_alpha <= 1.0 &&
                   alpha + one_minus_alpha <= 1.0 + 1e-12,
               SWEM_E_ARG, "overlay: need alpha and 1 - alpha in [0, 1] (the blended byte must stay a byte)");
  SWEM_REQUIRE(T > 0 && T <= 65535 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL / 3, SWEM_E_SHAPE,
               "overlay: need 1 <= T <= 65535 and H, W > 0, got T=%d %dx%d", T, H, W);
  SWEM_REQUIRE(ws_bytes >= swem_overlay_workspace(T), SWEM_E_WORKSPACE, "overlay: workspace %zu < %zu bytes", ws_bytes,
               swem_overlay_workspace(T));
  hipError_t e = hipMemsetAsync(ws, 0xff, (size_t)T * sizeof(unsigned), ST);
  if (e != hipSuccess) {
    swem_set_error("overlay: hipMemsetAsync: %s", hipGetErrorString(e));
    return SWEM_E_HIP;
  }
  const long long hw = (long long)H * W;
  const bool vec = (T == 1 || hw % 4 == 0) && aligned_to(frames, 4) && aligned_to(labels, 4) && aligned_to(out, 4);
  Palette pal;
  __builtin_memcpy(pal.rgb, palette768, 768);
  unsigned *smin = static_cast<unsigned *>(ws);
  const long long groups = (hw + 1023) / 1024;
  const dim3 gmin((unsigned)(groups < 64 ? groups : 64), (unsigned)T), grid((unsigned)groups, (unsigned)T);
  if (vec) {
    hipLaunchKernelGGL(overlay_min_kernel<true>, gmin, dim3(256), 0, ST, labels, smin, hw);
    SWEM_CHECK_LAUNCH("overlay_min");
    hipLaunchKernelGGL(overlay_kernel<true>, grid, dim3(256), 0, ST, frames, labels, smin, out, pal, alpha, one_minus_alpha, H, W);
  } else {
    hipLaunchKernelGGL(overlay_min_kernel<false>, gmin, dim3(256), 0, ST, labels, smin, hw);
    SWEM_CHECK_LAUNCH("overlay_min");
    hipLaunchKernelGGL(overlay_kernel<false>, grid, dim3(256), 0, ST, frames, labels, smin, out, pal, alpha, one_minus_alpha, H, W);
  }
  SWEM_CHECK_LAUNCH("overlay");
  return SWEM_OK;
}
