// The project's cubic (ATen's upsample_bicubic2d: A = -0.75, align_corners=False) for every kernel that samples an image: the
// weights of a fraction, the tap clamp and the 4x4 accumulate of resize_bicubic_kernel (pointwise.hip), stage_frames_kernel
// (stage.hip), aug_warp_kernel (augment.hip) and synth_composite_kernel (synth.hip); and the launch that clears a few words.
// Device-only, everything with internal linkage.
//
// Every fused multiply-add is spelled fmaf and every pair that rounds twice goes through mul_then_add, so the arithmetic is the
// same under any contraction mode of the including unit (augment.hip pins `on`, the others take hipcc's default).  The products
// left bare feed an fmaf's multiplicand: there is no addition beside them that a contraction could take.
//
// The byte kernels fuse every step.  resize_bicubic_kernel does not: when it held its own loop, hipcc's vectoriser packed some of
// its one-float multiplies apart from their adds, and those roundings are its results since.  The two template arguments below
// (SPLIT_FIRST, UNFUSED_ROWS) write that down, so that its bits no longer hang on a compiler's choice; a change that is allowed
// to move them sets both to the byte kernels' values and deletes the arguments.
#ifndef SWEM_IMAGE_SAMPLE_H
#define SWEM_IMAGE_SAMPLE_H
#include <hip/hip_runtime.h>

// c + a * b in two roundings
static __device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
  return c + a * b;
}

// A = -0.75 folded: (A + 2, A + 3) = (1.25, 2.25), (A, -5A, 8A, -4A) = (-0.75, 3.75, -6, 3), all exact in fp32
static __device__ __forceinline__ float cubic_near(float x) { return fmaf(fmaf(1.25f, x, -2.25f) * x, x, 1.f); }   // |x| <= 1
template <bool SPLIT>                                                                                            // 1 < |x| < 2
static __device__ __forceinline__ float cubic_far(float x) {
  const float u = fmaf(-0.75f, x, 3.75f);
  return fmaf(SPLIT ? mul_then_add(u, x, -6.f) : fmaf(u, x, -6.f), x, 3.f);
}

// the weights of taps floor(s) - 1 .. floor(s) + 2 for t = s - floor(s); SPLIT_FIRST: resize_bicubic_kernel's y weights (above)
template <bool SPLIT_FIRST = false>
static __device__ __forceinline__ void cubic_weights(float t, float w[4]) {
  w[0] = cubic_far<SPLIT_FIRST>(t + 1.f);
  w[1] = cubic_near(t);
  w[2] = cubic_near(1.f - t);
  w[3] = cubic_far<false>(2.f - t);
}

static __device__ __forceinline__ int clamp_tap(int i, int n) { return min(max(i, 0), n - 1); }

// acc[c] = sum_a wy[a] * (sum_q wx[q] * v(a, q)[c]): for each row the x-weighted sum from zero, then the y-weighted sum of the
// rows from zero, taps in ascending order.  The taps are (ix - 1 .., iy - 1 ..) clamped to the box [0, w) x [0, h);
// tap(yy, xx, v) loads the C values of box pixel (yy, xx), already converted to float.
// Every step is one fmaf, except the x-sums of the first UNFUSED_ROWS rows, which round the product and the sum separately
// (resize_bicubic_kernel: 3, above).
template <int C, int UNFUSED_ROWS, class Tap>
static __device__ __forceinline__ void cubic_accumulate(int ix, int iy, int w, int h, const float wx[4], const float wy[4], Tap tap,
                                                        float acc[C]) {
  int xx[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) xx[q] = clamp_tap(ix - 1 + q, w);
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int yy = clamp_tap(iy - 1 + a, h);
    float row[C];
#pragma unroll
    for (int c = 0; c < C; ++c) row[c] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[C];
      tap(yy, xx[q], v);
#pragma unroll
      for (int c = 0; c < C; ++c) row[c] = a < UNFUSED_ROWS ? mul_then_add(wx[q], v[c], row[c]) : fmaf(wx[q], v[c], row[c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = fmaf(wy[a], row[c], acc[c]);
  }
}

// three HWC bytes at p as floats (the caller scales or rounds after the sum)
static __device__ __forceinline__ void rgb_bytes(const unsigned char *p, float v[3]) {
  v[0] = (float)p[0];
  v[1] = (float)p[1];
  v[2] = (float)p[2];
}

// words[0..n) = 0 as a launch (where a captured call must not hold a memset node: DESIGN.md section 9)
static __global__ __launch_bounds__(256) void clear_words_kernel(unsigned *__restrict__ words, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) words[i] = 0u;
}

#endif  // SWEM_IMAGE_SAMPLE_H
