// What the convolution kernels on the 16-bit matrix cores share (conv_igemm_bf3_kernel, conv_igemm_bf3s_kernel,
// conv_t256_kernel; the raw buffer loads serve conv_igemm_pipe_kernel too): MFMA wrappers, buffer loads, and the epilogue
// for 16x16 accumulator tiles.
#pragma once
#include "conv_common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 bufload4(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
constexpr unsigned OOB = 0xfffffff0u;  // >= any num_records: the load returns 0 and touches no memory

__device__ __forceinline__ f32x16 mfma_bf16(uint4 a, uint4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 bufload2(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0);
  return make_uint2(v.x, v.y);
}

typedef float f32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4v mfma_bf16_16(uint4 a, uint4 b, f32x4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// F16: the planes hold fp16 pairs (bf16_split.h, split2h) and the products run on the f16 MFMA of the same shape -- the
// "f16x3" arithmetic: three products on 23-bit operands, fp32-level error at the bf16x3 kernel's cost.
template <bool F16>
__device__ __forceinline__ f32x4v mm16(uint4 a, uint4 b, f32x4v c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return mfma_bf16_16(a, b, c);
}
template <bool F16>
__device__ __forceinline__ f32x16 mm32(uint4 a, uint4 b, f32x16 c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return mfma_bf16(a, b, c);
}
// Epilogue for 16x16 accumulator tiles (v_mfma_f32_16x16x32_bf16): lane l holds column l % 16 and rows 4 (l / 16) + e.
// Same semantics as conv_epilogue; a wave owns TM2 x TN2 tiles = 16 TM2 rows x 16 TN2 columns.
template <int TM2, int TN2>
__device__ __forceinline__ void conv_epilogue16(const ConvP &p, f32x4v (&acc)[TM2][TN2], int mrow0, int ncol0, int lane) {
  const int col = lane & 15, rg = lane >> 4;
  if (p.partial) {
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
  if constexpr (TN2 == 4) {
    if (p.flags & SWEM_CONV_GLU) {
      // packed columns [group][f|a][32]: tiles 0,1 are f, tiles 2,3 the gates of the same 32 channels; the gated values go
      // through the wave's LDS slice and out in row layout (16-byte stores, bf16 planes)
      static_assert(TM2 % 2 == 0, "the output staging works on 32 x 32 sub-tiles");
      const bool nin = ncol0 + 64 <= p.Ncols;
      float scf[2], sca[2], shf[2], sha[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nf = ncol0 + 16 * j + col, na = nf + 32;
        scf[j] = (nin && p.scale) ? p.scale[nf] : p.uscale; sca[j] = (nin && p.scale) ? p.scale[na] : p.uscale;
        shf[j] = (nin && p.shift) ? p.shift[nf] : 0.f; sha[j] = (nin && p.shift) ? p.shift[na] : 0.f;
      }
      __syncthreads();   // every wave is done with the operand stages
      unsigned *lds = planes_lds();
#pragma unroll
      for (int i0 = 0; i0 < TM2; i0 += 2) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              lds[(16 * ii + 4 * rg + e) * PL_STRIDE + 16 * j + col] = __float_as_uint(
                  (acc[i0 + ii][j][e] * scf[j] + shf[j]) * sigmoidf_(acc[i0 + ii][j + 2][e] * sca[j] + sha[j]));
        out_tile32(p, lds, mrow0 + 16 * i0, nin ? (ncol0 >> 1) : p.Cout);
      }
      return;
    }
  }
  // 32 x 32 sub-tiles (2 x 2 accumulator tiles) through the wave's LDS slice, out in row layout (out_tile32)
  static_assert(TM2 % 2 == 0 && TN2 % 2 == 0, "the output staging works on 32 x 32 sub-tiles");
  __syncthreads();   // every wave is done with the operand stages
  unsigned *lds = planes_lds();
#pragma unroll
  for (int j0 = 0; j0 < TN2; j0 += 2) {
    float sc[2], sh[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int n = ncol0 + 16 * (j0 + jj) + col;
      const bool nin = n < p.Ncols;
      sc[jj] = (nin && p.scale) ? p.scale[n] : p.uscale;
      sh[jj] = (nin && p.shift) ? p.shift[n] : 0.f;
    }
#pragma unroll
    for (int i0 = 0; i0 < TM2; i0 += 2) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            lds[(16 * ii + 4 * rg + e) * PL_STRIDE + 16 * jj + col] = __float_as_uint(acc[i0 + ii][j0 + jj][e] * sc[jj] + sh[jj]);
      out_tile32(p, lds, mrow0 + 16 * i0, ncol0 + 16 * j0);
    }
  }
}

}  // namespace
