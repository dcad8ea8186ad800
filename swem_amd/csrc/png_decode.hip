// PNG files decoded on the device (include/swem_hip_io.h): T files in, T pixel slots out, the inverse of
// png.hip.
//   png_decode_kernel   one wavefront per file, all files of a call in one launch.  Everything a file goes through is
//                       pngd_decode_file of csrc/inflate_core.h: the chunk walk (CRC-32 by the 64 lanes over pieces, joined with
//                       the x^(8n) combine), the IDAT payloads compacted into the workspace, inflate (tables in LDS; every lane
//                       decodes the symbols redundantly, so the control flow is wave-uniform; lane 0 stores a literal, all
//                       lanes copy a match out of a 64 KiB ring in LDS; the ring is flushed to the workspace 32 KiB at a time),
//                       Adler-32 from the lanes' piece sums, the unfilter in place (types 0 and 2 along the row, type 1 as a
//                       prefix sum, types 3 and 4 by lane 0 over tiles in LDS), the palette index check and the unpack.
// What this file adds is the wavefront: one lane per thread, and a fence and a barrier where a lane reads what another stored.
#include "common.h"
#include "../../include/swem_hip_io.h"
#include "inflate_core.h"

namespace {

static_assert(PNGD_OK == SWEM_PNG_ST_OK && PNGD_OFFSETS == SWEM_PNG_ST_OFFSETS && PNGD_SIGNATURE == SWEM_PNG_ST_SIGNATURE &&
                  PNGD_CHUNK == SWEM_PNG_ST_CHUNK && PNGD_CRC == SWEM_PNG_ST_CRC && PNGD_IHDR == SWEM_PNG_ST_IHDR &&
                  PNGD_DIMENSIONS == SWEM_PNG_ST_DIMENSIONS && PNGD_UNSUPPORTED == SWEM_PNG_ST_UNSUPPORTED &&
                  PNGD_METHOD == SWEM_PNG_ST_METHOD && PNGD_PLTE == SWEM_PNG_ST_PLTE && PNGD_IDAT == SWEM_PNG_ST_IDAT &&
                  PNGD_CRITICAL == SWEM_PNG_ST_CRITICAL && PNGD_IEND == SWEM_PNG_ST_IEND && PNGD_TRAILING == SWEM_PNG_ST_TRAILING &&
                  PNGD_TOO_LARGE == SWEM_PNG_ST_TOO_LARGE && PNGD_ZLIB_CM == SWEM_PNG_ST_ZLIB_CM &&
                  PNGD_ZLIB_CINFO == SWEM_PNG_ST_ZLIB_CINFO && PNGD_ZLIB_FCHECK == SWEM_PNG_ST_ZLIB_FCHECK &&
                  PNGD_ZLIB_FDICT == SWEM_PNG_ST_ZLIB_FDICT && PNGD_BLOCK_TYPE == SWEM_PNG_ST_BLOCK_TYPE &&
                  PNGD_STORED_LEN == SWEM_PNG_ST_STORED_LEN && PNGD_HLIT_HDIST == SWEM_PNG_ST_HLIT_HDIST &&
                  PNGD_REPEAT == SWEM_PNG_ST_REPEAT && PNGD_OVERSUBSCRIBED == SWEM_PNG_ST_OVERSUBSCRIBED &&
                  PNGD_INCOMPLETE == SWEM_PNG_ST_INCOMPLETE && PNGD_NO_EOB == SWEM_PNG_ST_NO_EOB &&
                  PNGD_BAD_SYMBOL == SWEM_PNG_ST_BAD_SYMBOL && PNGD_DISTANCE == SWEM_PNG_ST_DISTANCE &&
                  PNGD_NO_FINAL == SWEM_PNG_ST_NO_FINAL && PNGD_TRUNCATED == SWEM_PNG_ST_TRUNCATED &&
                  PNGD_IDAT_LEFT == SWEM_PNG_ST_IDAT_LEFT && PNGD_LENGTH == SWEM_PNG_ST_LENGTH && PNGD_ADLER == SWEM_PNG_ST_ADLER &&
                  PNGD_FILTER == SWEM_PNG_ST_FILTER && PNGD_INDEX == SWEM_PNG_ST_INDEX,
              "inflate_core.h and swem_hip_io.h name the same status words");

// the joins of inflate_core.h for one wavefront: a thread is one lane; what a lane stored (LDS or workspace) is ordered before
// what another lane of the block loads by a workgroup-scope fence either side of the barrier
struct PngdWavefront {
  __host__ __device__ __forceinline__ int lane_begin() const {
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)threadIdx.x;
#else
    return 0;
#endif
  }
  __host__ __device__ __forceinline__ int lane_end() const { return lane_begin() + 1; }
  __host__ __device__ __forceinline__ bool first() const { return lane_begin() == 0; }
  __host__ __device__ __forceinline__ void sync() const {
#if defined(__HIP_DEVICE_COMPILE__)
    __threadfence_block();
    __syncthreads();
    __threadfence_block();
#endif
  }
};

__global__ __launch_bounds__(64) void png_decode_kernel(const unsigned char *__restrict__ blob, size_t blob_bytes,
                                                        const long long *__restrict__ offsets, int Hs, int Ws, int channels,
                                                        unsigned char *__restrict__ pixels, int *__restrict__ sizes,
                                                        unsigned char *__restrict__ palettes, int *__restrict__ n_palette,
                                                        int *__restrict__ status, unsigned char *__restrict__ comp_ws,
                                                        unsigned char *__restrict__ raw_ws, size_t raw_stride) {
  extern __shared__ __align__(16) unsigned char lds[];
  PngdLds *S = reinterpret_cast<PngdLds *>(lds);
  const size_t t = blockIdx.x;
  const PngdWavefront wv;
  pngd_decode_file(wv, S, blob, blob_bytes, offsets[t], offsets[t + 1], Hs, Ws, channels,
                   pixels + t * (size_t)Hs * (size_t)Ws * (size_t)channels, sizes + 2 * t, palettes ? palettes + 768 * t : nullptr,
                   n_palette ? n_palette + t : nullptr, status + t, comp_ws, raw_ws + t * raw_stride, (uint32_t)raw_stride);
}

inline bool pngd_aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }
inline bool pngd_shape_ok(int T, int Hs, int Ws, int channels) {
  return T >= 1 && T <= 65535 && (channels == 1 || channels == 3) && Hs >= 1 && Ws >= 1 && (long long)channels * Ws + 1 <= 65535 &&
         (long long)Hs * ((long long)channels * Ws + 1) < 0x80000000ll;
}
inline size_t pngd_raw_stride(int Hs, int Ws, int channels) { return align_up((size_t)Hs * ((size_t)channels * Ws + 1), 16); }

}  // namespace

#define ST static_cast<hipStream_t>(stream)

extern "C" size_t swem_png_decode_workspace(int T, int Hs, int Ws, int channels, size_t blob_bytes) {
  if (!pngd_shape_ok(T, Hs, Ws, channels) || blob_bytes < 1) return 0;
  return align_up(blob_bytes, 16) + (size_t)T * pngd_raw_stride(Hs, Ws, channels);
}

extern "C" int swem_png_decode_u8(void *stream, const unsigned char *blob, size_t blob_bytes, const long long *offsets, int T,
                                  int Hs, int Ws, int channels, unsigned char *pixels, int *sizes, unsigned char *palettes,
                                  int *n_palette, int *status, void *ws, size_t ws_bytes) {
  SWEM_REQUIRE(blob && offsets && pixels && sizes && status && ws, SWEM_E_ARG, "png_decode: null pointer");
  SWEM_REQUIRE(pngd_aligned(ws, 16) && pngd_aligned(offsets, 8) && pngd_aligned(sizes, 4) && pngd_aligned(status, 4) &&
                   pngd_aligned(n_palette, 4),
               SWEM_E_ARG, "png_decode: ws must be 16-byte aligned, offsets 8-byte, sizes, status and n_palette 4-byte aligned");
  SWEM_REQUIRE(channels == 1 || channels == 3, SWEM_E_ARG, "png_decode: channels is 1 or 3, got %d", channels);
  SWEM_REQUIRE(T >= 1 && T <= 65535, SWEM_E_SHAPE, "png_decode: need 1 <= T <= 65535 files, got %d", T);
  SWEM_REQUIRE(pngd_shape_ok(T, Hs, Ws, channels), SWEM_E_SHAPE,
               "png_decode: need Hs >= 1, Ws >= 1, channels * Ws + 1 <= 65535 and a slot below 2 GiB, got %dx%d with %d channels", Hs,
               Ws, channels);
  SWEM_REQUIRE(blob_bytes >= 1, SWEM_E_SHAPE, "png_decode: an empty blob");
  const size_t need = swem_png_decode_workspace(T, Hs, Ws, channels, blob_bytes);
  SWEM_REQUIRE(ws_bytes >= need, SWEM_E_WORKSPACE, "png_decode: insufficient workspace: %zu < %zu bytes", ws_bytes, need);
  unsigned char *comp_ws = static_cast<unsigned char *>(ws);
  unsigned char *raw_ws = comp_ws + align_up(blob_bytes, 16);
  SWEM_ALLOW_LDS(png_decode_kernel, sizeof(PngdLds));
  hipLaunchKernelGGL(png_decode_kernel, dim3((unsigned)T), dim3(64), sizeof(PngdLds), ST, blob, blob_bytes, offsets, Hs, Ws,
                     channels, pixels, sizes, palettes, n_palette, status, comp_ws, raw_ws, pngd_raw_stride(Hs, Ws, channels));
  SWEM_CHECK_LAUNCH("png_decode");
  return SWEM_OK;
}
