/*
 * swem_hip_io.h -- C ABI of libswem_hip.so, evaluation staging part: decoded bytes in, result bytes out (csrc/stage.hip).
 * Conventions, error codes and swem_last_error(): swem_hip.h.
 *
 * The reference's evaluation loop does this work on the host, a frame at a time: its dataset classes turn every decoded JPEG
 * into fp32 (datasets/data_utils.py:96-116) and every annotation into a one-hot float tensor (datasets/DAVIS_Test.py:40-49,
 * datasets/YTVOS_Test.py:116-132), its evaluator maps the predicted indices back to object ids one id at a time
 * (methods/basic_modules/basic_evaluator.py:202-206) and, under VAL.VISUALIZE, blends overlay pictures with numpy and scipy
 * (utils/visualization.py:46-72).  Here the bytes a decoder produced are uploaded as they are and four pointwise kernels do the
 * rest.  Every entry point checks its arguments before any HIP call, takes the stream, never synchronises, allocates nothing
 * and can be captured into a graph.  Tables (256 channel numbers, object ids, a 256x3 palette) are HOST pointers: they are
 * copied into the launch by value.
 */
#ifndef SWEM_HIP_IO_H
#define SWEM_HIP_IO_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWEM_IO_NO_CHANNEL 255 /* chan256[label] of a label that belongs to no channel */

/* data_utils.py:102 (`np.array(img, float32) / 255.0`), ToTensor's HWC -> CHW and basic_evaluator.py:160
 * (F.interpolate(..., mode='bicubic', align_corners=False)) in one pass; with Ho x Wo = the YouTube-VOS input size also
 * data_utils.py:105 (cv2.resize INTER_CUBIC; DESIGN.md section 10 on the two conventions).
 *   src : [T][Hs][Ws][3] uint8 RGB, interleaved (device; any width, no alignment assumed)
 *   dst : [T][3][Ho][Wo] fp32 (device)
 * Every sample is b / 255.0f correctly rounded; the resize is ATen's upsample_bicubic2d (A = -0.75, unclamped source
 * coordinate, 4x4 taps clamped to the image) in the operation order of swem_resize_planes_f32. */
int swem_stage_frames_u8(void *stream, const unsigned char *src, float *dst, int T, int Hs, int Ws, int Ho, int Wo);

/* The one-hot annotation of both datasets from one table: out[c][y][x] = (chan256[lab[y][x]] == c).
 *   DAVIS_Test.py:43-48 -> data_utils.py:141-186 (to_onehot_tensor, shuffle=False): channels 1.. = the ids present, ascending and
 *     compacted; every other label -> channel 0 (its background is "1 - sum"); single_obj: every label > 1 -> channel 1
 *   YTVOS_Test.py:124-130: label 0 -> channel 0, the frame's new ids -> channels 1.. in list order, every other label (an
 *     object annotated earlier) -> SWEM_IO_NO_CHANNEL: all-zero across the channels
 *   lab : [H][W] uint8 (device)     chan256 : 256 uint8 (HOST)     out : [C][H][W] fp32 (device), 1 <= C <= 255 */
int swem_labels_onehot_u8(void *stream, const unsigned char *lab, const unsigned char *chan256, float *out, int C, int H, int W);

/* basic_evaluator.py:202-206 (map_mask) fused with swem_pack_u8_i64 (:177): y[i] = ids[x[i]], 0 where x[i] is not in 0..n_ids-1.
 *   x : [n] int64 index maps (device)   y : [n] uint8 (device, 16-byte aligned)   ids : n_ids uint8 object ids (HOST), 1..256 */
int swem_pack_u8_lut_i64(void *stream, const long long *x, unsigned char *y, long long n, const unsigned char *ids, int n_ids);

/* visualization.py:46-72 (add_overlay as save_overlay calls it) for T frames at once: the sequential loop over the object ids
 * as a per-pixel closed form, RGB in and RGB out (the reference blends BGR with the reversed colour and
 * cv2.imwrite swaps back: the same picture).
 *   frames  : [T][H][W][3] uint8 RGB (device)        labels : [T][H][W] uint8 index maps (device)
 *   palette768 : 256 x 3 uint8 RGB (HOST)            out    : [T][H][W][3] uint8 RGB (device; not `frames`)
 *   alpha, one_minus_alpha : float64, the second computed by the caller as 1 - alpha in float64 (visualization.py:49); the
 *             blend trunc(img * alpha + one_minus_alpha * colour) is float64 with every product and the sum rounded
 *   ws      : swem_overlay_workspace(T) bytes, 4-byte aligned: each frame's smallest label (the loop's ids[1:] skips it)
 * memset + two launches. */
size_t swem_overlay_workspace(int T);
int swem_overlay_u8(void *stream, const unsigned char *frames, const unsigned char *labels, const unsigned char *palette768,
                    double alpha, double one_minus_alpha, unsigned char *out, int T, int H, int W, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SWEM_HIP_IO_H */
