/*
 * swem_hip_data.h -- C ABI of libswem_hip.so, training-data part: the augmentation of decoded training clips on the device
 * (csrc/augment.hip).  Conventions, error codes and swem_last_error(): swem_hip.h.
 *
 * The reference builds a clip on CPU workers (datasets/video_dataset.py:139-192, 269-344): per frame a PIL resized crop, a
 * PIL affine, two colour jitters, a random grayscale and a thin-plate-spline grid_sample, then label picking and one-hot masks.
 * Here the host only DRAWS the random numbers (swem_amd/augment.py); two kernels evaluate them on the decoded uint8 frames:
 * the geometry as ONE resample (TPS -> affine -> crop / flip composed per output pixel; DESIGN.md section 8 defines it and
 * states how it departs from the reference's three resamples), the colour chain as one pointwise pass behind one reduction,
 * the object choice from a 256-bit presence set.  Nothing synchronises with the host; memset + two launches, capturable.
 */
#ifndef SWEM_HIP_DATA_H
#define SWEM_HIP_DATA_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWEM_AUG_MAX_CHANNELS 8  /* N + 1 mask channels at the most (the lane of eight objects of the matching kernels) */
#define SWEM_AUG_FRAME_WORDS 64  /* 32-bit words of one frame's parameter record */
#define SWEM_AUG_CLIP_WORDS 256  /* 32-bit words of one clip's label order */
/* Parameter block of a call over B clips of T frames (device memory, 4-byte aligned):
 *   [B][T][SWEM_AUG_FRAME_WORDS] frame records, then [B][SWEM_AUG_CLIP_WORDS] int32 label orders.
 * Frame record (fp32 unless stated; (xc, yc) = (u + 0.5 - Wo/2, v + 0.5 - Ho/2) are CENTRED pixel-edge coordinates, so that the
 * products stay small in fp32):
 *    0.. 5  M_aff:  x' = m0*xc + m1*yc + m2,  y' = m3*xc + m4*yc + m5      (the pixel is FILL outside [0,Wo) x [0,Ho))
 *    6..11  M_src:  sx = s0*xc + s1*yc + s2,  sy = s3*xc + s4*yc + s5      (source pixel-edge coordinates)
 *   12..17  TPS affine part: q_x = a0 + a1*xn + a2*yn, q_y = a3 + a4*xn + a5*yn
 *   18..33  TPS W_k of q_x, 34..49 of q_y, k = 4*row + column of the 4x4 anchor grid on [-1,1]^2
 *   50..52  clip-level factors (brightness, contrast, saturation), 53..55 frame-level factors
 *   56      int32: TPS on (non-zero) / off       57  int32: order of the clip-level ops     58  int32: grayscale on / off
 *   59      int32: order of the frame-level ops  60..63  zero
 * An order is three 2-bit op codes, first op in bits 0-1: 0 brightness, 1 contrast, 2 saturation, 3 no op.
 * Label order: the 256 labels in the order of the clip's random priority (the inverse of the priority permutation). */
enum { SWEM_AUG_REGION_IMAGE = 0, SWEM_AUG_REGION_FILL = 1, SWEM_AUG_REGION_OUTSIDE_TPS = 2 };

/* Workspace of a call: [B][T][Ho][Wo] uint8 warped labels, [B][T][Ho][Wo] uint8 region codes, then (each 256-byte aligned)
 * [B][8] uint32 label presence bits of frame 0 and [B][T][tiles] fp32 gray partial sums, tiles = ceil(Wo/32) * ceil(Ho/8).
 * 0 for non-positive sizes. */
size_t swem_augment_workspace(int B, int T, int Ho, int Wo);

/* video_dataset.py:269-344 for B clips that share the source size.
 *   src    : [B][T][Hs][Ws][3] uint8 decoded frames (HWC, any width: no alignment is assumed)
 *   lab    : [B][T][Hs][Ws] uint8 label maps
 *   params : the block above
 *   frames : [B][T][3][Ho][Wo] fp32     masks : [B][T][N+1][Ho][Wo] fp32 one-hot     valid : [B][N+1] fp32
 *   label  : [B][T][Ho][Wo] int64 (the argmax of masks)       found : [B] int32, the labels found in frame 0 (0 and 255 apart)
 *            -- all five at the FIRST clip's slot: a call may fill clips b0..b1 of a larger batch
 *   N      : max objects, 1 <= N, N + 1 <= SWEM_AUG_MAX_CHANNELS;  Ho, Wo >= 2
 * Bitwise reproducible: the gray mean is a fixed-order sum of per-block partial sums in fixed slots, the presence set an
 * integer OR. */
int swem_augment_clips_u8(void *stream, const unsigned char *src, const unsigned char *lab, const void *params, float *frames,
                          float *masks, float *valid, long long *label, int *found, int B, int T, int Hs, int Ws, int Ho,
                          int Wo, int N, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SWEM_HIP_DATA_H */
