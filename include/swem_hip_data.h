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
 *   59      int32: order of the frame-level ops  60..63  zero (swem_augment_static_u8 reads them: below)
 * An order is three 2-bit op codes, first op in bits 0-1: 0 brightness, 1 contrast, 2 saturation, 3 no op.
 * Label order: the 256 labels in the order of the clip's random priority (the inverse of the priority permutation). */
enum { /* first word of each field of the frame record (words 60..63: swem_augment_static_u8, below) */
  SWEM_AUG_M_AFF = 0,
  SWEM_AUG_M_SRC = 6,
  SWEM_AUG_TPS_AFFINE = 12,
  SWEM_AUG_TPS_WX = 18,
  SWEM_AUG_TPS_WY = 34,
  SWEM_AUG_CLIP_FACTORS = 50,
  SWEM_AUG_FRAME_FACTORS = 53,
  SWEM_AUG_TPS_ON = 56,
  SWEM_AUG_CLIP_ORDER = 57,
  SWEM_AUG_GRAY = 58,
  SWEM_AUG_FRAME_ORDER = 59,
  SWEM_AUG_STATIC_FLAGS = 60,
  SWEM_AUG_SRC_H = 61,
  SWEM_AUG_SRC_W = 62,
  SWEM_AUG_HUE = 63
};
enum { /* word SWEM_AUG_STATIC_FLAGS: bit 0, and the 2-bit field in bits 4-5 */
  SWEM_AUG_FLAG_SRC_FILL = 1,
  SWEM_AUG_FLAG_HUE_BEFORE_SHIFT = 4,
  SWEM_AUG_FLAG_HUE_BEFORE_MASK = 3
};
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

/* ---- Stage-0 training clips from static images (datasets/static_dataset.py) ------------------------------
 *
 * synthesis_frames (static_dataset.py:82-147): the objects of n_img images with masks are cut out at their bounding boxes and
 * pasted, per frame at a drawn size and place and in a drawn order, onto image 0, whose own object is painted over with its
 * mean colour.  The host draws the numbers; the device measures the boxes (integer min / max / add on words a launch has cleared:
 * bitwise reproducible; a captured stage-0 call holds no memset node), evaluates random_resize /
 * place_object in float64 (one thread per clip, frame and object) and gathers every output pixel once: nearest mask and cubic
 * colour (A = -0.75) straight from the boxed source, no intermediate resize. */
#define SWEM_SYNTH_MAX_IMAGES 7   /* N images per clip at the most (N + 1 <= SWEM_AUG_MAX_CHANNELS) */
#define SWEM_SYNTH_CLIP_WORDS 32  /* 32-bit words of one clip's record */
#define SWEM_SYNTH_FRAME_WORDS 64 /* 32-bit words of one frame's record */
#define SWEM_SYNTH_STAT_WORDS 8   /* uint32 words of one image's statistics */
#define SWEM_SYNTH_PLAN_WORDS 8   /* int32 words of one (frame, object) placement */
/* Synth parameter block of a call over B clips of T frames (device memory, 4-byte aligned):
 *   [B][SWEM_SYNTH_CLIP_WORDS] clip records, then [B][T][SWEM_SYNTH_FRAME_WORDS] frame records.
 * Clip record (int32):
 *    0        n_img, the images in use (1 <= n_img <= N; the device clamps it to that range)
 *    2+2k     h_k,  3+2k  w_k: the real size of image k inside its slot, k < 7 (clamped to [1, Hmax] x [1, Wmax])
 *   16+k      the label id of object k (the low 8 bits are used)                       the other words: zero
 * Frame record:
 *    0..6     int32 paste order: word p names the object pasted p-th (later ones cover earlier ones); an entry outside
 *             [0, n_img) is skipped
 *    8+4k..   fp32 area, aspect, ux, uy of object k: area the fraction of the box area (random_resize's scale), aspect its
 *             width / height ratio, (ux, uy) in [0,1) the place (place_object's two randint draws)
 * Image statistics in the workspace, [B][N][SWEM_SYNTH_STAT_WORDS] uint32 (foreground = mask != 0):
 *    0  ~hmin   1  ~wmin   2  hmax + 1   3  wmax + 1  (all four built by integer max)   4  pixel count   5..7  sum of r, g, b
 * Placement table, [B][T][N][SWEM_SYNTH_PLAN_WORDS] int32:  rh, rw, tx, ty, id, present, 0, 0  with (hc, wc) the box size,
 *   rh = max(1, rint(sqrt(area hc wc / aspect))), rw = max(1, rint(sqrt(area hc wc aspect))),
 *   tx = lo + min(hi - lo, floor(ux (hi - lo + 1))) - rw/2,  lo = rw/2, hi = max(w0 - rw/2, rw/2)  (integer halves; y alike),
 *   present = 0 for k >= n_img and for an empty mask. */
enum { /* clip record, frame record: first word of each field */
  SWEM_SYNTH_N_IMG = 0,
  SWEM_SYNTH_SIZES = 2,
  SWEM_SYNTH_IDS = 16,
  SWEM_SYNTH_PASTE = 0,
  SWEM_SYNTH_OBJECTS = 8
};
enum { /* image statistics */
  SWEM_SYNTH_STAT_NOT_HMIN = 0,
  SWEM_SYNTH_STAT_NOT_WMIN = 1,
  SWEM_SYNTH_STAT_HMAX1 = 2,
  SWEM_SYNTH_STAT_WMAX1 = 3,
  SWEM_SYNTH_STAT_COUNT = 4,
  SWEM_SYNTH_STAT_SUM_R = 5,
  SWEM_SYNTH_STAT_SUM_G = 6,
  SWEM_SYNTH_STAT_SUM_B = 7
};
enum { /* placement */
  SWEM_SYNTH_PLAN_RH = 0,
  SWEM_SYNTH_PLAN_RW = 1,
  SWEM_SYNTH_PLAN_TX = 2,
  SWEM_SYNTH_PLAN_TY = 3,
  SWEM_SYNTH_PLAN_ID = 4,
  SWEM_SYNTH_PLAN_PRESENT = 5
};

/* Workspace of a call: the statistics, then (256-byte aligned) the placement table.  0 for non-positive sizes. */
size_t swem_synth_workspace(int B, int T, int N);

/*   imgs     : [B][N][Hmax][Wmax][3] uint8 (HWC), each image at the top left of its slot; bytes outside its real size are never read
 *   masks    : [B][N][Hmax][Wmax] uint8
 *   params   : the synth block above
 *   comp     : [B][T][Hmax][Wmax][3] uint8 composite frames, comp_lab : [B][T][Hmax][Wmax] uint8 labels -- both written at image
 *              0's size (h_0 x w_0) only; with n_img == 1 they are image 0 and its mask bytes
 *   1 <= N <= SWEM_SYNTH_MAX_IMAGES;  Hmax, Wmax <= 4096 (the uint32 colour sums hold 255 Hmax Wmax) */
int swem_synth_frames_u8(void *stream, const unsigned char *imgs, const unsigned char *masks, const void *params,
                         unsigned char *comp, unsigned char *comp_lab, int B, int T, int N, int Hmax, int Wmax, void *ws,
                         size_t ws_bytes);

/* The static chain (static_dataset.py:198-239) on composite frames: swem_augment_clips_u8 with words 60..63 of the frame record read:
 *   60  int32 flags: bit 0: a pixel whose (sx, sy) lies outside [0, ws) x [0, hs) is FILL (the second fill test);
 *                    bits 4-5: how many of the three clip-level ops run before the hue op
 *   61, 62  int32: the clip's source height hs and width ws inside the slot (taps and labels clamp to them); a value outside
 *           [1, Hs] / [1, Ws] means the call's Hs / Ws
 *   63  fp32: the clip-level hue shift (torchvision's tensor form: RGB -> HSV, h = fmod(h + shift + 1, 1), back); 0: no hue op
 * Hs, Ws are the slot size (the row and frame strides).  With words 60..63 zero the outputs are those of swem_augment_clips_u8,
 * bit for bit. */
int swem_augment_static_u8(void *stream, const unsigned char *src, const unsigned char *lab, const void *params, float *frames,
                           float *masks, float *valid, long long *label, int *found, int B, int T, int Hs, int Ws, int Ho,
                           int Wo, int N, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SWEM_HIP_DATA_H */
