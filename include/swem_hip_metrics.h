/*
 * swem_hip_metrics.h -- C ABI of libswem_hip.so, validation part: the DAVIS J&F scores of a whole sequence computed on
 * the device from the index maps the evaluator holds there (csrc/metrics.hip).  Conventions, error codes and
 * swem_last_error(): swem_hip.h.
 *
 * The reference scores on the host, one frame and object at a time (methods/basic_modules/basic_evaluator.py:271-328 ->
 * evaluation/davis2017/evaluation.py:47-60, 265-322 -> evaluation/davis2017/metrics.py:6-178: numpy sums for J,
 * cv2.dilate of the two boundary maps with a disk for F).  Here the maps never leave the device: only six integers per
 * frame and object do, and the host forms J and F from them with the reference's own float64 expressions
 * (swem_amd.metrics.jf_from_counts) -- equal integers give bit-equal scores.
 */
#ifndef SWEM_HIP_METRICS_H
#define SWEM_HIP_METRICS_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWEM_JF_MAX_RADIUS 64 /* the dilation works on (left, centre, right) 64-pixel words: a disk reaches one word */
#define SWEM_JF_COUNTS 6      /* integers per frame and object, in this order: */
enum {
  SWEM_JF_INTER = 0,    /* |pred & gt|                                metrics.py:29 */
  SWEM_JF_UNION = 1,    /* |pred | gt|                                metrics.py:30 */
  SWEM_JF_N_FG = 2,     /* boundary pixels of the prediction          metrics.py:81,96 (_seg2bmap :122-178) */
  SWEM_JF_N_GT = 3,     /* boundary pixels of the annotation */
  SWEM_JF_FG_MATCH = 4, /* ... of the prediction within the disk of a boundary pixel of the annotation  metrics.py:89,93 */
  SWEM_JF_GT_MATCH = 5  /* ... of the annotation within the disk of a boundary pixel of the prediction */
};

/* metrics.py:6-37 (db_eval_iou) and :57-119 (f_measure, same-size seg2bmap) up to their integer sums, for every frame and
 * every object of a sequence in one launch sequence (memset, pack, match): nothing is launched per frame.
 *   gt, pred : index maps [T][H][W] uint8, object ids 1..N, 0 = background, ids above N ignored (as `map == o` does)
 *   void_    : [T][H][W] uint8 or NULL; non-zero = void, removed from both masks of every object before anything else
 *              (evaluation.py:57-59 passes one void map for all objects)
 *   counts   : [T][N][SWEM_JF_COUNTS] int32, overwritten
 *   r        : radius of the disk x*x + y*y <= r*r in pixels (metrics.py:77-78: bound_th, or ceil(bound_th * diagonal));
 *              0 <= r <= SWEM_JF_MAX_RADIUS (3840x2160 at the default 0.008 gives 36).  Pixels outside the image are never set.
 *   ws       : swem_jf_workspace bytes: the masks as bit-planes [T][N][2][H][ceil(W/64)] of 64-bit words
 * N <= 255.  The sums are integer: any order of the blocks gives the same result. */
size_t swem_jf_workspace(int T, int N, int H, int W);
int swem_jf_counts_u8(void *stream, const unsigned char *gt, const unsigned char *pred, const unsigned char *void_or_null,
                      int *counts, int T, int N, int H, int W, int r, void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SWEM_HIP_METRICS_H */
