/*
 * swem_hip_io.h -- C ABI of libswem_hip.so, evaluation staging part: decoded bytes in, result bytes out (csrc/stage.hip), result
 * PNG files out (csrc/png.hip), PNG files in (csrc/png_decode.hip).
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

/* utils/visualization.py:40-43 (save_seg_mask: Image.fromarray, putpalette, save) as the evaluator calls it for every result
 * frame (basic_evaluator.py:177-192, 254-260), without the host: T index maps in, T complete PNG files out (csrc/png.hip,
 * DESIGN.md section 11).  Scanlines use filter type 0; the deflate stream is cut into segments of up to 16 whole scanlines (at
 * most 65535 bytes), each coded on its own with literals and matches at distance 1 under the fixed Huffman codes, or as a
 * stored block where that is shorter, ended on a byte boundary and carried by an IDAT chunk of its own.  Any PNG reader
 * decodes the files to the maps, byte for byte; they are larger than zlib's.
 *
 * The largest file a H x W map can give: every segment stored, plus the headers --
 *   8 + 25 + 780 (signature, IHDR, PLTE) + 2 (zlib header) + H * (W + 1) + 17 * nseg (a stored block's 5 bytes and a chunk's 12)
 *   + 21 + 12 (closing IDAT with the final empty block and the Adler-32, IEND),
 *   nseg = ceil(H / min(16, floor(65535 / (W + 1)))).
 * 0 for a shape the encoder refuses (H < 1, W < 1, W + 1 > 65535). */
size_t swem_png_capacity(int H, int W);
/* basic_evaluator.py:177-192, 254-260: the scratch of one call on T frames (segment slots and their lengths / checksums) */
size_t swem_png_workspace(int T, int H, int W);
/* visualization.py:40-43 for the T maps of basic_evaluator.py:177-192, 254-260 in three launches (encode, offsets, pack).
 *   maps       : [T][H][W] uint8 (device)
 *   palette768 : 256 x 3 uint8 RGB (HOST) -> colour type 3 with a 256-entry PLTE; NULL -> colour type 0 (grayscale), no PLTE:
 *                save_seg_mask(palette=None)
 *   blob       : blob_bytes >= T * swem_png_capacity(H, W) (device): the T files back to back, file t = blob[offsets[t] ..
 *                offsets[t + 1])
 *   offsets    : T + 1 int64 (device, 8-byte aligned); offsets[0] = 0, offsets[T] = the bytes to copy to the host
 *   ws         : swem_png_workspace(T, H, W) bytes, 16-byte aligned
 * 1 <= T <= 65535.  A blob or workspace below those sizes is refused (SWEM_E_WORKSPACE) before anything is launched: the
 * kernels cannot write past either. */
int swem_png_encode_u8(void *stream, const unsigned char *maps, const unsigned char *palette768, unsigned char *blob,
                       size_t blob_bytes, long long *offsets, int T, int H, int W, void *ws, size_t ws_bytes);

/* The same files with a Huffman table of each segment's own, and truecolour pictures: the overlay pictures of
 * utils/visualization.py:46-72 as basic_evaluator.py:185-196, 241-265 writes them.
 *   channels 1 : index maps as above (filter type 0; colour type 3 with a palette, 0 without)
 *   channels 3 : [T][H][W][3] uint8 RGB -> colour type 2, no PLTE.  Every scanline takes the filter type 0-4 with the smallest
 *                sum of |signed residual| (ties: the lower type); the row above the first row of a segment is the source
 *                picture's, above row 0 zeros.
 * A scanline is rw = channels * W + 1 bytes; a segment is min(16, floor(65535 / rw)) whole scanlines, coded on its own with
 * literals and matches at distance 1 and ended as above, so one-channel files under SWEM_PNG_CODES_FIXED are byte for byte
 * those of swem_png_encode_u8.
 *   SWEM_PNG_CODES_FIXED   : a segment is the smaller of its stored block and its fixed-code block (coded only if strictly
 *                            smaller)
 *   SWEM_PNG_CODES_DYNAMIC : also a dynamic block (RFC 1951 section 3.2.7): literal/length code lengths of at most 15 bits,
 *                            optimal for the segment's own histogram (package-merge, ties by symbol index), canonical codes,
 *                            the lengths run-length coded with symbols 16-18 under a code-length code of at most 7 bits, and
 *                            one distance code of length 1 (HDIST = 0: only distance 1 occurs).  The segment takes the
 *                            dynamic block only if strictly smaller than the fixed one, and a coded block only if strictly
 *                            smaller than the stored one: a file never grows past the capacity.
 * Capacity: the formula above with rw = channels * W + 1 in the place of W + 1, without the 780 PLTE bytes for 3 channels.
 * 0 for a shape the encoder refuses (channels not 1 or 3, H < 1, W < 1, channels * W + 1 > 65535). */
#define SWEM_PNG_CODES_FIXED 0
#define SWEM_PNG_CODES_DYNAMIC 1
size_t swem_png_capacity_px(int H, int W, int channels);
size_t swem_png_workspace_px(int T, int H, int W, int channels);
/* pixels: [T][H][W] (channels 1) or [T][H][W][3] (channels 3) uint8 (device); palette768 as above, NULL with 3 channels;
 * blob_bytes >= T * swem_png_capacity_px(H, W, channels); offsets, ws (swem_png_workspace_px bytes) as above.  Refused before
 * anything is launched: null pointers, channels not 1 or 3, a palette with 3 channels, an unknown `codes`, a row past 65535
 * bytes, a short blob or workspace.  Three launches; the encode launch declares up to 65536 bytes of LDS for the segment and,
 * under SWEM_PNG_CODES_DYNAMIC, about 10 KiB of tables behind it. */
int swem_png_encode_px_u8(void *stream, const unsigned char *pixels, int channels, const unsigned char *palette768, int codes,
                          unsigned char *blob, size_t blob_bytes, long long *offsets, int T, int H, int W, void *ws,
                          size_t ws_bytes);

/* The way back (csrc/png_decode.hip, csrc/inflate_core.h): T PNG files in, T pixel slots out -- the
 * annotations of datasets/DAVIS_Test.py:40-49 and datasets/YTVOS_Test.py:116-132 and the palette file of VAL.DAVIS_PALETTE_DIR,
 * which the reference opens with PIL on the host.  One wavefront per file, all files in one launch: the chunks are walked and
 * their CRC-32 checked, the IDAT payloads compacted, the zlib stream inflated (stored, fixed and dynamic blocks, distances up to
 * 32768), the Adler-32 checked, the scanlines unfiltered (types 0-4) and depths 1, 2 and 4 unpacked, most significant bits first.
 * Reads: no interlace; colour type 3 and 0 at depths 1, 2, 4, 8 (channels 1: the samples as stored, nothing is scaled), colour
 * type 2 at depth 8 (channels 3).  As strict as tests/png_ref.py and zlib's inflate; a file it refuses gets a status word, an
 * all-zero slot and sizes (0, 0), and its neighbours are decoded.  0 is a good file. */
#define SWEM_PNG_ST_OK 0
#define SWEM_PNG_ST_OFFSETS 1         /* offsets[t] > offsets[t + 1], outside 0..blob_bytes, or a file of 2 GiB and more */
#define SWEM_PNG_ST_SIGNATURE 2
#define SWEM_PNG_ST_CHUNK 3           /* a chunk runs past the file */
#define SWEM_PNG_ST_CRC 4
#define SWEM_PNG_ST_IHDR 5            /* not first, not once, not 13 bytes */
#define SWEM_PNG_ST_DIMENSIONS 6      /* zero, or past 2^31 - 1 */
#define SWEM_PNG_ST_UNSUPPORTED 7     /* a depth, colour type or interlace this decoder does not read; the other `channels` */
#define SWEM_PNG_ST_METHOD 8          /* compression or filter method not 0 */
#define SWEM_PNG_ST_PLTE 9            /* missing, late, doubled, of a bad length; present without colour type 3 */
#define SWEM_PNG_ST_IDAT 10           /* absent, or not consecutive */
#define SWEM_PNG_ST_CRITICAL 11       /* an unknown critical chunk */
#define SWEM_PNG_ST_IEND 12           /* missing, or not empty */
#define SWEM_PNG_ST_TRAILING 13       /* bytes after IEND */
#define SWEM_PNG_ST_TOO_LARGE 14      /* larger than the slot */
#define SWEM_PNG_ST_ZLIB_CM 15
#define SWEM_PNG_ST_ZLIB_CINFO 16
#define SWEM_PNG_ST_ZLIB_FCHECK 17
#define SWEM_PNG_ST_ZLIB_FDICT 18
#define SWEM_PNG_ST_BLOCK_TYPE 19     /* block type 3 */
#define SWEM_PNG_ST_STORED_LEN 20     /* LEN != ~NLEN */
#define SWEM_PNG_ST_HLIT_HDIST 21     /* more than 286 literal/length or 30 distance codes */
#define SWEM_PNG_ST_REPEAT 22         /* a repeat with nothing before it, or past the last length */
#define SWEM_PNG_ST_OVERSUBSCRIBED 23
#define SWEM_PNG_ST_INCOMPLETE 24     /* (an empty set and a single code of one bit are legal) */
#define SWEM_PNG_ST_NO_EOB 25         /* no code for symbol 256 */
#define SWEM_PNG_ST_BAD_SYMBOL 26     /* symbol 286 or 287, distance symbol 30 or 31, a code that no symbol has */
#define SWEM_PNG_ST_DISTANCE 27       /* a distance reaching before the start of the output */
#define SWEM_PNG_ST_NO_FINAL 28       /* the stream ends before the final block */
#define SWEM_PNG_ST_TRUNCATED 29      /* input running past the IDAT data */
#define SWEM_PNG_ST_IDAT_LEFT 30      /* IDAT bytes after the Adler-32 */
#define SWEM_PNG_ST_LENGTH 31         /* inflated length != h * (rowbytes + 1); a longer stream is cut off there */
#define SWEM_PNG_ST_ADLER 32
#define SWEM_PNG_ST_FILTER 33         /* a filter byte past 4 */
#define SWEM_PNG_ST_INDEX 34          /* an index beyond the PLTE entries */
/* The scratch of one call: the compacted IDAT streams (blob_bytes, rounded up to 16) and T times the inflated scanlines of a full
 * slot, Hs * (channels * Ws + 1) bytes rounded up to 16.  0 for what the call refuses: T outside 1..65535, Hs or Ws < 1,
 * channels not 1 or 3, channels * Ws + 1 > 65535, Hs * (channels * Ws + 1) >= 2^31, blob_bytes == 0. */
size_t swem_png_decode_workspace(int T, int Hs, int Ws, int channels, size_t blob_bytes);
/*   blob, offsets : as swem_png_encode_* leave them, both on the device: file t = blob[offsets[t] .. offsets[t + 1]); offsets:
 *                   T + 1 int64, 8-byte aligned.  The kernel checks them against blob_bytes (SWEM_PNG_ST_OFFSETS).
 *   pixels        : [T][Hs][Ws][channels] uint8 (device); a file of h x w <= Hs x Ws fills the top-left corner, the rest is zero
 *   sizes         : [T][2] int32 (h, w)                     status : [T] int32 (SWEM_PNG_ST_*)
 *   palettes      : [T][768] uint8, the PLTE entries and zeros behind them (all zero without a PLTE), or NULL
 *   n_palette     : [T] int32, the number of PLTE entries, or NULL
 *   ws            : swem_png_decode_workspace(...) bytes, 16-byte aligned
 * One launch; the kernel declares about 77 KiB of LDS (a 64 KiB ring of inflated bytes, the code tables).  Refused before any HIP
 * call: null pointers, a misaligned ws / offsets / sizes / status, channels not 1 or 3, the shapes above (SWEM_E_SHAPE), a short
 * workspace (SWEM_E_WORKSPACE).  Nothing a file contains makes the kernel read or write outside blob, pixels and ws. */
int swem_png_decode_u8(void *stream, const unsigned char *blob, size_t blob_bytes, const long long *offsets, int T, int Hs, int Ws,
                       int channels, unsigned char *pixels, int *sizes, unsigned char *palettes, int *n_palette, int *status,
                       void *ws, size_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SWEM_HIP_IO_H */
