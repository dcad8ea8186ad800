"""Yardstick of the evaluation staging kernels (csrc/stage.hip, swem_amd/io.py): numpy restatements of the reference lines they
replace, written from those lines and checked against the reference's own functions by tests/golden/make_golden_io.py (fixture
g10_io.npz; tests/test_io_host.py).  numpy only: no scipy, no cv2, no torch.

  add_overlay        utils/visualization.py:46-64, the SEQUENTIAL loop over the object ids; binary_dilation with scipy's default
                     structuring element (the cross, zero border) as the OR of four zero-padded shifts
  overlay_closed     the per-pixel closed form the kernel evaluates, in numpy: tests compare it with the loop
  onehot_davis       datasets/DAVIS_Test.py:43-48 -> datasets/data_utils.py:141-186 (shuffle=False, valid_shuffle=False)
  onehot_ytvos       datasets/YTVOS_Test.py:124-130
  map_mask           methods/basic_modules/basic_evaluator.py:202-206
  suit_size, input_size   datasets/YTVOS_Test.py:14-19, 75-91
  stage_frames64     data_utils.py:102 (b / 255) + F.interpolate(bicubic, align_corners=False) in float64
"""
import numpy as np


# ------------------------------------------------------------------------------------------------------------- overlay
def dilate4(b):
    """binary_dilation(b) with the default structure: a pixel is set when it or one of its four edge neighbours is."""
    out = b.copy()
    out[1:, :] |= b[:-1, :]
    out[:-1, :] |= b[1:, :]
    out[:, 1:] |= b[:, :-1]
    out[:, :-1] |= b[:, 1:]
    return out


def add_overlay(img, mask, colors, alpha=0.4):
    """img (H,W,3) uint8, mask (H,W) integer labels, colors 256x3 (any shape) -> (H,W,3) uint8.  Channel-wise: whether img and
    colors are both RGB or both BGR gives the same picture, so the reference's `[::-1]` on the colour is the caller's business
    (here: img and colors in the SAME channel order)."""
    ids = np.unique(mask)
    out = img.copy()
    rest = np.ones(3) * (1 - alpha)            # the reference's ones_np, one pixel of it
    colors = np.reshape(colors, (-1, 3))
    for i in ids[1:]:
        m = mask == i
        # the reference forms the whole canvas and takes canvas[m]; the same float64 values, formed for the object's pixels only
        out[m] = img[m] * alpha + rest * np.array(colors[i])        # float64 -> uint8: truncation
        out[dilate4(m) ^ m, :] = 0
    return out


def overlay_closed(img, mask, colors, alpha=0.4):
    """The same picture without the loop.  S = labels present without the smallest; for a pixel with label L, M = the largest
    label of S other than L among its four edge neighbours (inside the image).  L in S and L > M: the blend; else M exists: 0;
    else img."""
    mask = mask.astype(np.int64)
    colors = np.reshape(colors, (-1, 3)).astype(np.float64)
    s0 = int(mask.min())
    pad = np.full((mask.shape[0] + 2, mask.shape[1] + 2), -1, np.int64)
    pad[1:-1, 1:-1] = mask
    M = np.full(mask.shape, -1, np.int64)
    for nb in (pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]):
        ok = (nb >= 0) & (nb != mask) & (nb != s0)
        M = np.where(ok, np.maximum(M, nb), M)
    blend = (mask != s0) & (mask > M)
    canvas = img.astype(np.float64) * alpha + (1 - alpha) * colors[mask]
    out = img.copy()
    out[blend] = canvas[blend]
    out[~blend & (M >= 0)] = 0
    return out


# ------------------------------------------------------------------------------------------------------------- one-hot
def onehot_davis(mask, single_obj=False):
    """(obj_n,H,W) float32, obj_n = mask.max() + 1: the ids present in ascending order in channels 1.., the rest of the channels
    empty, channel 0 = 1 - the sum of the others."""
    mask = mask.astype(np.int64)
    if single_obj:
        mask = np.where(mask > 1, 1, mask)
    obj_n = int(mask.max()) + 1
    ids = [i for i in range(1, obj_n) if (mask == i).any()]
    out = np.zeros((obj_n,) + mask.shape, np.float32)
    for k, i in enumerate(ids[:obj_n - 1]):
        out[k + 1] = mask == i
    out[0] = 1 - out.sum(0)
    return out


def apply_table(mask, table, channels):
    """What swem_labels_onehot_u8 computes: out[c] = (table[mask] == c)."""
    ch = np.asarray(table)[mask]
    return (ch[None] == np.arange(channels)[:, None, None]).astype(np.float32)


def onehot_ytvos(mask, ids):
    """(len(ids)+1,H,W) float32: channel 0 where the label is 0, channel k+1 where it is ids[k]; other labels nowhere."""
    out = np.zeros((len(ids) + 1,) + mask.shape, np.float32)
    out[0][mask == 0] = 1
    for k, i in enumerate(ids):
        out[k + 1][mask == i] = 1
    return out


def id_list(ann):
    """obj_idx_list (YTVOS_Test.py:117-128) of ann = {frame_idx: (label, ids)} visited in frame order."""
    out = [0]
    for f in sorted(ann):
        for i in ann[f][1]:
            out.append(int(i))
    return out


def map_mask(idx, ids):
    """pred[idx == i] = ids[i] for every i; zero elsewhere; -> uint8."""
    pred = np.zeros_like(idx)
    for i in range(len(ids)):
        pred[idx == i] = ids[i]
    return pred.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- sizes
def suit_size(size, ratio=16):
    r = size % ratio
    size -= r
    if r > 7:
        size += 16
    return size


def input_size(h, w, short_size=495):
    ss = suit_size(short_size)
    if h < w:
        if h < ss:
            out_h, out_w = suit_size(h), suit_size(w)
        else:
            out_h = ss
            out_w = suit_size(int(w * out_h / h))
            out_w = suit_size(out_w)
    else:
        if w < ss:
            out_h, out_w = suit_size(h), suit_size(w)
        else:
            out_w = ss
            out_h = suit_size(int(h * out_w / w))
    return out_h, out_w


# ------------------------------------------------------------------------------------------------------------- frames
def cubic_weights(t, f, a=-0.75):
    """The four cubic weights of the fraction t in dtype f: the one cubic of the test references (tests/augment_ref.py and
    tests/synth_ref.py sample with it too)."""
    a = f(a)

    def c1(x):
        return ((a + f(2)) * x - (a + f(3))) * x * x + f(1)

    def c2(x):
        return ((a * x - f(5) * a) * x + f(8) * a) * x - f(4) * a
    return [c2(t + f(1)), c1(t), c1(f(1) - t), c2(f(2) - t)]


def _cubic_matrix(n_in, n_out):
    """(n_out, n_in) float64: ATen's upsample_bicubic2d along one axis, align_corners=False, A = -0.75, taps clamped."""
    o = np.arange(n_out, dtype=np.float64)
    s = (n_in / n_out) * (o + 0.5) - 0.5
    f = np.floor(s)
    w = np.stack(cubic_weights(s - f, np.float64), 1)
    m = np.zeros((n_out, n_in), np.float64)
    for k in range(4):
        idx = np.clip(f.astype(np.int64) - 1 + k, 0, n_in - 1)
        np.add.at(m, (np.arange(n_out), idx), w[:, k])
    return m


def stage_frames64(frames_u8, size):
    """(T,H,W,3) uint8 -> (T,3,Ho,Wo) float64: b / 255, then the bicubic resize."""
    x = frames_u8.astype(np.float64).transpose(0, 3, 1, 2) / 255.0
    my, mx = _cubic_matrix(x.shape[2], size[0]), _cubic_matrix(x.shape[3], size[1])
    return np.einsum('oh,tchw,pw->tcop', my, x, mx, optimize=True)
