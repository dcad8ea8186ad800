"""GPU: the frame pipeline's pointwise kernels (the inference side of csrc/pointwise.hip: input packing, the pooled stem, the
decoder's upsample-adds, resize_planes, mask_prep, both decoder heads, the argmax, the movers behind ops.py) against float64 at
the corners tests/test_gpu_ops.py does not reach: frames of one 2x2 block, maps of one pixel, every (H, W) of the max-pool up to
its first interior window, fewer pixels than the 32 of a plane-writing block and a partial channel-group block beside them,
sources of one, two and three rows, downscaling, a second and third tile column of the matrix-core prediction head and a tile
that is all halo but two columns, the generic head just past the dispatch, every clamp branch of the decode head, argmax ties,
both paths of pack_u8, transposes whose grid is sized by the padding.

Every comparison is per kernel through the C ABI, identical fp32 inputs on both sides.  The reference is torch on the CPU on
.double() inputs or a numpy restatement (the space-to-depth layout); the decode head's is tests/test_gpu_train_edges.py's
(decode_forward: the clamp bounds are the fp32 ones).  Every output lies in front of a sentinel-filled guard band of GUARD
elements that must come back untouched: a store past a partial block lands there and faults nothing.  The plane-writing
variants must give the plain kernel's y bit for bit and the split kernels' planes of it bit for bit.

Bars, measured as tests/test_gpu_train_edges.py's rel() (max error over max |reference|): 2e-6 for packing, resampling,
mask_prep and lincomb (that module's BARS['bilinear']), 2e-5 for the two heads (tests/test_gpu_ops.py's own).  Every float sweep
exists twice: `test_*` marked gpu runs the kernels, `test_standin_*` (no GPU) runs the SAME cases with fp32 torch on the CPU
standing in for the kernel and asserts that the stand-in sits at least 4x under the bar.  Worst stand-in error / bar (CPU, fp32):
    packing       9.5e-8 / 2e-6 (image channels), 6.1e-8 (`other` of soft masks)       lincomb      4.7e-8 / 2e-6
    upsample_add  1.5e-7 / 2e-6          resize_planes   bilinear 1.7e-7, bicubic 1.1e-7 / 2e-6          mask_prep    1.4e-7 / 2e-6
    pred head     2.3e-7 / 2e-5          decode head     logits 2.0e-7, probabilities 5.7e-7 / 2e-5 (beyond the per-pixel term below)
Where a case's stand-in is NOT 4x under the bar, the case's bar is 8x what the stand-in measures on it, computed beside the
kernel (Sweep.add(standin=)).  The cases that may be on that rule are declared (MAY8_PAIRS, MAY8_BICUBIC, MAY8_MASK, the two
conditions in dec_check): every case whose stand-in was measured above an EIGHTH of its bar -- the stand-in tests assert that
every other case is 4x under its bar.  Measured on them (the fp32 source coordinate scale * (dst + 0.5) - 0.5 and the weights taken
from it):
    7x9 -> 13x27      upsample_add 5.1e-7, bilinear 4.9e-7, bicubic 6.2e-7, mask_prep 4.2e-7 (4.3e-7 with the hard mask at 13x27)
    27x31 -> 107x61   upsample_add 1.7e-6, bilinear 2.6e-6, bicubic 2.4e-6, mask_prep 1.9e-6
    48x85 -> 30x54    upsample_add 3.7e-6, bilinear 5.4e-6, bicubic 4.7e-6, mask_prep 3.9e-6
    31x45 -> 9x11     upsample_add 1.5e-6, bilinear 2.4e-6, bicubic 3.1e-6, mask_prep 1.4e-6
    bicubic alone     1x1 -> 3x5 3.8e-7, 2x3 -> 7x5 4.3e-7 (declared; under 5e-7 here, so on the fixed bar)
    decode head       8x32 -> 31x125 at N(0, 4^2): logits 2.4e-6, probabilities 1.1e-5; the N(0, 40^2) maps: logits 2.2e-5,
                      probabilities 9.6e-5 (a weight's rounding times a neighbour difference of 100, on a logit scale of 16)
The decode head's saturated logits: of the two treatments the issue leaves open this module takes the README's term -- every
logit may miss float64 by 2.5e-7 / (p (1 - p)) on top of the bar, per pixel (dec_excess; fp32 resolves 1 - p to 6e-8, and plain
rel() of fp32 ATen is 1.6e-3 on the N(0, 4^2) logits and 0.1 on the N(0, 40^2) probabilities: 8x that would be no bar) -- and the
8x rule on what is left.  A wrong clamp branch is O(1).
What a bar is worth, with a stand-in that drops ONE source pixel / filter tap at the sweep's largest case
(`test_standin_with_a_dropped_element_misses_the_bars`), as multiples of the case's bar: upsample_add 27x31 -> 107x61 at C = 72
29000x, pred head 13x61 at C = 256 12800x, decode head 8x32 -> 31x125 at N = 7 logits 940x, probabilities 1800x.
What the kernels measure is printed and recorded under frame_edges/<kernel> (helpers.record_parity) before anything is asserted."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from swem_amd import _lib, ops
from tests import helpers as H
from tests import test_gpu_train_edges as TE
from tests.test_gpu_train_edges import DEV, F32, F64, dv, rel

gpu = pytest.mark.gpu
I16, I32, I64, U8 = torch.int16, torch.int32, torch.int64, torch.uint8
PF16 = ops.PLANES_F16

# the project's bars: resampling / packing / mask_prep / lincomb (tests/test_gpu_train_edges.py), the heads (tests/test_gpu_ops.py)
BARS = {'bilinear': TE.BARS['bilinear'], 'heads': 2e-5}


# ------------------------------------------------------------------------------------------------------------ helpers
def sweep(key, shrink=1.0):
    S = TE.Sweep(key, shrink, bars=BARS, prefix='frame_edges/')
    S.eight = {}
    return S


def stand_add(S, tag, name, stand, bar, may8):
    """The stand-in's side of a float comparison: asserted 4x under the bar, unless the case is declared to be on the 8x rule."""
    if may8:
        S.eight[(name,) + tuple(tag)] = float('%.3g' % stand)
    else:
        S.add(tag, name, stand, bar)


GUARD = 4096                # elements behind every output: more than one block can write (256 threads x 8 floats)
FILL = {F32: -12345.5, I16: 0x5A5A, I64: -77, U8: 0xA5}


class Out:
    """A device output of `shape` in front of a guard band; the whole buffer starts as the sentinel."""

    def __init__(self, *shape, dtype=F32):
        self.n, self.fill = int(np.prod(shape)), FILL[dtype]
        self.buf = torch.full((self.n + GUARD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.buf[:self.n].view(*shape)

    def ptr(self):
        return self.buf.data_ptr()

    def band(self):
        return bool((self.buf[self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def biteq(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and bool(torch.equal(a.view(I32), b.view(I32)))


def nhwc(t):
    return dv(t.permute(0, 2, 3, 1))


def first_argmax(p):
    """argmax over dim 1 with the FIRST index winning ties, written out"""
    n = p.shape[1]
    ar = torch.arange(n).view(1, n, *([1] * (p.dim() - 2)))
    return torch.where(p == p.amax(1, keepdim=True), ar, n).amin(1)


def interp(x, size, mode):
    return F.interpolate(x, size=size, mode=mode, **({} if mode == 'nearest' else {'align_corners': False}))


# ---- the plane-writing variants: y is the plain kernel's, the planes are the split kernels' of it
VARIANTS = [(2, 0), (3, 0), (PF16, 0), (0, 2), (0, 3), (0, PF16), (3, 2), (PF16, PF16), (2, PF16)]     # (planes of y, of relu(y))


def plane_rows(npl):
    return 2 if npl == PF16 else npl


def split_planes(y, M, C, relu, npl):
    """swem_split_bf16x3_f32 / swem_split_f16x2_f32 of the device map y (M pixels x C): the first `npl` planes, as int16."""
    st = ops._stream()
    if npl == PF16:
        out = torch.zeros(2, M * C, dtype=I16, device=DEV)
        _lib.call('swem_split_f16x2_f32', st, y.data_ptr(), out.data_ptr(), M, C, int(relu), ops._fault_ptr(y.device))
        return out
    out = torch.zeros(3, M * C, dtype=I16, device=DEV)
    _lib.call('swem_split_bf16x3_f32', st, y.data_ptr(), out.data_ptr(), M, C, int(relu))
    return out[:npl]


def planes_checks(S, tag, launch, y_plain, M, C, variants=VARIANTS):
    """launch(y_ptr, plane arguments) runs the plane-writing form; for every requested variant and layout: y and its band, the
    planes and their bands."""
    yard = {}
    for npl, nplr in variants:
        y = Out(*y_plain.shape)
        pl = Out(plane_rows(npl), M * C, dtype=I16) if npl else None
        plr = Out(plane_rows(nplr), M * C, dtype=I16) if nplr else None
        launch(y.ptr(), (pl.ptr() if pl else 0, npl or 3, plr.ptr() if plr else 0, nplr or 3, ops._fault_ptr(y_plain.device)))
        S.add(tag + (npl, nplr), 'planes_form_y_is_the_plain_kernels', biteq(y.t, y_plain))
        S.add(tag + (npl, nplr), 'guard_band', y.band() and (pl is None or pl.band()) and (plr is None or plr.band()))
        for relu, (p, n) in enumerate(((pl, npl), (plr, nplr))):
            if p is not None:
                if (relu, n) not in yard:
                    yard[relu, n] = split_planes(y_plain, M, C, relu, n)
                S.add(tag + (npl, nplr), 'planes_are_the_split_kernels', bool(torch.equal(p.t, yard[relu, n])))


# ====================================================================================== 1. input packing
PACK_CASES = [(1, 1, 2, 2), (2, 3, 6, 10), (1, 2, 38, 52), (3, 1, 4, 130)]
MEAN, STD = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])


def pack_inputs(B, N, Hh, Ww, soft):
    g = torch.Generator().manual_seed(100 + B + N + Hh * Ww + soft)
    frames = torch.rand(B, 3, Hh, Ww, generator=g)
    if soft:
        m = torch.rand(B, N + 1, Hh, Ww, generator=g) * 0.5       # (not normalised: with N = 1 `other` would be 0 in float64)
    else:
        m = F.one_hot(torch.randint(0, N + 1, (B, Hh, Ww), generator=g), N + 1).permute(0, 3, 1, 2).float().contiguous()
    return frames, m


def pack_ref(frames, masks, single, dtype):
    """swem.py:48-53 + networks.py:115-117 on the fp32 mean and std -> the value form (B N, H, W, 8):
    (r, g, b, mask, 1 - mask - background, 0, 0, 0); its first object's (r, g, b, 0, ...) is the key form."""
    B, _, Hh, Ww = frames.shape
    N = masks.shape[1] - 1
    img = (frames.to(dtype) - MEAN.to(dtype).view(1, 3, 1, 1)) / STD.to(dtype).view(1, 3, 1, 1)
    out = torch.zeros(B, N, Hh, Ww, 8, dtype=dtype)
    out[..., :3] = img.permute(0, 2, 3, 1)[:, None]
    out[..., 3] = masks[:, 1:].to(dtype)
    if not single:
        out[..., 4] = 1 - masks[:, 1:].to(dtype) - masks[:, :1].to(dtype)
    return out.view(B * N, Hh, Ww, 8)


def s2d_layout(v):
    """The comment above prep_input_s2d_kernel restated: a 2x2 pixel block becomes one pixel of 4 phases x 8 channels, channel
    (py 2 + px) 8 + c, stored behind one zero block row and column: (BN, H, W, 8) -> (BN, H/2 + 1, W/2 + 1, 32)."""
    a = v.numpy()
    BN, Hh, Ww, _ = a.shape
    out = np.zeros((BN, Hh // 2 + 1, Ww // 2 + 1, 32), a.dtype)
    out[:, 1:, 1:] = a.reshape(BN, Hh // 2, 2, Ww // 2, 2, 8).transpose(0, 1, 3, 2, 4, 5).reshape(BN, Hh // 2, Ww // 2, 32)
    return torch.from_numpy(out)


def key_of(v, B, N):
    """the key form (B, H, W, 8: r, g, b and five zeros) of a value form"""
    k = v.view(B, N, *v.shape[1:])[:, 0].clone()
    k[..., 3:] = 0
    return k


def s2d_call(frames_d, masks_d, out, planes, npl, B, N, Hh, Ww, single):
    m3, s3 = ops._f3(MEAN), ops._f3(STD)
    _lib.call('swem_prep_input_s2d_f32', ops._stream(), frames_d.data_ptr(), 0 if masks_d is None else masks_d.data_ptr(),
              ctypes.addressof(m3), ctypes.addressof(s3), out, planes, npl, B, N, Hh, Ww, int(single),
              ops._fault_ptr(frames_d.device))


def pack_hip(frames, masks, single):
    B, _, Hh, Ww = frames.shape
    N = masks.shape[1] - 1
    m3, s3, st = ops._f3(MEAN), ops._f3(STD), ops._stream()
    fd, md = dv(frames), dv(masks)
    key, val = Out(B, Hh, Ww, 4), Out(B * N, Hh, Ww, 8)
    s2d, s2k = Out(B * N, Hh // 2 + 1, Ww // 2 + 1, 32), Out(B, Hh // 2 + 1, Ww // 2 + 1, 32)
    _lib.call('swem_prep_key_input_f32', st, fd.data_ptr(), ctypes.addressof(m3), ctypes.addressof(s3), key.ptr(), B, Hh, Ww)
    _lib.call('swem_prep_value_input_f32', st, fd.data_ptr(), md.data_ptr(), ctypes.addressof(m3), ctypes.addressof(s3), val.ptr(),
              B, N, Hh, Ww, int(single))
    s2d_call(fd, md, s2d.ptr(), 0, 3, B, N, Hh, Ww, single)
    s2d_call(fd, None, s2k.ptr(), 0, 3, B, 1, Hh, Ww, single)
    bands = key.band() and val.band() and s2d.band() and s2k.band()
    return key.t.cpu(), val.t.cpu(), s2d.t.cpu(), s2k.t.cpu(), bands


def pack_check(S, hip):
    for B, N, Hh, Ww in PACK_CASES:
        for soft in (0, 1):
            frames, masks = pack_inputs(B, N, Hh, Ww, soft)
            for single in (0, 1):
                tag = (B, N, Hh, Ww, soft, single)
                want = pack_ref(frames, masks, single, F64)
                if hip:
                    key, val, s2d, s2k, bands = pack_hip(frames, masks, single)
                    S.add(tag, 'guard_band', bands)
                else:
                    val = pack_ref(frames, masks, single, F32)
                    key, s2d, s2k = key_of(val, B, N)[..., :4], s2d_layout(val), s2d_layout(key_of(val, B, N))
                wkey = key_of(want, B, N)
                S.add(tag, 'key_image', rel(key[..., :3], wkey[..., :3]), 'bilinear')
                S.add(tag, 'value_image', rel(val[..., :3], want[..., :3]), 'bilinear')
                S.add(tag, 'pad_channels_zero', bool((key[..., 3] == 0).all() and (val[..., 5:] == 0).all()))
                S.add(tag, 'mask_channel_is_the_input', bool(torch.equal(val[..., 3].reshape(B, N, Hh, Ww), masks[:, 1:])))
                if soft and not single:
                    S.add(tag, 'other_soft', rel(val[..., 4], want[..., 4]), 'bilinear')
                else:
                    S.add(tag, 'other_exact', bool(torch.equal(val[..., 4].double(), want[..., 4])))
                # the space-to-depth forms: the zero block row and column, and the (block, phase, channel) layout -- the value / key
                # kernels' own numbers rearranged by the restatement, bit for bit -- and float64 in the same layout
                S.add(tag, 's2d_zero_row_and_column', bool((s2d[:, 0] == 0).all() and (s2d[:, :, 0] == 0).all()
                                                           and (s2k[:, 0] == 0).all() and (s2k[:, :, 0] == 0).all()))
                S.add(tag, 's2d_layout_value_form', biteq(s2d, s2d_layout(val)))
                S.add(tag, 's2d_layout_key_form', biteq(s2k, s2d_layout(key_of(val, B, N))))
                S.add(tag, 's2d_image', rel(s2d, s2d_layout(want)), 'bilinear')


@gpu
def test_input_packing_vs_float64(lib):
    """swem_prep_key_input_f32, swem_prep_value_input_f32 and swem_prep_input_s2d_f32 (value form and key form, masks == NULL) at
    one 2x2 block, B > 1 with N > 1, 38x52 and a 4x130 strip; single_obj both ways; one-hot masks (`other` exact) and soft ones
    (within 2e-6): image channels against float64 (f - mean) / std on the fp32 mean and std, pad channels exactly 0, the mask
    channel exactly the input, the space-to-depth zero row / column and layout against the numpy restatement."""
    S = sweep('packing')
    pack_check(S, True)
    S.finish()


def test_standin_input_packing():
    S = sweep('standin/packing', shrink=0.25)
    pack_check(S, False)
    S.finish(record=False)


@gpu
def test_s2d_planes_are_the_split_kernels_planes(lib):
    """swem_prep_input_s2d_f32's operand planes (nplanes 2, 3 and SWEM_PLANES_F16; value and key form; with the fp32 image and
    planes only) are bit for bit the split kernels' of the fp32 image it writes."""
    S = sweep('s2d_planes')
    for B, N, Hh, Ww in PACK_CASES:
        frames, masks = pack_inputs(B, N, Hh, Ww, 1)
        fd = dv(frames)
        for md, n in ((dv(masks), N), (None, 1)):
            Hb, Wb = Hh // 2 + 1, Ww // 2 + 1
            M = B * n * Hb * Wb
            img = Out(B * n, Hb, Wb, 32)
            s2d_call(fd, md, img.ptr(), 0, 3, B, n, Hh, Ww, 0)
            for npl in (2, 3, PF16):
                tag = (B, n, Hh, Ww, md is not None, npl)
                want = split_planes(img.t, M, 32, 0, npl)
                for with_image in (1, 0):
                    out, pl = Out(B * n, Hb, Wb, 32), Out(plane_rows(npl), M * 32, dtype=I16)
                    s2d_call(fd, md, out.ptr() if with_image else 0, pl.ptr(), npl, B, n, Hh, Ww, 0)
                    S.add(tag, 'planes_are_the_split_kernels', bool(torch.equal(pl.t, want)))
                    S.add(tag, 'image_beside_the_planes', biteq(out.t, img.t) if with_image else out.untouched())
                    S.add(tag, 'guard_band', pl.band() and out.band())
    ops.check_faults()
    S.finish()


# ====================================================================================== 2. max-pool
POOL_SIZES = (1, 2, 3, 4, 5, 8)
POOL_C = (4, 12, 8, 72, 136)


@gpu
def test_maxpool_every_small_size_and_its_planes(lib):
    """swem_maxpool3x3s2_nhwc_f32 at every (H, W) in {1, 2, 3, 4, 5, 8}^2, B = 2, C = 4, 12, 8, 72, 136: EQUAL to float64
    max_pool2d (a max is exact), on inputs that are all negative in half the cases (a padded tap read as 0 would win).  The planes
    form at the multiples of 8 (72 and 136: a partial last channel-group block; B Ho Wo = 2 .. 32: never more than one pixel
    block, full only at 8x8): y bit-equal to the plain kernel, every variant (plain, ReLU, both) and layout (2, 3, f16) bit-equal
    to the split kernels of y."""
    S = sweep('maxpool')
    g = torch.Generator().manual_seed(200)
    st = ops._stream()
    for Hh in POOL_SIZES:
        for Ww in POOL_SIZES:
            for i, C in enumerate(POOL_C):
                neg = (Hh + Ww + i) % 2
                x = torch.randn(2, Hh, Ww, C, generator=g)
                x = -x.abs() - 0.5 if neg else x
                want = F.max_pool2d(x.permute(0, 3, 1, 2).double(), 3, 2, 1).permute(0, 2, 3, 1)
                Ho, Wo = want.shape[1:3]
                xd, y = dv(x), Out(2, Ho, Wo, C)
                _lib.call('swem_maxpool3x3s2_nhwc_f32', st, xd.data_ptr(), y.ptr(), 2, Hh, Ww, C)
                tag = (Hh, Ww, C, neg)
                S.add(tag, 'equals_float64_max_pool2d', bool(torch.equal(y.t.cpu().double(), want)))
                S.add(tag, 'guard_band', y.band())
                if C % 8 == 0:
                    planes_checks(S, tag, lambda yp, pa: _lib.call('swem_maxpool3x3s2_nhwc_f32_planes', st, xd.data_ptr(), yp, 2, Hh, Ww,
                                                                   C, *pa), y.t, 2 * Ho * Wo, C)
    ops.check_faults()
    S.finish()


# ====================================================================================== 3. resampling
PAIRS = [((1, 1), (3, 5)), ((2, 3), (7, 5)), ((7, 9), (13, 27)), ((15, 27), (30, 54)), ((27, 31), (107, 61)), ((48, 85), (30, 54)),
         ((31, 45), (9, 11)), ((13, 7), (13, 7))]
# the size pairs whose fp32 stand-in was measured above an eighth of the 2e-6 bar on some kernel (values in the module docstring)
MAY8_PAIRS = {((7, 9), (13, 27)), ((27, 31), (107, 61)), ((48, 85), (30, 54)), ((31, 45), (9, 11))}
MAY8_BICUBIC = MAY8_PAIRS | {((1, 1), (3, 5)), ((2, 3), (7, 5))}          # (sixteen taps with weights of both signs)
UP_C = (4, 8, 72)


def test_nearest_picks_the_same_pixel_in_both_precisions():
    """What lets `nearest` be compared EXACTLY: for every size pair used here (PAIRS, and the 23x37 -> 3x5 of mask_prep) fp32 and
    float64 ATen pick the same source pixel."""
    for src, dst in PAIRS + [((23, 37), (3, 5))]:
        idx = torch.arange(src[0] * src[1], dtype=F32).view(1, 1, *src)
        assert torch.equal(interp(idx, dst, 'nearest').double(), interp(idx.double(), dst, 'nearest')), (src, dst)


def up_inputs(src, dst, C):
    g = torch.Generator().manual_seed(300 + C + src[0] * src[1] + dst[0])
    return (torch.randn(2, C, *dst, generator=g), torch.randn(2, C, *src, generator=g),
            torch.randn(6, C, *src, generator=g) if C <= 8 else None)


def up_call(name, skip_d, skip_bs, group, low_d, yp, B, src, dst, C, pa=()):
    args = (skip_d.data_ptr(), skip_bs) + ((group,) if 'grouped' in name else ()) + (low_d.data_ptr(), yp, B, src[0], src[1], dst[0], dst[1], C)
    _lib.call(name, ops._stream(), *args, *pa)


def up_forms(src, dst, C):
    """(form, entry point, skip, skip_bs, group, low): the plain call, a skip shared by the batch (skip_bs = 0), and -- at C <= 8,
    to stay small -- six items in groups of 3 on two skip images"""
    skip, low, low6 = up_inputs(src, dst, C)
    n = dst[0] * dst[1] * C
    forms = [('plain', 'swem_upsample_add_nhwc_f32', skip, n, 1, low), ('shared', 'swem_upsample_add_nhwc_f32', skip[:1], 0, 1, low)]
    if low6 is not None:
        forms.append(('grouped', 'swem_upsample_add_grouped_nhwc_f32', skip, n, 3, low6))
    return forms


def up_check(S, hip):
    for src, dst in PAIRS:
        for C in UP_C:
            for form, name, skip, sbs, group, low in up_forms(src, dst, C):
                B = low.shape[0]
                sk = skip.repeat_interleave(B // skip.shape[0], 0)            # (item b adds skip image b // group; shared: image 0)
                want = sk.double() + interp(low.double(), dst, 'bilinear')
                stand = rel(sk + interp(low, dst, 'bilinear'), want)
                tag = (src, dst, C, form)
                if hip:
                    y, sd, ld = Out(B, *dst, C), nhwc(skip), nhwc(low)
                    up_call(name, sd, sbs, group, ld, y.ptr(), B, src, dst, C)
                    S.add(tag, 'upsample_add', rel(y.t.permute(0, 3, 1, 2), want), 'bilinear', standin=stand)
                    S.add(tag, 'guard_band', y.band())
                    if C % 8 == 0 and form != 'shared':
                        planes_checks(S, tag, lambda yp, pa: up_call(name + '_planes', sd, sbs, group, ld, yp, B, src, dst, C, pa),
                                      y.t, B * dst[0] * dst[1], C)
                else:
                    stand_add(S, tag, 'upsample_add', stand, 'bilinear', (src, dst) in MAY8_PAIRS)


@gpu
def test_upsample_add_vs_float64_and_its_planes(lib):
    """swem_upsample_add_nhwc_f32 (plain, and skip_bs = 0: one skip image for the batch), swem_upsample_add_grouped_nhwc_f32
    (group 3) and their _planes forms at PAIRS -- a 1-pixel source, sources of 2 and 3 rows (i1 = i0 + (i0 < in - 1)), x2, x3.96
    on one axis with x1.97 on the other, two downscalings, the identity -- and C = 4, 8, 72 (a partial channel-group block), against
    float64 skip + F.interpolate.  The planes forms: y bit-equal to the plain kernel, the planes to the split kernels."""
    S = sweep('upsample_add')
    up_check(S, True)
    ops.check_faults()
    S.finish()


def test_standin_upsample_add():
    S = sweep('standin/upsample_add', shrink=0.25)
    up_check(S, False)
    print('declared for the 8x rule (on it where above 5e-7): %s' % S.eight)
    S.finish(record=False)


def resize_check(S, hip):
    g = torch.Generator().manual_seed(310)
    for src, dst in PAIRS:
        x = torch.randn(2, 3, *src, generator=g)
        xd = dv(x) if hip else None
        for mode, name in ((1, 'bilinear'), (2, 'bicubic')):
            want = interp(x.double(), dst, name)
            stand = rel(interp(x, dst, name), want)
            if hip:
                y = Out(2, 3, *dst)
                _lib.call('swem_resize_planes_f32', ops._stream(), xd.data_ptr(), y.ptr(), 6, src[0], src[1], dst[0], dst[1], mode)
                S.add((src, dst), name, rel(y.t, want), 'bilinear', standin=stand)
                S.add((src, dst, name), 'guard_band', y.band())
            else:
                stand_add(S, (src, dst), name, stand, 'bilinear', (src, dst) in (MAY8_BICUBIC if mode == 2 else MAY8_PAIRS))
        if hip:
            y = Out(2, 3, *dst)
            _lib.call('swem_resize_planes_f32', ops._stream(), xd.data_ptr(), y.ptr(), 6, src[0], src[1], dst[0], dst[1], 0)
            S.add((src, dst), 'nearest_exact', bool(torch.equal(y.t.cpu(), interp(x, dst, 'nearest'))) and y.band())


@gpu
def test_resize_planes_vs_float64(lib):
    """swem_resize_planes_f32 at PAIRS: bilinear and bicubic against float64 F.interpolate, nearest EXACTLY F.interpolate's on the
    CPU (the header promises ATen's index arithmetic), the flip exactly torch.flip at W = 1, 2 and 85."""
    S = sweep('resize_planes')
    resize_check(S, True)
    g = torch.Generator().manual_seed(311)
    for Ww in (1, 2, 85):
        x = torch.randn(2, 3, 5, Ww, generator=g)
        xd, y = dv(x), Out(2, 3, 5, Ww)
        _lib.call('swem_resize_planes_f32', ops._stream(), xd.data_ptr(), y.ptr(), 6, 5, Ww, 5, Ww, 3)
        S.add(('flip', Ww), 'flip_exact', bool(torch.equal(y.t.cpu(), torch.flip(x, dims=[-1]))) and y.band())
    S.finish()


def test_standin_resize_planes():
    S = sweep('standin/resize_planes', shrink=0.25)
    resize_check(S, False)
    print('declared for the 8x rule (on it where above 5e-7): %s' % S.eight)
    S.finish(record=False)


# (hard size, soft size, output size): every pair with both masks at the source size, the two sizes of swem.py:79-84 apart, and
# the hard mask already at the output size (h = Hh: no nearest step)
MASK_CASES = [(s, s, d) for s, d in PAIRS] + [((23, 37), (24, 40), (3, 5)), ((13, 27), (7, 9), (13, 27))]
MAY8_MASK = {c for c in MASK_CASES if (c[1], c[2]) in MAY8_PAIRS}


def mask_check(S, hip):
    g = torch.Generator().manual_seed(320)
    for hard_hw, soft_hw, out_hw in MASK_CASES:
        for N in (1, 3):
            idx = torch.randint(0, N + 1, (2,) + hard_hw, generator=g)
            hard = F.one_hot(idx, N + 1).permute(0, 3, 1, 2).contiguous()                      # exact 0 / 1, int64
            soft = torch.rand(2, N + 1, *soft_hw, generator=g)
            mh = interp(hard[:, 1:].float(), out_hw, 'nearest')
            P = out_hw[0] * out_hw[1]

            def ref(dtype):
                ms = interp(soft[:, 1:].to(dtype), out_hw, 'bilinear')
                return torch.stack([(1 - mh.to(dtype)) * (1 - ms), mh.to(dtype) * ms], 2).reshape(2 * N, 2, P)
            want, tag = ref(F64), (hard_hw, soft_hw, out_hw, N)
            stand = rel(ref(F32), want)
            if hip:
                sd = dv(soft)
                for dtype in (I64, F32):
                    hd, y = dv(hard.to(dtype)), Out(2 * N, 2, P)
                    _lib.call('swem_mask_prep_f32', ops._stream(), hd.data_ptr(), int(dtype == I64), hard_hw[0], hard_hw[1], sd.data_ptr(),
                              soft_hw[0], soft_hw[1], y.ptr(), 2, N, out_hw[0], out_hw[1])
                    S.add(tag + (str(dtype),), 'mask_prep', rel(y.t, want), 'bilinear', standin=stand)
                    S.add(tag + (str(dtype),), 'guard_band', y.band())
            else:
                stand_add(S, tag, 'mask_prep', stand, 'bilinear', (hard_hw, soft_hw, out_hw) in MAY8_MASK)


@gpu
def test_mask_prep_vs_float64(lib):
    """swem_mask_prep_f32 with B = 2, N = 1 and 3, int64 and float hard masks (exact 0 / 1: the nearest step is exact, ATen's
    pixel) at MASK_CASES, against (1 - h)(1 - s), h s with the soft mask resampled in float64."""
    S = sweep('mask_prep')
    mask_check(S, True)
    S.finish()


def test_standin_mask_prep():
    S = sweep('standin/mask_prep', shrink=0.25)
    mask_check(S, False)
    print('declared for the 8x rule (on it where above 5e-7): %s' % S.eight)
    S.finish(record=False)


# ====================================================================================== 4. heads
PRED_CASES = [(256, (1, 6, 30)), (256, (1, 7, 31)), (256, (2, 5, 29)), (256, (1, 13, 61)), (256, (1, 1, 33)), (256, (1, 12, 1)),
              (260, (1, 7, 31))]


def test_pred_cases_reach_what_they_are_for():
    """(tile rows, tile columns, width of the last tile column, height of the last tile row) of the 6 x 30 output tiles: exactly one
    tile; one extra row and column (the second tiles hold ONE output row / column); a partial tile in both directions; 3 x 3 tiles
    whose last column is one pixel wide (its 8 x 32 input tile is out of the image but for two columns); H = 1; W = 1."""
    got = [(-(-h // 6), -(-w // 30), w - (-(-w // 30) - 1) * 30, h - (-(-h // 6) - 1) * 6) for C, (_, h, w) in PRED_CASES if C == 256]
    assert got == [(1, 1, 30, 6), (2, 2, 1, 1), (1, 1, 29, 5), (3, 3, 1, 1), (1, 2, 3, 1), (2, 1, 1, 6)], got


def pred_inputs(C, bhw):
    g = torch.Generator().manual_seed(400 + C + bhw[0] * bhw[1] * bhw[2])
    return (torch.randn(bhw[0], C, *bhw[1:], generator=g), torch.randn(1, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5,
            torch.randn(1, generator=g) + 2.0)


def pred_check(S, hip):
    for C, bhw in PRED_CASES:
        x, w, b = pred_inputs(C, bhw)
        want = F.conv2d(F.relu(x.double()), w.double(), b.double(), padding=1)[:, 0]
        stand = rel(F.conv2d(F.relu(x), w, b, padding=1)[:, 0], want)
        S.add((C, bhw), 'half_of_x_is_negative', bool(0.4 < float((x < 0).float().mean()) < 0.6 and float(b.abs()) > 0.1))
        if hip:
            xd, wd, bd, y = nhwc(x), nhwc(w), dv(b), Out(*bhw)
            _lib.call('swem_pred_head_f32', ops._stream(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.ptr(), *bhw, C)
            S.add((C, bhw), 'logit', rel(y.t, want), 'heads', standin=stand)
            S.add((C, bhw), 'guard_band', y.band())
        else:
            stand_add(S, (C, bhw), 'logit', stand, 'heads', False)


@gpu
def test_pred_head_tile_edges_vs_float64(lib):
    """swem_pred_head_f32 at C = 256 (pred_head_mfma_kernel: 6 x 30 output tiles on 8 x 32 haloed input tiles) where the tiling can
    go wrong (test_pred_cases_reach_what_they_are_for), and at C = 260, the generic kernel just past the dispatch, against
    float64 conv2d(relu(x)) with a non-zero bias."""
    S = sweep('pred_head')
    pred_check(S, True)
    S.finish()


def test_standin_pred_head():
    S = sweep('standin/pred_head', shrink=0.25)
    pred_check(S, False)
    S.finish(record=False)


DEC_SIZES = [((5, 7), (20, 28)), ((6, 5), (23, 19)), ((8, 32), (31, 125))]
DEC_CASES = [(N, hw, val, sigma) for sigma in (4.0, 40.0) for N in (1, 2, 3, 7) for hw in DEC_SIZES for val in ('none', 'one', 'all')]
GAP = 1e-4
ULP4 = 2.5e-7          # the README's term: 4 ulp of a probability near 1, through d(logit) / dp = 1 / (p (1 - p))


def dec_excess(lg, pr, agg, lg64, pr64):
    """The decode head's two measures.  fp32 resolves 1 - p to 6e-8, so a saturated logit is not a 2e-5 quantity in ANY fp32
    arithmetic (fp32 ATen is 1.6e-3 from float64 on the N(0, 4^2) maps and 2.5e-2 on the N(0, 40^2) ones, where its probabilities
    are 0.1 off: 8x that would be no bar at all) -- of the two ways the issue leaves open this is the README's: every logit may miss
    float64 by e = 2.5e-7 / (p (1 - p)) (p the clamped probability it is the logit of) on top of the bar.  The probabilities are
    softmax(logits): with every logit anywhere within its e, P_k lies in [P_k exp(-e_k) / sum_j P_j exp(e_j),
    P_k exp(e_k) / sum_j P_j exp(-e_j)] -- what is measured is how far the kernel's lies outside that interval.  Where no logit
    saturates, e is 1e-6 and both measures are the plain error."""
    pc = agg.clamp(TE.LO32, TE.HI32)
    e = ULP4 / (pc * (1 - pc))
    lg, pr = lg.double(), pr.double()
    logit = float(((lg - lg64).abs() - e).clamp(min=0).max() / lg64.abs().max())
    lo = pr64 * torch.exp(-e) / (pr64 * torch.exp(e)).sum(1, keepdim=True)
    hi = pr64 * torch.exp(e) / (pr64 * torch.exp(-e)).sum(1, keepdim=True)
    prob = float(torch.maximum(pr - hi, lo - pr).clamp(min=0).max() / pr64.max())
    return logit, prob, e


def dec_inputs(N, hw, val, sigma):
    g = torch.Generator().manual_seed(500 + N + hw[0][0] * hw[0][1] + int(sigma))
    l4 = torch.randn(2 * N, *hw[0], generator=g) * sigma
    valid = None
    if val != 'none':
        valid = torch.ones(2, N + 1)
        if val == 'one':
            valid[1, 1 + (N - 1) // 2] = 0
        else:
            valid[:, 1:] = 0
    return l4, valid


def dec_hip(l4, valid, N, hw):
    (h4, w4), (Ho, Wo) = hw
    ld, vd = dv(l4), dv(valid)
    lg, pr, am = Out(2, N + 1, Ho, Wo), Out(2, N + 1, Ho, Wo), Out(2, Ho, Wo, dtype=I64)
    _lib.call('swem_decode_head_f32', ops._stream(), ld.data_ptr(), TE.ptr(vd), lg.ptr(), pr.ptr(), am.ptr(), 2, N, h4, w4, Ho, Wo)
    return lg.t.cpu(), pr.t.cpu(), am.t.cpu(), lg.band() and pr.band() and am.band()


def dec_check(S, hip):
    seen = dict(p_low=0, p_high=0, bg_low=0, bg_high=0, invalid=0)
    left_out = {}
    for N, hw, val, sigma in DEC_CASES:
        l4, valid = dec_inputs(N, hw, val, sigma)
        agg, lg64, pr64 = TE.decode_forward(l4.double(), valid, 2, N, hw[1])
        _, lg32, pr32 = TE.decode_forward(l4, valid, 2, N, hw[1])
        tag = (N, hw[0], val, sigma)
        if sigma > 10:
            p, bg = agg[:, 1:], agg[:, :1]
            for n, t in (('p_low', p < TE.LO32), ('p_high', p > TE.HI32), ('bg_low', bg < TE.LO32), ('bg_high', bg > TE.HI32)):
                seen[n] += int(t.sum())
            seen['invalid'] += 0 if valid is None else int((valid[:, 1:] == 0).sum())
        if hip:
            lg, pr, am, bands = dec_hip(l4, valid, N, hw)
            S.add(tag, 'guard_band', bands)
            S.add(tag, 'argmax_is_the_first_maximum_of_its_own_prob', bool(torch.equal(am, first_argmax(pr))))
        st_l, st_p, e = dec_excess(lg32, pr32, agg, lg64, pr64)
        if hip:
            ex_l, ex_p, _ = dec_excess(lg, pr, agg, lg64, pr64)
            S.add(tag, 'logits', ex_l, 'heads', standin=st_l)
            S.add(tag, 'prob', ex_p, 'heads', standin=st_p)
        else:
            am = first_argmax(pr32)
            # (declared for the 8x rule: the N(0, 40^2) maps -- a bilinear weight's fp32 rounding times a neighbour difference of
            # 100 -- and 8x32 -> 31x125, whose source coordinates round like 27 -> 107's)
            stand_add(S, tag, 'logits', st_l, 'heads', sigma > 10 or hw[0] == (8, 32))
            stand_add(S, tag, 'prob', st_p, 'heads', sigma > 10 or hw[0] == (8, 32))
        top = pr64.topk(2, dim=1)
        clear = (top.values[:, 0] - top.values[:, 1]) > GAP
        if sigma > 10:
            # saturated maps: a clear float64 argmax also needs the top two LOGITS further apart than fp32 can move them (two objects
            # an ulp of 1 - p apart are 0.7 apart in logit and 0.3 in probability, and either may win in fp32)
            l2, e2 = lg64.gather(1, top.indices), e.gather(1, top.indices)
            clear = clear & ((l2[:, 0] - l2[:, 1]) > e2.sum(1))
        S.add(tag, 'argmax_is_float64s_off_ties', bool(torch.equal(am[clear], first_argmax(pr64)[clear])))
        left_out[tag] = round(1 - float(clear.double().mean()), 4)
        if sigma < 10:                      # (the N(0, 40^2) maps tie BY CONSTRUCTION: several objects clamped to the same bound)
            S.add(tag, 'left_out_at_most_1_per_cent', left_out[tag] <= 0.01)
    print('decode head, pixels without a clear float64 argmax: %s' % left_out)
    print('decode head, clamp branches in the N(0, 40^2) references: %s' % seen)
    S.add('all', 'every_clamp_branch_occurs_in_the_reference', min(seen.values()) > 0)


@gpu
def test_decode_head_every_clamp_branch_vs_float64(lib):
    """swem_decode_head_f32 with B = 2, N = 1, 2, 3, 7, three size pairs, valid NULL / with one zero / all zero, logit4 ~ N(0, 4^2)
    and N(0, 40^2) (every clamp branch -- p < 1e-7, p > 1 - 1.19e-7, the same two for the background product, valid = 0 -- occurs
    in the reference: asserted): logits and probabilities against tests/test_gpu_train_edges.py's float64 restatement (8x-stand-in
    rule where fp32 does not resolve 1 - p), the index map EXACTLY the first maximum of the kernel's own prob, and float64's argmax
    wherever float64's top two probabilities are more than 1e-4 apart (at most 1 % of an N(0, 4^2) case is not)."""
    S = sweep('decode_head')
    dec_check(S, True)
    S.finish()


def test_standin_decode_head():
    S = sweep('standin/decode_head', shrink=0.25)
    dec_check(S, False)
    print('declared for the 8x rule (on it where above 5e-6): %s' % S.eight)
    S.finish(record=False)


@gpu
def test_argmax_ties(lib):
    """Constructed ties.  swem_decode_head_f32 on logit4 = 0: p = 1/2 for every valid object, a background / object tie at N = 1
    (and at N = 2 with one object invalid), object / object ties above -- the probabilities tie exactly in any precision, the
    first index wins.  swem_argmax_onehot_i64 on planes quantised to four levels (exact duplicates everywhere), N1 = 1, 2, 8,
    HW = 1, 255, 257, B = 2, with `argmax` only, `onehot` only and both."""
    S = sweep('argmax_ties')
    for N in (1, 2, 3, 7):
        for val in ('none', 'one'):
            hw = DEC_SIZES[1]
            _, valid = dec_inputs(N, hw, val, 4.0)
            l4 = torch.zeros(2 * N, *hw[0])
            _, _, pr64 = TE.decode_forward(l4.double(), valid, 2, N, hw[1])
            want = first_argmax(pr64)
            ties = (pr64 == pr64.amax(1, keepdim=True)).sum(1)
            lg, pr, am, bands = dec_hip(l4, valid, N, hw)
            S.add((N, val), 'reference_ties', bool((ties >= 2)[0].all()) and (N != 1 or bool((want == 0).all())))
            S.add((N, val), 'first_index_wins', bool(torch.equal(am, want)) and bool(torch.equal(am, first_argmax(pr))) and bands)
    g = torch.Generator().manual_seed(520)
    for N1 in (1, 2, 8):
        for HW in (1, 255, 257):
            prob = torch.randint(0, 4, (2, N1, HW), generator=g).float() / 4
            want = first_argmax(prob)
            hot = F.one_hot(want, N1).permute(0, 2, 1).contiguous()
            pd = dv(prob)
            for want_a, want_o in ((1, 0), (0, 1), (1, 1)):
                am, oh = Out(2, HW, dtype=I64), Out(2, N1, HW, dtype=I64)
                _lib.call('swem_argmax_onehot_i64', ops._stream(), pd.data_ptr(), am.ptr() if want_a else 0, oh.ptr() if want_o else 0,
                          2, N1, HW)
                tag = (N1, HW, want_a, want_o)
                S.add(tag, 'argmax', bool(torch.equal(am.t.cpu(), want)) if want_a else am.untouched())
                S.add(tag, 'onehot', bool(torch.equal(oh.t.cpu(), hot)) if want_o else oh.untouched())
                S.add(tag, 'guard_band', am.band() and oh.band())
    S.finish()


# ====================================================================================== 5. movers
def lincomb_check(S, hip):
    g = torch.Generator().manual_seed(530)
    alpha, beta = float(np.float32(0.3)), float(np.float32(0.7))
    for n in (1, 257):
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        for with_b in (1, 0):
            want = alpha * a.double() + (beta * b.double() if with_b else 0)
            if hip:
                ad, bd, y = dv(a), dv(b), Out(n)
                _lib.call('swem_lincomb_f32', ops._stream(), ad.data_ptr(), alpha, bd.data_ptr() if with_b else 0, beta, y.ptr(), n)
                S.add((n, with_b), 'lincomb', rel(y.t, want), 'bilinear')
                S.add((n, with_b), 'guard_band', y.band())
            else:
                S.add((n, with_b), 'lincomb', rel(alpha * a + beta * b if with_b else alpha * a, want), 'bilinear')


@gpu
def test_movers_exact(lib):
    """swem_transpose_f32 (one element; 31 x 33 -> ld 32 and 33 x 31 -> ld 96: a grid sized by the padding; the EM shape 405 x
    128 -> 408; batch 3; pad columns zero), swem_concat2_nhwc_f32 (either source shared), swem_pack_u8_i64 (the 16-wide path, the
    scalar tail, both; values of 256 and above keep their low byte), swem_inject_objects_f32: all exact.  swem_lincomb_f32 against
    float64 at 2e-6."""
    S = sweep('movers')
    st = ops._stream()
    g = torch.Generator().manual_seed(540)
    for R, Cc, ld in ((1, 1, 1), (31, 33, 32), (33, 31, 96), (405, 128, 408)):
        x = torch.randn(3, R, Cc, generator=g)
        xd, y = dv(x), Out(3, Cc, ld)
        _lib.call('swem_transpose_f32', st, xd.data_ptr(), y.ptr(), 3, R, Cc, ld)
        got = y.t.cpu()
        S.add((R, Cc, ld), 'transpose', bool(torch.equal(got[:, :, :R], x.transpose(1, 2)) and (got[:, :, R:] == 0).all()) and y.band())
    for c0, c1 in ((4, 12), (64, 4)):
        for P in (1, 37):
            for sh0, sh1 in ((0, 0), (1, 0), (0, 1)):
                x0, x1 = torch.randn(1 if sh0 else 3, P, c0, generator=g), torch.randn(1 if sh1 else 3, P, c1, generator=g)
                d0, d1, y = dv(x0), dv(x1), Out(3, P, c0 + c1)
                _lib.call('swem_concat2_nhwc_f32', st, d0.data_ptr(), c0, 0 if sh0 else P * c0, d1.data_ptr(), c1, 0 if sh1 else P * c1,
                          y.ptr(), 3, P)
                want = torch.cat([x0.expand(3, P, c0), x1.expand(3, P, c1)], 2)
                S.add((c0, c1, P, sh0, sh1), 'concat2', bool(torch.equal(y.t.cpu(), want)) and y.band())
    for n in (1, 15, 16, 17, 4101):
        x = torch.randint(0, 1000, (n,), generator=g)
        x[0] = 256 + 7
        xd, y = dv(x), Out(n, dtype=U8)
        _lib.call('swem_pack_u8_i64', st, xd.data_ptr(), y.ptr(), n)
        S.add(n, 'pack_u8', bool(np.array_equal(y.t.cpu().numpy(), x.numpy().astype(np.uint8))) and y.band())
    for N1 in (1, 3):
        for Nn1 in (2, 4):
            for HW in (1, 300):
                prob = torch.rand(2, N1, HW, generator=g)
                newm = (torch.rand(2, Nn1, HW, generator=g) < 0.3).float()
                newm[0, 1:, 0] = 0                                           # (both outcomes at HW = 1: batch item 0 keeps its score)
                newm[1, 1, 0] = 1
                want = prob.clone()
                want[(newm[:, 1:].sum(1, keepdim=True) > 0).expand_as(want)] = 0
                want = torch.cat([want, newm[:, 1:]], 1)
                pd, nd, y = dv(prob), dv(newm), Out(2, N1 + Nn1 - 1, HW)
                _lib.call('swem_inject_objects_f32', st, pd.data_ptr(), nd.data_ptr(), y.ptr(), 2, N1, Nn1, HW)
                S.add((N1, Nn1, HW), 'inject_objects', bool(torch.equal(y.t.cpu(), want)) and y.band())
    lincomb_check(S, True)
    S.finish()


def test_standin_lincomb():
    S = sweep('standin/lincomb', shrink=0.25)
    lincomb_check(S, False)
    S.finish(record=False)


# ====================================================================================== CBAM's plane-writing apply kernel
@gpu
def test_cbam_planes_form_is_the_plain_kernel(lib):
    """swem_cbam_f32_planes against swem_cbam_f32 (whose values tests/test_gpu_train_edges.py holds to float64): cbam_apply_planes
    keeps u + u g s as plain C and relies on the compiler contracting it as in cbam_apply_kernel -- y and cscale bit-equal, the
    planes the split kernels' of y, at C = 8, 72, 136 and 1, 30 and 35 pixels (below, and ragged against, the 32-pixel block)."""
    S = sweep('cbam_planes')
    st = ops._stream()
    g = torch.Generator().manual_seed(550)
    for C, hid in ((8, 4), (72, 6), (136, 16)):
        for B, Hh, Ww in ((1, 1, 1), (2, 3, 5), (1, 5, 7)):
            x = nhwc(torch.randn(B, C, Hh, Ww, generator=g))
            par = [dv(torch.randn(*s, generator=g) * f) for s, f in (((hid, C), C ** -0.5), ((hid,), 0.3), ((C, hid), hid ** -0.5), ((C,), 0.3),
                                                                      ((1, 2, 7, 7), 0.3), ((1,), 0.3))]
            wsb = _lib.query('swem_cbam_workspace', B, Hh, Ww, C)
            ws = torch.empty(wsb // 4, device=DEV)
            pp = [p.data_ptr() for p in par]
            cs0, y0 = Out(B, C), Out(B, Hh, Ww, C)
            _lib.call('swem_cbam_f32', st, x.data_ptr(), *pp, cs0.ptr(), y0.ptr(), B, Hh, Ww, C, hid, ws.data_ptr(), wsb)
            S.add((C, B, Hh, Ww), 'guard_band', cs0.band() and y0.band())
            cs = Out(B, C)
            planes_checks(S, (C, B, Hh, Ww), lambda yp, pa: _lib.call('swem_cbam_f32_planes', st, x.data_ptr(), *pp, cs.ptr(), yp, B, Hh, Ww,
                                                                      C, hid, ws.data_ptr(), wsb, *pa), y0.t, B * Hh * Ww, C)
            S.add((C, B, Hh, Ww), 'cscale_bit_equal', biteq(cs.t, cs0.t) and cs.band())
    ops.check_faults()
    S.finish()


# ====================================================================================== 6. refusals
@gpu
def test_refused_calls_leave_their_outputs_untouched(lib):
    """Every refusal below comes with its error code (SWEM_E_SHAPE = -1, SWEM_E_ARG = -4) and BEFORE anything is launched: the
    sentinel-filled outputs are still the sentinel everywhere."""
    st, fault = ops._stream(), ops._fault_ptr(torch.device('cuda', 0))
    x = torch.randn(4096, device=DEV)
    xi = torch.zeros(64, dtype=I64, device=DEV)
    m3, s3 = ops._f3(MEAN), ops._f3(STD)
    am, asd = ctypes.addressof(m3), ctypes.addressof(s3)
    y, pl, y8 = Out(4096), Out(3, 4096, dtype=I16), Out(64, dtype=U8)
    xp, yp, pp = x.data_ptr(), y.ptr(), pl.ptr()
    wsb = _lib.query('swem_cbam_workspace', 1, 2, 2, 12)
    ws = torch.empty(wsb // 4, device=DEV)
    cases = [
        ('maxpool C % 4', -1, 'swem_maxpool3x3s2_nhwc_f32', (xp, yp, 1, 4, 4, 6)),
        ('maxpool_planes C % 8', -1, 'swem_maxpool3x3s2_nhwc_f32_planes', (xp, yp, 1, 4, 4, 12, pp, 3, 0, 3, fault)),
        ('upsample_add_planes C % 8', -1, 'swem_upsample_add_nhwc_f32_planes', (xp, 48, xp, yp, 1, 1, 1, 2, 2, 12, pp, 3, 0, 3, fault)),
        ('cbam_planes C % 8', -1, 'swem_cbam_f32_planes', (xp,) * 7 + (yp, yp + 4096, 1, 2, 2, 12, 4, ws.data_ptr(), wsb, pp, 3, 0, 3, fault)),
        ('s2d odd frame', -1, 'swem_prep_input_s2d_f32', (xp, 0, am, asd, yp, 0, 3, 1, 1, 5, 6, 0, fault)),
        ('s2d nplanes = 5', -4, 'swem_prep_input_s2d_f32', (xp, 0, am, asd, yp, pp, 5, 1, 1, 4, 6, 0, fault)),
        ('resize_planes mode 4', -4, 'swem_resize_planes_f32', (xp, yp, 2, 4, 4, 4, 4, 4)),
        ('flip that changes the size', -1, 'swem_resize_planes_f32', (xp, yp, 2, 4, 4, 4, 5, 3)),
        ('transpose ld < R', -1, 'swem_transpose_f32', (xp, yp, 1, 8, 4, 7)),
        ('pack_u8 n = 0', -4, 'swem_pack_u8_i64', (xi.data_ptr(), y8.ptr(), 0)),
        ('pack_u8 misaligned y', -4, 'swem_pack_u8_i64', (xi.data_ptr(), y8.ptr() + 1, 16)),
        ('inject_objects Nn1 = 1', -4, 'swem_inject_objects_f32', (xp, xp, yp, 1, 2, 1, 16)),
        ('concat2 c0 = 0', -1, 'swem_concat2_nhwc_f32', (xp, 0, 0, xp, 4, 4, yp, 1, 1)),
    ]
    ok = {}
    for what, code, name, args in cases:
        with pytest.raises(_lib.SwemHipError, match=r'%s failed \(%d\)' % (name, code)):
            _lib.call(name, st, *args)
        torch.cuda.synchronize()
        ok[what] = y.untouched() and pl.untouched() and y8.untouched()
        for o in (y, pl, y8):                  # (a case that wrote is not held against the cases behind it)
            o.buf.fill_(o.fill)
    H.record_parity('frame_edges/refusals', {'cases': len(ok), 'outputs_untouched': all(ok.values())})
    assert all(ok.values()), [k for k, v in ok.items() if not v]


# ====================================================================================== what a bar is worth
def test_standin_with_a_dropped_element_misses_the_bars():
    """At the largest case of the resampling, prediction-head and decode-head sweeps: the fp32 stand-in with ONE source pixel
    (resampling, decode head) or ONE filter tap (prediction head) left out, as a multiple of that case's bar (8x the intact
    stand-in where the case is on that rule) -- the bars separate arithmetic from indexing."""
    ratio = {}
    src, dst = PAIRS[4]
    skip, low, _ = up_inputs(src, dst, 72)
    want = skip.double() + interp(low.double(), dst, 'bilinear')
    stand = rel(skip + interp(low, dst, 'bilinear'), want)
    less = low.clone()
    less[1, :, 13, 17] = 0
    bar = 8 * stand if stand > BARS['bilinear'] / 4 else BARS['bilinear']
    ratio['upsample_add 27x31 -> 107x61, C = 72'] = rel(skip + interp(less, dst, 'bilinear'), want) / bar
    C, bhw = PRED_CASES[3]
    x, w, b = pred_inputs(C, bhw)
    want = F.conv2d(F.relu(x.double()), w.double(), b.double(), padding=1)
    less = w.clone()
    less[0, :, 2, 2] = 0
    ratio['pred head 13x61, C = 256'] = rel(F.conv2d(F.relu(x), less, b, padding=1), want) / BARS['heads']
    N, hw, val, sigma = 7, DEC_SIZES[2], 'none', 4.0
    l4, valid = dec_inputs(N, hw, val, sigma)
    agg, lg64, pr64 = TE.decode_forward(l4.double(), valid, 2, N, hw[1])
    less = l4.clone()
    less[9, 4, 16] = 0
    _, lgd, prd = TE.decode_forward(less, valid, 2, N, hw[1])
    ex_l, ex_p, _ = dec_excess(lgd, prd, agg, lg64, pr64)
    ratio['decode head logits 8x32 -> 31x125, N = 7'] = ex_l / BARS['heads']
    ratio['decode head prob 8x32 -> 31x125, N = 7'] = ex_p / BARS['heads']
    print('one dropped element / bar: %s' % {n: round(r, 1) for n, r in ratio.items()})
    assert min(ratio.values()) > 10, ratio
