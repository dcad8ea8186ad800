"""Training-clip augmentation on the device (csrc/augment.hip, include/swem_hip_data.h).

The reference augments on CPU workers (datasets/video_dataset.py:139-192, 269-344).  Here the host only draws the random numbers
(`draw_params`, a numpy Generator: no attempt to follow torch's stream) and does the small float64 maths (`tps_coefficients`,
`inverse_affine`, `compose`); `pack_params` lays them out as the 32-bit block the kernels read, and `ClipAugmenter` turns decoded
uint8 frames and label maps into the four tensors of `SWEMTrainer.one_step`.  Parameters are plain data: a caller may hand in any
transform, also ones `draw_params` never draws.
"""
from types import SimpleNamespace

import numpy as np

IM_MEAN = (124, 116, 104)                  # data_utils.py:8, the affine's fill colour


class Rec:
    """The defines and enums of include/swem_hip_data.h without their SWEM_ prefix: record sizes, the first word of each field, the
    flag bits of word STATIC_FLAGS, statistics and placement words (tests/test_abi.py holds the two lists equal)."""
    AUG_MAX_CHANNELS, AUG_FRAME_WORDS, AUG_CLIP_WORDS = 8, 64, 256
    AUG_M_AFF, AUG_M_SRC, AUG_TPS_AFFINE, AUG_TPS_WX, AUG_TPS_WY = 0, 6, 12, 18, 34
    AUG_CLIP_FACTORS, AUG_FRAME_FACTORS, AUG_TPS_ON, AUG_CLIP_ORDER, AUG_GRAY, AUG_FRAME_ORDER = 50, 53, 56, 57, 58, 59
    AUG_STATIC_FLAGS, AUG_SRC_H, AUG_SRC_W, AUG_HUE = 60, 61, 62, 63
    AUG_FLAG_SRC_FILL, AUG_FLAG_HUE_BEFORE_SHIFT, AUG_FLAG_HUE_BEFORE_MASK = 1, 4, 3
    AUG_REGION_IMAGE, AUG_REGION_FILL, AUG_REGION_OUTSIDE_TPS = 0, 1, 2
    SYNTH_MAX_IMAGES, SYNTH_CLIP_WORDS, SYNTH_FRAME_WORDS, SYNTH_STAT_WORDS, SYNTH_PLAN_WORDS = 7, 32, 64, 8, 8
    SYNTH_N_IMG, SYNTH_SIZES, SYNTH_IDS, SYNTH_PASTE, SYNTH_OBJECTS = 0, 2, 16, 0, 8
    SYNTH_STAT_NOT_HMIN, SYNTH_STAT_NOT_WMIN, SYNTH_STAT_HMAX1, SYNTH_STAT_WMAX1 = 0, 1, 2, 3
    SYNTH_STAT_COUNT, SYNTH_STAT_SUM_R, SYNTH_STAT_SUM_G, SYNTH_STAT_SUM_B = 4, 5, 6, 7
    SYNTH_PLAN_RH, SYNTH_PLAN_RW, SYNTH_PLAN_TX, SYNTH_PLAN_TY, SYNTH_PLAN_ID, SYNTH_PLAN_PRESENT = 0, 1, 2, 3, 4, 5


def frame_block_words(B, T):
    """32-bit words of the parameter block of swem_augment_clips_u8 / swem_augment_static_u8: frame records, then label orders."""
    return B * T * Rec.AUG_FRAME_WORDS + B * Rec.AUG_CLIP_WORDS


def synth_block_words(B, T):
    """32-bit words of the parameter block of swem_synth_frames_u8: clip records, then frame records."""
    return B * Rec.SYNTH_CLIP_WORDS + B * T * Rec.SYNTH_FRAME_WORDS


def _align256(n):
    return (n + 255) // 256 * 256


def augment_layout(B, T, Ho, Wo):
    """Byte offsets of the workspace of swem_augment_clips_u8 (aug_layout of csrc/augment.hip): warped labels, region codes,
    presence bits, gray partial sums (one per 32x8 tile), total = swem_augment_workspace."""
    px = B * T * Ho * Wo
    tiles = -(-Wo // 32) * -(-Ho // 8)
    lay = {'wlab': 0, 'wreg': px, 'presence': _align256(2 * px)}
    lay['partial'] = lay['presence'] + _align256(B * 8 * 4)
    lay['total'] = lay['partial'] + _align256(B * T * tiles * 4)
    return lay


def synth_layout(B, T, N):
    """Byte offsets of the workspace of swem_synth_frames_u8 (synth_layout of csrc/synth.hip): statistics, placement table,
    total = swem_synth_workspace."""
    lay = {'stats': 0, 'plan': _align256(B * N * Rec.SYNTH_STAT_WORDS * 4)}
    lay['total'] = lay['plan'] + _align256(B * T * N * Rec.SYNTH_PLAN_WORDS * 4)
    return lay


REGION_IMAGE, REGION_FILL, REGION_OUTSIDE_TPS = Rec.AUG_REGION_IMAGE, Rec.AUG_REGION_FILL, Rec.AUG_REGION_OUTSIDE_TPS
BRIGHTNESS, CONTRAST, SATURATION, NO_OP = 0, 1, 2, 3
TPS_GRID = 4
# the 16 fixed anchors X_k, k = 4*row + column, (x, y) on [-1,1]^2 (thinplatespline/utils.py:13-22)
TPS_ANCHORS = np.stack([np.tile(np.linspace(-1.0, 1.0, TPS_GRID), TPS_GRID),
                        np.repeat(np.linspace(-1.0, 1.0, TPS_GRID), TPS_GRID)], axis=1)
TPS_INNER = [5, 6, 9, 10]


def _tps_kernel(d2):
    return d2 * np.log(d2 + 1e-9)


def tps_coefficients(Y, X=None):
    """(A, W) of the thin-plate spline f with f(X_k) = Y_k: A (3,2) the affine part on (1, x, y), W (16,2) the weights of
    U(|p - X_k|^2), U(d) = d log(d + 1e-9) -- the 19x19 system of thinplatespline/batch.py:69-89, in float64."""
    X = TPS_ANCHORS if X is None else np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    k = X.shape[0]
    L = np.zeros((k + 3, k + 3))
    L[:k, :k] = _tps_kernel(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    L[:k, k] = 1.0
    L[:k, k + 1:] = X
    L[k:, :k] = L[:k, k:].T
    Z = np.zeros((k + 3, 2))
    Z[:k] = Y
    Q = np.linalg.solve(L, Z)
    return Q[k:], Q[:k]


def tps_eval(A, W, pts, X=None):
    """f at points (n,2) of [-1,1]^2, float64."""
    X = TPS_ANCHORS if X is None else np.asarray(X, np.float64)
    pts = np.asarray(pts, np.float64)
    U = _tps_kernel(((pts[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    return A[0] + pts @ A[1:] + U @ W


def affine_forward(angle, shear, out_hw):
    """Rotation by `angle` and x-shear by `shear` (degrees) about the centre (Wo/2, Ho/2), pixel-edge coordinates: 2x3."""
    Ho, Wo = out_hw
    r, s = np.deg2rad(float(angle)), np.deg2rad(float(shear))
    a, b = np.cos(r), -np.cos(r) * np.tan(s) - np.sin(r)
    c, d = np.sin(r), -np.sin(r) * np.tan(s) + np.cos(r)
    lin = np.array([[a, b], [c, d]])
    ctr = np.array([Wo / 2.0, Ho / 2.0])
    return np.concatenate([lin, (ctr - lin @ ctr)[:, None]], axis=1)


def inverse_affine(angle, shear, out_hw):
    """M_aff (2x3): the inverse of `affine_forward`, output pixel -> pre-affine pixel (torchvision's
    _get_inverse_affine_matrix for a rotation and an x-shear about the centre, no translation, unit scale)."""
    Ho, Wo = out_hw
    fwd = affine_forward(angle, shear, out_hw)
    (a, b), (c, d) = fwd[:, :2]          # a*d - b*c = 1
    lin = np.array([[d, -b], [-c, a]])
    ctr = np.array([Wo / 2.0, Ho / 2.0])
    return np.concatenate([lin, (ctr - lin @ ctr)[:, None]], axis=1)


def compose(M_aff, crop, flip, out_hw):
    """M_src (2x3): crop / flip after the affine.  crop = (top, left, ch, cw) in source pixels;
    sx = left + (flip ? Wo - x' : x') * cw / Wo, sy = top + y' * ch / Ho with (x', y') = M_aff (x, y, 1)."""
    Ho, Wo = out_hw
    top, left, ch, cw = [float(v) for v in crop]
    kx, ky = cw / Wo, ch / Ho
    C = np.array([[-kx, 0.0, left + cw], [0.0, ky, top]]) if flip else np.array([[kx, 0.0, left], [0.0, ky, top]])
    M3 = np.concatenate([np.asarray(M_aff, np.float64), [[0.0, 0.0, 1.0]]], axis=0)
    return C @ M3


def _resized_crop(rng, src_hw, scale, ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCrop's box: area fraction U(scale), log-uniform aspect, ten tries, then the centre crop."""
    H, W = src_hw
    for _ in range(10):
        area = H * W * rng.uniform(scale[0], scale[1])
        aspect = np.exp(rng.uniform(np.log(ratio[0]), np.log(ratio[1])))
        w, h = int(round(np.sqrt(area * aspect))), int(round(np.sqrt(area / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
    if W / H < ratio[0]:
        w, h = W, min(H, int(round(W / ratio[0])))
    elif W / H > ratio[1]:
        h, w = H, min(W, int(round(H * ratio[1])))
    else:
        h, w = H, W
    return (H - h) // 2, (W - w) // 2, h, w


def _jitter(rng, b, c, s):
    return ((rng.uniform(1 - b, 1 + b), rng.uniform(1 - c, 1 + c), rng.uniform(1 - s, 1 + s)),
            tuple(int(v) for v in rng.permutation(3)))


def draw_params(rng, T, src_hw, out_hw, is_bl=False):
    """One clip's parameters with the reference's distributions (video_dataset.py:141-191):
    clip level: flip p = 0.5; resized crop, scale (0.36, 1) -- (0.25, 1) for `is_bl` --, ratio (3/4, 4/3); jitter brightness
    0.9-1.1, contrast and saturation 0.97-1.03 in random order; grayscale p = 0.05; the label priority permutation;
    per frame: angle U(-15, 15), x-shear U(-10, 10); jitter 0.99-1.01 in random order; TPS (p = 1) with noise (U - 0.5) * 0.25 on
    the four inner anchors."""
    p = {'src_hw': tuple(src_hw), 'out_hw': tuple(out_hw)}
    p['flip'] = bool(rng.random() < 0.5)
    p['crop'] = _resized_crop(rng, src_hw, (0.25, 1.0) if is_bl else (0.36, 1.0))
    p['factors'], p['order'] = _jitter(rng, 0.1, 0.03, 0.03)
    p['gray'] = bool(rng.random() < 0.05)
    p['prio'] = rng.permutation(256)
    p['frames'] = []
    for _ in range(T):
        f = {'angle': rng.uniform(-15.0, 15.0), 'shear': rng.uniform(-10.0, 10.0)}
        f['factors'], f['order'] = _jitter(rng, 0.01, 0.01, 0.01)
        f['tps_on'] = True
        Y = TPS_ANCHORS.copy()
        Y[TPS_INNER] += (rng.random((4, 2)) - 0.5) * 0.25
        f['tps_Y'] = Y
        p['frames'].append(f)
    return p


def frame_matrices(clip, frame):
    """(M_aff, M_src) of one frame, float64 2x3 on (x, y, 1).  A frame may carry its own 'M_aff' instead of angle / shear, and its
    own 'M_src' instead of the clip's crop / flip (the static chain: `static_frame_matrices`)."""
    M_aff = np.asarray(frame['M_aff'], np.float64) if 'M_aff' in frame else \
        inverse_affine(frame.get('angle', 0.0), frame.get('shear', 0.0), clip['out_hw'])
    if 'M_src' in frame:
        return M_aff, np.asarray(frame['M_src'], np.float64)
    return M_aff, compose(M_aff, clip['crop'], clip['flip'], clip['out_hw'])


def centred(M, out_hw):
    """The 2x3 form on (x, y, 1) as the form on (x - Wo/2, y - Ho/2, 1) the kernels evaluate (small products in fp32)."""
    Ho, Wo = out_hw
    M = np.array(M, np.float64)
    M[:, 2] += M[:, 0] * (Wo / 2.0) + M[:, 1] * (Ho / 2.0)
    return M


def order_code(order):
    """Three op codes (BRIGHTNESS, CONTRAST, SATURATION, NO_OP), first op in the low bits."""
    o = [int(v) for v in order]
    if len(o) != 3 or any(v not in (0, 1, 2, 3) for v in o):
        raise ValueError('an op order is three codes out of 0..3, got %r' % (order,))
    return o[0] | (o[1] << 2) | (o[2] << 4)


def label_order(prio):
    """The labels in the order of their priority: the inverse of the permutation prio[label]."""
    prio = np.asarray(prio)
    if prio.shape != (256,) or sorted(prio.tolist()) != list(range(256)):
        raise ValueError('prio must be a permutation of 0..255')
    return np.argsort(prio, kind='stable').astype(np.int32)


def pack_params(clips):
    """The parameter block of a call (include/swem_hip_data.h) for a list of clip dicts as `draw_params` returns them: an int32
    array of B*T*64 + B*256 words, the fp32 fields bit-cast.  All the maths before the cast to fp32 is float64."""
    B, T = len(clips), len(clips[0]['frames'])
    block = np.zeros(frame_block_words(B, T), np.int32)
    frames = block[:B * T * Rec.AUG_FRAME_WORDS].reshape(B, T, Rec.AUG_FRAME_WORDS)
    orders = block[B * T * Rec.AUG_FRAME_WORDS:].reshape(B, Rec.AUG_CLIP_WORDS)
    for b, clip in enumerate(clips):
        if len(clip['frames']) != T or tuple(clip['out_hw']) != tuple(clips[0]['out_hw']):
            raise ValueError('the clips of one call share T and the output size')
        for t, fr in enumerate(clip['frames']):
            rec = frames[b, t]
            fl = rec.view(np.float32)
            M_aff, M_src = frame_matrices(clip, fr)
            fl[Rec.AUG_M_AFF:Rec.AUG_M_AFF + 6] = centred(M_aff, clip['out_hw']).reshape(-1)
            fl[Rec.AUG_M_SRC:Rec.AUG_M_SRC + 6] = centred(M_src, clip['out_hw']).reshape(-1)
            if fr.get('tps_on', False):
                A, W = tps_coefficients(fr['tps_Y'])
                fl[Rec.AUG_TPS_AFFINE:Rec.AUG_TPS_AFFINE + 6] = A.T.reshape(-1)
                fl[Rec.AUG_TPS_WX:Rec.AUG_TPS_WX + 16] = W[:, 0]
                fl[Rec.AUG_TPS_WY:Rec.AUG_TPS_WY + 16] = W[:, 1]
                rec[Rec.AUG_TPS_ON] = 1
            fl[Rec.AUG_CLIP_FACTORS:Rec.AUG_CLIP_FACTORS + 3] = clip.get('factors', (1.0, 1.0, 1.0))
            fl[Rec.AUG_FRAME_FACTORS:Rec.AUG_FRAME_FACTORS + 3] = fr.get('factors', (1.0, 1.0, 1.0))
            rec[Rec.AUG_CLIP_ORDER] = order_code(clip.get('order', (NO_OP,) * 3))
            rec[Rec.AUG_GRAY] = int(bool(clip.get('gray', False)))
            rec[Rec.AUG_FRAME_ORDER] = order_code(fr.get('order', (NO_OP,) * 3))
        orders[b] = label_order(clip.get('prio', np.arange(256)))
    return block


class StagedBlock:
    """A parameter block of `words` 32-bit words on the device, refilled through pinned memory: `dev`, `pinned` (int32 tensors) and
    `done`, the event behind the last copy out of a pinned block.  Blocks that are refilled together share one event (`done=`):
    all but the last are filled with record=False, so that every copy stands in front of the one event the next refill waits on."""

    def __init__(self, words, device, done=None):
        import torch
        self.device = device
        self.dev = torch.zeros(words, dtype=torch.int32, device=device)
        self.pinned = torch.zeros(words, dtype=torch.int32).pin_memory()
        self.done = torch.cuda.Event() if done is None else done

    def fill(self, block, what='a block', record=True):
        """Copy a numpy block of 32-bit words to the device without blocking; returns the device tensor."""
        import torch
        if block.dtype.itemsize != 4 or block.size != self.pinned.numel():
            raise ValueError('%s has %d 32-bit words, got %d' % (what, self.pinned.numel(), block.size))
        self.done.synchronize()          # (the previous copy out of the pinned block, not the kernels)
        self.pinned.numpy()[:] = block.view(np.int32)
        with torch.cuda.device(self.device):
            self.dev.copy_(self.pinned, non_blocking=True)
            if record:
                self.done.record()
        return self.dev


class ClipAugmenter:
    """callable(frames_u8, labels_u8, params=None, out=None, b0=0) -> (frames, masks, valid_obj, label, found)

    frames_u8 (B,T,Hs,Ws,3) and labels_u8 (B,T,Hs,Ws): decoded uint8 clips on the device.  params: a list of B clip dicts or a
    packed block (staged through pinned memory into the static device buffer of this batch size); None = what the static buffer
    holds (`set_params`; the form to use under graph capture, where the buffer is refilled between replays).  out: the five
    tensors of a batch of Bo >= b0 + B clips to fill at slots b0.. (None: fresh tensors of B clips).
    frames (B,T,3,Ho,Wo) fp32, masks (B,T,N+1,Ho,Wo) fp32 one-hot (init_mask = masks[:, 0]), valid_obj (B,N+1) fp32, label
    (B,T,Ho,Wo) int64: what SWEMTrainer.one_step takes; found (B,) int32: the labels found in frame 0, for the host to read LATER if
    it wants to redraw clips without objects (the reference's five trials) -- nothing here waits for it.
    memset + two launches on the current stream, no host synchronisation."""

    def __init__(self, out_hw, max_nobj, T, device=None):
        import torch
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.N, self.T = int(max_nobj), int(T)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._state = {}      # B -> (workspace, StagedBlock of the frame records and label orders)

    def _buffers(self, B):
        import torch
        from . import _lib
        st = self._state.get(B)
        if st is None:
            Ho, Wo = self.out_hw
            nbytes = _lib.query('swem_augment_workspace', B, self.T, Ho, Wo)
            if nbytes == 0:
                raise _lib.SwemHipError('ClipAugmenter: no workspace for B=%d T=%d %dx%d' % (B, self.T, Ho, Wo))
            st = SimpleNamespace(ws=torch.empty(nbytes, dtype=torch.uint8, device=self.device),
                                 params=StagedBlock(frame_block_words(B, self.T), self.device))
            self._state[B] = st
        return st

    def set_params(self, params, B=None):
        """Copy a parameter block (or pack a list of clip dicts) into the static device buffer of its batch size."""
        block = params if isinstance(params, np.ndarray) else pack_params(params)
        if B is None:
            B = block.size // frame_block_words(1, self.T)
        return self._buffers(B).params.fill(block, 'a block of B=%d, T=%d' % (B, self.T))

    def empty_out(self, B):
        import torch
        (Ho, Wo), T, N, d = self.out_hw, self.T, self.N, self.device
        return (torch.empty((B, T, 3, Ho, Wo), dtype=torch.float32, device=d),
                torch.empty((B, T, N + 1, Ho, Wo), dtype=torch.float32, device=d),
                torch.empty((B, N + 1), dtype=torch.float32, device=d),
                torch.empty((B, T, Ho, Wo), dtype=torch.int64, device=d), torch.empty((B,), dtype=torch.int32, device=d))

    def __call__(self, frames_u8, labels_u8, params=None, out=None, b0=0):
        import torch
        from . import ops
        B = labels_u8.shape[0]
        if labels_u8.shape[1] != self.T:
            raise ValueError('ClipAugmenter was made for T=%d frames, got %d' % (self.T, labels_u8.shape[1]))
        if params is not None:
            self.set_params(params, B)
        st = self._buffers(B)
        if out is None:
            out = self.empty_out(B)
        with torch.cuda.device(self.device):
            ops.augment_clips(frames_u8, labels_u8, st.params.dev, out[0], out[1], out[2], out[3], out[4], st.ws, b0)
        return out

    # ---- what the last call of batch size B left in the workspace (views, for checks)
    def _ws_bytes(self, B, field, nbytes):
        o = augment_layout(B, self.T, *self.out_hw)[field]
        return self._buffers(B).ws[o:o + nbytes]

    def warped_labels(self, B):
        return self._ws_bytes(B, 'wlab', B * self.T * self.out_hw[0] * self.out_hw[1]).view(B, self.T, *self.out_hw)

    def regions(self, B):
        return self._ws_bytes(B, 'wreg', B * self.T * self.out_hw[0] * self.out_hw[1]).view(B, self.T, *self.out_hw)

    def presence(self, B):
        """(B, 256) bool: the labels of the warped frame 0 (0 and 255 are never entered)."""
        import torch
        words = self._ws_bytes(B, 'presence', B * 32).view(torch.int32).view(B, 8)
        return ((words[:, :, None] >> torch.arange(32, device=words.device)) & 1).bool().view(B, 256)


# ------------------------------------------------------------------------------------ stage 0: clips from static images
# (datasets/static_dataset.py; csrc/synth.hip and the static form of csrc/augment.hip)
HUE = 3                                    # the fourth op of the clip-level jitter's drawn order


def static_scale(size0, out_hw):
    """r of Resize(short side -> output) for image 0 of size (h0, w0): max(Ho/h0, Wo/w0)."""
    return max(out_hw[0] / float(size0[0]), out_hw[1] / float(size0[1]))


def draw_static_params(rng, T, sizes, out_hw):
    """One static clip's parameters with the reference's distributions (static_dataset.py:43-79, 112-140, 198-239).  `sizes`: the
    (h_k, w_k) of the n_img images, image 0 first.
    synthesis: the ids, a shuffle of 1..n_img+1 of which the first n_img are used; per frame a paste order and per object fp32
    (area U[0.16, 0.81), aspect log-uniform in [3/4, 4/3], ux, uy U[0, 1));
    clip level: scale s1 U(0.8, 1.5) about the centre, flip p = 0.5; jitter brightness 0.9-1.1, contrast and saturation 0.95-1.05,
    hue +-0.05 in a random order of the four; grayscale p = 0.05; the label priority permutation;
    per frame: angle U(-20, 20), x-shear U(-10, 10), scale s2 U(0.9, 1.1); the crop offset; jitter 0.9-1.1 / 0.95-1.05 / 0.95-1.05
    in random order; TPS (p = 1) with noise (U - 0.5) * 0.3 on the four inner anchors."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    n_img = len(sizes)
    if not 1 <= n_img <= Rec.SYNTH_MAX_IMAGES:
        raise ValueError('a static clip has 1..%d images, got %d' % (Rec.SYNTH_MAX_IMAGES, n_img))
    Ho, Wo = out_hw
    h0, w0 = sizes[0]
    r = static_scale(sizes[0], out_hw)
    p = {'sizes': sizes, 'out_hw': (int(Ho), int(Wo)), 'src_fill': True}
    p['ids'] = [int(v) + 1 for v in rng.permutation(n_img + 1)[:n_img]]
    p['s1'] = rng.uniform(0.8, 1.5)
    p['flip'] = bool(rng.random() < 0.5)
    four = [int(v) for v in rng.permutation(4)]
    p['factors'] = (rng.uniform(0.9, 1.1), rng.uniform(0.95, 1.05), rng.uniform(0.95, 1.05))
    p['hue'] = rng.uniform(-0.05, 0.05)
    p['order'] = tuple(v for v in four if v != HUE)
    p['hue_before'] = four.index(HUE)
    p['gray'] = bool(rng.random() < 0.05)
    p['prio'] = rng.permutation(256)
    p['frames'] = []
    for _ in range(T):
        f = {'angle': rng.uniform(-20.0, 20.0), 'shear': rng.uniform(-10.0, 10.0), 's2': rng.uniform(0.9, 1.1)}
        f['top'] = int(rng.integers(0, max(int(np.floor(r * h0)) - Ho, 0) + 1))
        f['left'] = int(rng.integers(0, max(int(np.floor(r * w0)) - Wo, 0) + 1))
        f['factors'] = (rng.uniform(0.9, 1.1), rng.uniform(0.95, 1.05), rng.uniform(0.95, 1.05))
        f['order'] = tuple(int(v) for v in rng.permutation(3))
        f['tps_on'] = True
        Y = TPS_ANCHORS.copy()
        Y[TPS_INNER] += (rng.random((4, 2)) - 0.5) * 0.3
        f['tps_Y'] = Y
        obj = np.empty((n_img, 4), np.float32)
        obj[:, 0] = rng.uniform(0.16, 0.81, n_img)
        obj[:, 1] = np.exp(rng.uniform(np.log(3.0 / 4.0), np.log(4.0 / 3.0), n_img))
        obj[:, 2:] = rng.random((n_img, 2))
        obj[:, 0] = np.minimum(obj[:, 0], np.nextafter(np.float32(0.81), np.float32(0)))     # (the cast may round up to the bound)
        obj[:, 2:] = np.minimum(obj[:, 2:], np.nextafter(np.float32(1), np.float32(0)))
        f['objects'] = obj
        f['paste'] = [int(v) for v in rng.permutation(n_img)]
        p['frames'].append(f)
    return p


def static_frame_matrices(clip, frame):
    """(M_aff, M_src) of a static frame, float64 2x3 on (x, y, 1) = (u + 0.5, v + 0.5, 1): M_aff maps to
    (px Wo / w0, py Ho / h0), so that the kernel's test against [0, Wo) x [0, Ho) is the test of (px, py) against image 0;
    M_src is the whole map to the source coordinate (sx, sy)."""
    Ho, Wo = clip['out_hw']
    h0, w0 = clip['sizes'][0]
    r = static_scale(clip['sizes'][0], clip['out_hw'])
    c = np.array([w0 / 2.0, h0 / 2.0])
    A2 = np.array([[1.0 / r, 0.0, frame.get('left', 0) / r], [0.0, 1.0 / r, frame.get('top', 0) / r], [0.0, 0.0, 1.0]])
    inv = inverse_affine(frame.get('angle', 0.0), frame.get('shear', 0.0), (h0, w0))
    s2 = float(frame.get('s2', 1.0))
    A3 = np.eye(3)
    A3[:2, :2] = inv[:, :2] / s2
    A3[:2, 2] = c + (inv[:, 2] - c) / s2
    P = A3 @ A2
    F4 = np.array([[-1.0, 0.0, w0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) if clip.get('flip', False) else np.eye(3)
    s1 = float(clip.get('s1', 1.0))
    A5 = np.eye(3)
    A5[:2, :2] /= s1
    A5[:2, 2] = c - c / s1
    return (np.diag([Wo / float(w0), Ho / float(h0), 1.0]) @ P)[:2], (A5 @ F4 @ P)[:2]


def pack_static_params(clips, max_images=None):
    """(synth block, frame block) of a call for a list of clip dicts as `draw_static_params` returns them: two int32 arrays, of
    B*32 + B*T*64 words (include/swem_hip_data.h, the synth record) and of B*T*64 + B*256 words (the frame record with words
    60..63 set).  A missing key means the identity (no scale, no rotation, no hue, ...)."""
    B, T = len(clips), len(clips[0]['frames'])
    full = []
    for clip in clips:
        frames = []
        for fr in clip['frames']:
            M_aff, M_src = static_frame_matrices(clip, fr)
            frames.append(dict(fr, M_aff=M_aff, M_src=M_src))
        full.append(dict(clip, frames=frames))
    block = pack_params(full)
    frames = block[:B * T * Rec.AUG_FRAME_WORDS].reshape(B, T, Rec.AUG_FRAME_WORDS)
    synth = np.zeros(synth_block_words(B, T), np.int32)
    sclips = synth[:B * Rec.SYNTH_CLIP_WORDS].reshape(B, Rec.SYNTH_CLIP_WORDS)
    sframes = synth[B * Rec.SYNTH_CLIP_WORDS:].reshape(B, T, Rec.SYNTH_FRAME_WORDS)
    for b, clip in enumerate(clips):
        sizes = clip['sizes']
        n_img = len(sizes)
        if not 1 <= n_img <= (Rec.SYNTH_MAX_IMAGES if max_images is None else max_images):
            raise ValueError('clip %d has %d images' % (b, n_img))
        before = int(clip.get('hue_before', 0))
        if not 0 <= before <= Rec.AUG_FLAG_HUE_BEFORE_MASK:
            raise ValueError('hue_before counts the clip-level ops in front of the hue op: 0..3')
        sclips[b, Rec.SYNTH_N_IMG] = n_img
        sclips[b, Rec.SYNTH_SIZES:Rec.SYNTH_SIZES + 2 * n_img] = np.asarray(sizes, np.int64).reshape(-1)
        sclips[b, Rec.SYNTH_IDS:Rec.SYNTH_IDS + n_img] = clip.get('ids', list(range(1, n_img + 1)))[:n_img]
        for t, fr in enumerate(clip['frames']):
            rec = frames[b, t]
            rec[Rec.AUG_STATIC_FLAGS] = (Rec.AUG_FLAG_SRC_FILL if clip.get('src_fill', True) else 0) | \
                (before << Rec.AUG_FLAG_HUE_BEFORE_SHIFT)
            rec[Rec.AUG_SRC_H], rec[Rec.AUG_SRC_W] = int(sizes[0][0]), int(sizes[0][1])
            rec.view(np.float32)[Rec.AUG_HUE] = clip.get('hue', 0.0)
            srec = sframes[b, t]
            paste = fr.get('paste', list(range(n_img)))
            srec[Rec.SYNTH_PASTE:Rec.SYNTH_PASTE + len(paste)] = paste
            srec[Rec.SYNTH_PASTE + len(paste):Rec.SYNTH_PASTE + Rec.SYNTH_MAX_IMAGES] = -1
            if n_img > 1 or 'objects' in fr:
                obj = np.asarray(fr['objects'], np.float32).reshape(n_img, 4)
                srec.view(np.float32)[Rec.SYNTH_OBJECTS:Rec.SYNTH_OBJECTS + 4 * n_img] = obj.reshape(-1)
    return synth, block


class StaticClipSynthesizer(ClipAugmenter):
    """callable(imgs_u8, masks_u8, params=None, out=None, b0=0) -> (frames, masks, valid_obj, label, found): stage-0 clips from
    static images, `ClipAugmenter`'s call contract.

    imgs_u8 (B,N,Hmax,Wmax,3) and masks_u8 (B,N,Hmax,Wmax): decoded uint8 images and masks on the device, each at the top left of its
    slot (N = max_nobj, slot_hw = (Hmax, Wmax)); the real sizes travel in the parameters.  params: a list of B clip dicts
    (`draw_static_params`), a pair of packed blocks (`pack_static_params`), or None = what the static buffers hold.
    The composites (B,T,Hmax,Wmax,3) / (B,T,Hmax,Wmax) uint8 stay in this object's buffers (`composites`); statistics and the
    placement table are readable through `stats` / `plan`.  Seven launches (the two clearing ones included; no memset node), no
    host synchronisation, capturable."""

    def __init__(self, out_hw, max_nobj, T, slot_hw, device=None):
        super().__init__(out_hw, max_nobj, T, device)
        self.slot_hw = (int(slot_hw[0]), int(slot_hw[1]))
        if not 1 <= self.N <= Rec.SYNTH_MAX_IMAGES:
            raise ValueError('StaticClipSynthesizer: 1 <= max_nobj <= %d, got %d' % (Rec.SYNTH_MAX_IMAGES, self.N))
        self._synth = {}      # B -> (workspace, StagedBlock of the synth records, comp, comp_lab)

    def _synth_buffers(self, B):
        import torch
        from . import _lib
        st = self._synth.get(B)
        if st is None:
            nbytes = _lib.query('swem_synth_workspace', B, self.T, self.N)
            if nbytes == 0:
                raise _lib.SwemHipError('StaticClipSynthesizer: no workspace for B=%d T=%d N=%d' % (B, self.T, self.N))
            Hm, Wm = self.slot_hw
            st = SimpleNamespace(ws=torch.zeros(nbytes, dtype=torch.uint8, device=self.device),
                                 params=StagedBlock(synth_block_words(B, self.T), self.device, done=self._buffers(B).params.done),
                                 comp=torch.zeros((B, self.T, Hm, Wm, 3), dtype=torch.uint8, device=self.device),
                                 comp_lab=torch.zeros((B, self.T, Hm, Wm), dtype=torch.uint8, device=self.device))
            self._synth[B] = st
        return st

    def set_params(self, params, B=None):
        """Copy a pair of packed blocks (or pack a list of clip dicts) into the static device buffers of its batch size."""
        synth, block = params if isinstance(params, tuple) else pack_static_params(params, self.N)
        if B is None:
            B = block.size // frame_block_words(1, self.T)
        self._synth_buffers(B).params.fill(synth, 'a synth block of B=%d, T=%d' % (B, self.T), record=False)
        return super().set_params(block, B)          # (records the shared event behind both copies)

    def __call__(self, imgs_u8, masks_u8, params=None, out=None, b0=0):
        import torch
        from . import ops
        B = masks_u8.shape[0]
        if tuple(masks_u8.shape[1:]) != (self.N,) + self.slot_hw:
            raise ValueError('StaticClipSynthesizer was made for %d slots of %dx%d, got %s'
                             % ((self.N,) + self.slot_hw + (tuple(masks_u8.shape),)))
        if params is not None:
            self.set_params(params, B)
        syn = self._synth_buffers(B)
        with torch.cuda.device(self.device):
            ops.synth_frames(imgs_u8, masks_u8, syn.params.dev, syn.comp, syn.comp_lab, syn.ws)
        return self.warp(syn.comp, syn.comp_lab, None, out, b0)

    def warp(self, comp, comp_lab, params=None, out=None, b0=0):
        """The second stage alone on given composites (B,T,Hmax,Wmax,3) / (B,T,Hmax,Wmax): the static chain of the parameters."""
        import torch
        from . import ops
        B = comp_lab.shape[0]
        if params is not None:
            self.set_params(params, B)
        st = self._buffers(B)
        if out is None:
            out = self.empty_out(B)
        with torch.cuda.device(self.device):
            ops.augment_static(comp, comp_lab, st.params.dev, out[0], out[1], out[2], out[3], out[4], st.ws, b0)
        return out

    # ---- what the last call of batch size B left behind (views / small copies, for checks)
    def composites(self, B):
        return self._synth_buffers(B).comp, self._synth_buffers(B).comp_lab

    def _synth_words(self, B, field, shape):
        import torch
        o = synth_layout(B, self.T, self.N)[field]
        return self._synth_buffers(B).ws[o:o + 4 * int(np.prod(shape))].view(torch.int32).view(*shape)

    def stats(self, B):
        """(B, N, 8) int64: hmin, wmin, hmax + 1, wmax + 1, count, sum r, sum g, sum b of every image's foreground (the box of
        an empty mask is meaningless: count 0)."""
        import torch
        raw = self._synth_words(B, 'stats', (B, self.N, Rec.SYNTH_STAT_WORDS))
        st = raw.to(torch.int64) & 0xffffffff
        for w in (Rec.SYNTH_STAT_NOT_HMIN, Rec.SYNTH_STAT_NOT_WMIN):
            st[:, :, w] = (~raw[:, :, w]).to(torch.int64) & 0xffffffff
        return st

    def plan(self, B):
        """(B, T, N, 6) int32: rh, rw, tx, ty, id, present of every (frame, object)."""
        return self._synth_words(B, 'plan', (B, self.T, self.N, Rec.SYNTH_PLAN_WORDS))[..., :Rec.SYNTH_PLAN_PRESENT + 1]
