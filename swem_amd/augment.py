"""Training-clip augmentation on the device (csrc/augment.hip, include/swem_hip_data.h).

The reference augments on CPU workers (datasets/video_dataset.py:139-192, 269-344).  Here the host only draws the random numbers
(`draw_params`, a numpy Generator: no attempt to follow torch's stream) and does the small float64 maths (`tps_coefficients`,
`inverse_affine`, `compose`); `pack_params` lays them out as the 32-bit block the kernels read, and `ClipAugmenter` turns decoded
uint8 frames and label maps into the four tensors of `SWEMTrainer.one_step`.  Parameters are plain data: a caller may hand in any
transform, also ones `draw_params` never draws.
"""
import numpy as np

IM_MEAN = (124, 116, 104)                  # data_utils.py:8, the affine's fill colour
FRAME_WORDS, CLIP_WORDS = 64, 256          # include/swem_hip_data.h
REGION_IMAGE, REGION_FILL, REGION_OUTSIDE_TPS = 0, 1, 2
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
    """(M_aff, M_src) of one frame, float64 2x3 on (x, y, 1).  A frame may carry its own 'M_aff' instead of angle / shear."""
    M_aff = np.asarray(frame['M_aff'], np.float64) if 'M_aff' in frame else \
        inverse_affine(frame.get('angle', 0.0), frame.get('shear', 0.0), clip['out_hw'])
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
    block = np.zeros(B * T * FRAME_WORDS + B * CLIP_WORDS, np.int32)
    fl = block.view(np.float32)
    for b, clip in enumerate(clips):
        if len(clip['frames']) != T or tuple(clip['out_hw']) != tuple(clips[0]['out_hw']):
            raise ValueError('the clips of one call share T and the output size')
        for t, fr in enumerate(clip['frames']):
            o = (b * T + t) * FRAME_WORDS
            M_aff, M_src = frame_matrices(clip, fr)
            fl[o:o + 6] = centred(M_aff, clip['out_hw']).reshape(-1)
            fl[o + 6:o + 12] = centred(M_src, clip['out_hw']).reshape(-1)
            if fr.get('tps_on', False):
                A, W = tps_coefficients(fr['tps_Y'])
                fl[o + 12:o + 18] = A.T.reshape(-1)
                fl[o + 18:o + 34] = W[:, 0]
                fl[o + 34:o + 50] = W[:, 1]
                block[o + 56] = 1
            fl[o + 50:o + 53] = clip.get('factors', (1.0, 1.0, 1.0))
            fl[o + 53:o + 56] = fr.get('factors', (1.0, 1.0, 1.0))
            block[o + 57] = order_code(clip.get('order', (NO_OP,) * 3))
            block[o + 58] = int(bool(clip.get('gray', False)))
            block[o + 59] = order_code(fr.get('order', (NO_OP,) * 3))
        o = B * T * FRAME_WORDS + b * CLIP_WORDS
        block[o:o + CLIP_WORDS] = label_order(clip.get('prio', np.arange(256)))
    return block


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
        self._state = {}      # B -> (workspace, device block, pinned block, copy-done event)

    def _buffers(self, B):
        import torch
        from . import _lib
        st = self._state.get(B)
        if st is None:
            Ho, Wo = self.out_hw
            nbytes = _lib.query('swem_augment_workspace', B, self.T, Ho, Wo)
            if nbytes == 0:
                raise _lib.SwemHipError('ClipAugmenter: no workspace for B=%d T=%d %dx%d' % (B, self.T, Ho, Wo))
            words = B * self.T * FRAME_WORDS + B * CLIP_WORDS
            st = (torch.empty(nbytes, dtype=torch.uint8, device=self.device),
                  torch.zeros(words, dtype=torch.int32, device=self.device),
                  torch.zeros(words, dtype=torch.int32).pin_memory(), torch.cuda.Event())
            self._state[B] = st
        return st

    def set_params(self, params, B=None):
        """Copy a parameter block (or pack a list of clip dicts) into the static device buffer of its batch size."""
        import torch
        block = params if isinstance(params, np.ndarray) else pack_params(params)
        if B is None:
            B = block.size // (self.T * FRAME_WORDS + CLIP_WORDS)
        _ws, dev, pinned, done = self._buffers(B)
        if block.dtype.itemsize != 4 or block.size != pinned.numel():
            raise ValueError('a block of B=%d, T=%d has %d 32-bit words, got %d' % (B, self.T, pinned.numel(), block.size))
        done.synchronize()          # (the previous copy out of the pinned block, not the kernels)
        pinned.numpy()[:] = block.view(np.int32)
        with torch.cuda.device(self.device):
            dev.copy_(pinned, non_blocking=True)
            done.record()
        return dev

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
        ws, dev, _pinned, _done = self._buffers(B)
        if out is None:
            out = self.empty_out(B)
        with torch.cuda.device(self.device):
            ops.augment_clips(frames_u8, labels_u8, dev, out[0], out[1], out[2], out[3], out[4], ws, b0)
        return out

    # ---- what the last call of batch size B left in the workspace (views, for checks)
    def _px(self, B):
        return B * self.T * self.out_hw[0] * self.out_hw[1]

    def warped_labels(self, B):
        return self._buffers(B)[0][:self._px(B)].view(B, self.T, *self.out_hw)

    def regions(self, B):
        return self._buffers(B)[0][self._px(B):2 * self._px(B)].view(B, self.T, *self.out_hw)

    def presence(self, B):
        """(B, 256) bool: the labels of the warped frame 0 (0 and 255 are never entered)."""
        import torch
        o = (2 * self._px(B) + 255) // 256 * 256
        words = self._buffers(B)[0][o:o + B * 32].view(torch.int32).view(B, 8)
        return ((words[:, :, None] >> torch.arange(32, device=words.device)) & 1).bool().view(B, 256)
