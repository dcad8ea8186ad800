"""J&F (region similarity and boundary accuracy) of DAVIS: numpy/scipy restatement of the reference's fork of the
davis2017 toolkit, ``evaluation/davis2017/metrics.py:6-178`` and ``utils.py:136-162``.

The reference needs ``cv2`` and ``skimage`` (absent here) and ``np.bool`` (removed from NumPy >= 1.24); this file
depends on numpy and scipy.ndimage only.  CPU metric code: it scores index maps, it is not on the GPU path.
KAT: the reference's own ``test_void_masks`` (evaluation/pytest/test_evaluation.py:118-128) in tests/test_metrics.py.

The second half of the file ("on the device") is the GPU path: the same scores from six integers per frame and object that
csrc/metrics.hip counts on the device (include/swem_hip_metrics.h).  The functions above stay the yardstick: the device counts
are tested for equality with theirs (tests/test_gpu_metrics.py), and ``jf_from_counts`` repeats their float64 expressions, so
equal counts give bit-equal J and F.
"""
import math

import numpy as np
from scipy import ndimage


def db_eval_iou(annotation, segmentation, void_pixels=None):
    """metrics.py:6-37: Jaccard index over the last two axes; empty union counts as 1."""
    assert annotation.shape == segmentation.shape
    annotation = annotation.astype(bool)
    segmentation = segmentation.astype(bool)
    void = np.zeros_like(segmentation) if void_pixels is None else void_pixels.astype(bool)
    inters = np.sum((segmentation & annotation) & ~void, axis=(-2, -1))
    union = np.sum((segmentation | annotation) & ~void, axis=(-2, -1))
    with np.errstate(divide='ignore', invalid='ignore'):
        j = inters / union
    if np.ndim(j) == 0:
        return 1 if np.isclose(union, 0) else j
    j[np.isclose(union, 0)] = 1
    return j


def seg2bmap(seg):
    """metrics.py:122-178 for the same-size case: 1-pixel boundaries offset half a pixel towards the origin."""
    seg = seg.astype(bool)
    assert seg.ndim == 2
    e = np.zeros_like(seg)
    s = np.zeros_like(seg)
    se = np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = seg ^ e | seg ^ s | seg ^ se
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = 0
    return b


def disk(radius):
    """skimage.morphology.disk: (2r+1)^2 footprint of the points with x^2 + y^2 <= r^2."""
    r = int(radius)
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (x * x + y * y) <= r * r


def f_measure(foreground_mask, gt_mask, void_pixels=None, bound_th=0.008):
    """metrics.py:57-119: boundary precision/recall with a disk tolerance of bound_th * image diagonal."""
    assert np.atleast_3d(foreground_mask).shape[2] == 1
    void = np.zeros_like(foreground_mask, dtype=bool) if void_pixels is None else void_pixels.astype(bool)
    bound_pix = bound_th if bound_th >= 1 else math.ceil(bound_th * np.linalg.norm(foreground_mask.shape))
    fg_boundary = seg2bmap(foreground_mask * ~void)
    gt_boundary = seg2bmap(gt_mask * ~void)
    fp = disk(bound_pix)
    fg_dil = ndimage.binary_dilation(fg_boundary, structure=fp)      # cv2.dilate with the same footprint
    gt_dil = ndimage.binary_dilation(gt_boundary, structure=fp)
    gt_match = gt_boundary & fg_dil
    fg_match = fg_boundary & gt_dil
    n_fg, n_gt = np.sum(fg_boundary), np.sum(gt_boundary)
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1, 0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0, 1
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1, 1
    else:
        precision = np.sum(fg_match) / float(n_fg)
        recall = np.sum(gt_match) / float(n_gt)
    return 0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)


def db_eval_boundary(annotation, segmentation, void_pixels=None, bound_th=0.008):
    """metrics.py:40-54."""
    assert annotation.shape == segmentation.shape
    if annotation.ndim == 3:
        return np.array([f_measure(segmentation[i], annotation[i], None if void_pixels is None else void_pixels[i],
                                   bound_th=bound_th) for i in range(annotation.shape[0])])
    if annotation.ndim == 2:
        return f_measure(segmentation, annotation, void_pixels, bound_th=bound_th)
    raise ValueError('db_eval_boundary does not support tensors with %d dimensions' % annotation.ndim)


def db_statistics(per_frame_values):
    """utils.py:136-162: mean, recall (> 0.5) and decay (first minus last quarter)."""
    v = np.asarray(per_frame_values, dtype=float)
    with np.errstate(invalid='ignore'):
        M = np.nanmean(v)
        O = np.nanmean(v > 0.5)
        ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.uint8)
        bins = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
        D = np.nanmean(bins[0]) - np.nanmean(bins[3])
    return M, O, D


def evaluate_semisupervised(gt_index_maps, pred_index_maps, num_objects=None):
    """evaluation.py:265-322 for one sequence of the semi-supervised task: index maps (T,H,W) incl. the first and
    the last frame, which the protocol excludes (``[:, 1:-1]``); returns per-object J/F statistics and J&F mean."""
    gt = np.asarray(gt_index_maps)[1:-1]
    pr = np.asarray(pred_index_maps)[1:-1]
    n = int(num_objects if num_objects is not None else gt.max())
    out = {'J': [], 'F': []}
    for o in range(1, n + 1):
        j = db_eval_iou(gt == o, pr == o)
        f = db_eval_boundary(gt == o, pr == o)
        out['J'].append(db_statistics(j))
        out['F'].append(db_statistics(f))
    jm = float(np.mean([s[0] for s in out['J']]))
    fm = float(np.mean([s[0] for s in out['F']]))
    out['J&F-Mean'] = (jm + fm) / 2
    return out


# ---------------------------------------------------------------------------------------------------------------- on the device
COUNTS = ('inter', 'union', 'n_fg', 'n_gt', 'fg_match', 'gt_match')       # include/swem_hip_metrics.h, SWEM_JF_*
G_MEASURES = ('J&F-Mean', 'J-Mean', 'J-Recall', 'J-Decay', 'F-Mean', 'F-Recall', 'F-Decay')      # basic_evaluator.py:290


def bound_pixels(shape, bound_th=0.008):
    """The disk radius of ``f_measure`` for an image of ``shape`` = (H, W) as an int (metrics.py:77-78; host float64)."""
    if bound_th >= 1:
        if bound_th != int(bound_th):
            raise ValueError('bound_th >= 1 is a radius in pixels and must be integral (got %r)' % (bound_th,))
        return int(bound_th)
    return int(math.ceil(bound_th * np.linalg.norm(tuple(int(v) for v in shape))))


def jf_from_counts(counts):
    """(..., 6) integer counts (``COUNTS``) -> (J, F), float64 arrays of shape ``counts.shape[:-1]``: the expressions of
    ``db_eval_iou`` and ``f_measure`` above on their own integers."""
    c = np.asarray(counts)
    assert c.shape[-1] == len(COUNTS) and c.dtype.kind in 'iu'
    c = c.astype(np.int64)
    inters, union = c[..., 0], c[..., 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        j = np.asarray(inters / union, dtype=np.float64)
    j[np.isclose(union, 0)] = 1
    f = np.empty(c.shape[:-1], dtype=np.float64)
    for i in np.ndindex(*c.shape[:-1]):
        n_fg, n_gt, fg_match, gt_match = c[i][2], c[i][3], c[i][4], c[i][5]
        if n_fg == 0 and n_gt > 0:
            precision, recall = 1, 0
        elif n_fg > 0 and n_gt == 0:
            precision, recall = 0, 1
        elif n_fg == 0 and n_gt == 0:
            precision, recall = 1, 1
        else:
            precision = fg_match / float(n_fg)
            recall = gt_match / float(n_gt)
        f[i] = 0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    return j, f


def _index_maps_u8(t, name):
    import torch
    from . import _lib, ops
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 3):
        raise _lib.SwemHipError('%s must be a (T, H, W) device tensor' % name)
    if t.dtype == torch.int64:
        return ops.pack_u8(t.contiguous())
    if t.dtype != torch.uint8:
        raise _lib.SwemHipError('%s must be uint8 or int64 index maps (got %s)' % (name, t.dtype))
    return t.contiguous()


def jf_counts_device(gt, pred, num_objects, void=None, bound_th=0.008):
    """Index maps (T, H, W) on the device, uint8 or int64 (object ids 1..num_objects; ``void``: non-zero = void, shared by all
    objects) -> the int32 device tensor (T, num_objects, 6) of ``COUNTS``.  Three stream-ordered launches on the current stream for
    the whole sequence; nothing synchronises."""
    import torch
    from . import _lib, ops
    with torch.cuda.device(gt.device):
        g = _index_maps_u8(gt, 'gt')
        p = _index_maps_u8(pred, 'pred')
        v = None if void is None else _index_maps_u8(void, 'void')
        if p.shape != g.shape or p.device != g.device or (v is not None and (v.shape != g.shape or v.device != g.device)):
            raise _lib.SwemHipError('jf_counts_device: gt, pred and void must have one shape and device')
        T, H, W = g.shape
        n = int(num_objects)
        r = bound_pixels((H, W), bound_th)
        counts = torch.empty((T, n, len(COUNTS)), dtype=torch.int32, device=g.device)
        nbytes = _lib.query('swem_jf_workspace', T, n, H, W)
        ws = ops.workspace(nbytes, g.device)
        _lib.call('swem_jf_counts_u8', ops._stream(), g.data_ptr(), p.data_ptr(), ops._ptr(v), counts.data_ptr(), T, n, H, W, r,
                  ws.data_ptr(), nbytes)
    return counts


def _sequence_statistics(j, f):
    """evaluation.py:301-316 for one sequence: per-frame J, F of shape (frames, objects) -> the per-object (M, R, D) lists."""
    out = {'J': [], 'F': []}
    for o in range(j.shape[1]):
        out['J'].append(db_statistics(np.ascontiguousarray(j[:, o])))
        out['F'].append(db_statistics(np.ascontiguousarray(f[:, o])))
    return out


def evaluate_semisupervised_device(gt, pred, num_objects=None):
    """``evaluate_semisupervised`` with the counting on the device: (T, H, W) device index maps incl. the first and the last
    frame; the same result dict.  One device-to-host copy (the counts) per sequence; ``num_objects=None`` reads ``gt.max()``
    back first, like the CPU function."""
    if gt.shape[0] < 3:
        raise ValueError('the semi-supervised protocol scores frames [1:-1]: need at least 3 frames')
    n = int(num_objects if num_objects is not None else gt.max())
    counts = jf_counts_device(gt[1:-1], pred[1:-1], n).cpu().numpy()
    out = _sequence_statistics(*jf_from_counts(counts))
    jm = float(np.mean([s[0] for s in out['J']]))
    fm = float(np.mean([s[0] for s in out['F']]))
    out['J&F-Mean'] = (jm + fm) / 2
    return out


class JFMeter:
    """The reference's ``get_metrics()`` (basic_evaluator.py:271-328 -> evaluation.py:265-322) without the PNG round trip:
    ``add`` queues the scoring of a sequence behind the launches that produced its maps and keeps the counts on the device,
    ``results`` synchronises once and returns the global table.  ``stream``: a side stream to score on (the maps' producer
    stream is waited for; inference of the next sequence goes on beside it); default: the current stream."""

    def __init__(self, bound_th=0.008, stream=None):
        self.bound_th = bound_th
        self.stream = stream
        self._seqs = []          # (name, device counts (T-2, N, 6))
        self._streams = []

    def add(self, name, gt, preds, num_objects=None):
        """``preds``: what evaluate_davis_seq / run_sequences / SequencePool.run / LockstepPool.run return for the sequence, a
        list of (1, H, W) int64 device maps for frames 1..T-1; ``gt``: the (T, H, W) annotation (tensor or array, any integer
        type).  The protocol scores frames 1..T-2 (evaluation.py:289-290).  ``num_objects=None``: ``gt.max()`` (read back when
        ``gt`` is on the device)."""
        import torch
        dev = preds[0].device
        gt = torch.as_tensor(gt)
        T = gt.shape[0]
        if T < 3 or len(preds) != T - 1:
            raise ValueError('JFMeter.add: need T >= 3 annotated frames and T - 1 predicted maps (got %d, %d)' % (T, len(preds)))
        n = int(num_objects if num_objects is not None else gt.max())
        if gt.dtype not in (torch.uint8, torch.int64):
            gt = gt.to(torch.int64)
        with torch.cuda.device(dev):
            g = gt[1:T - 1].to(dev)
            p = torch.cat([m.reshape(1, *m.shape[-2:]) for m in preds[:T - 2]], 0)
            cur = torch.cuda.current_stream()
            if self.stream is None or self.stream == cur:
                counts = jf_counts_device(g, p, n, bound_th=self.bound_th)
                st = cur
            else:
                st = self.stream
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    counts = jf_counts_device(g, p, n, bound_th=self.bound_th)
                g.record_stream(st)
                p.record_stream(st)
        if all(st != s for s in self._streams):
            self._streams.append(st)
        self._seqs.append((str(name), counts))

    def results(self):
        """The seven global measures (each the mean over every object of every sequence, basic_evaluator.py:290-294) and
        ``'per_object'``: {'<name>_<i>': {'J-Mean', 'F-Mean'}} (evaluation.py:302-315)."""
        import torch
        if not self._seqs:
            raise ValueError('JFMeter.results: no sequence was added')
        dev = self._seqs[0][1].device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream()
            for st in self._streams:
                if st != cur:
                    cur.wait_stream(st)
            flat = torch.cat([c.reshape(-1) for _, c in self._seqs]).cpu().numpy()      # the one synchronise
        J = {'M': [], 'R': [], 'D': []}
        F = {'M': [], 'R': [], 'D': []}
        per_object = {}
        at = 0
        for name, c in self._seqs:
            counts = flat[at:at + c.numel()].reshape(tuple(c.shape))
            at += c.numel()
            st = _sequence_statistics(*jf_from_counts(counts))
            for i in range(c.shape[1]):
                for acc, (m, r, d) in ((J, st['J'][i]), (F, st['F'][i])):
                    acc['M'].append(m)
                    acc['R'].append(r)
                    acc['D'].append(d)
                per_object['%s_%d' % (name, i + 1)] = {'J-Mean': st['J'][i][0], 'F-Mean': st['F'][i][0]}
        final_mean = (np.mean(J['M']) + np.mean(F['M'])) / 2.
        values = [final_mean, np.mean(J['M']), np.mean(J['R']), np.mean(J['D']), np.mean(F['M']), np.mean(F['R']), np.mean(F['D'])]
        out = {k: float(v) for k, v in zip(G_MEASURES, values)}
        out['per_object'] = per_object
        return out
