"""GPU: J&F scored on the device (csrc/metrics.hip, swem_amd.metrics "on the device") against the CPU metric of the same file.

The yardstick is ``swem_amd/metrics.py``'s numpy / scipy code (pinned by the reference toolkit's known-answer test in
tests/test_metrics.py), never the device path.  Every comparison is integer or float64 EQUALITY: the six counts per frame and
object are integers, and ``jf_from_counts`` repeats the CPU functions' float64 expressions on them."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from swem_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ------------------------------------------------------------------------------------------------ generator and CPU yardstick
def make_maps(T, H, W, N, seed, roll=(5, -7), flip=2e-4):
    """Seeded index maps (T, H, W) uint8: warped ellipses that move over the frames (later ids occlude earlier ones); the
    prediction is the ground truth rolled by a few pixels plus sparse flipped pixels."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    par = [(rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, max(1.0, rng.uniform(0.10, 0.22) * H),
            max(1.0, rng.uniform(0.08, 0.2) * W), rng.uniform(0, 6.28), rng.uniform(-2, 2), rng.uniform(-3, 3)) for _ in range(N)]
    gt = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        for o, (cy, cx, b, a, ph, vy, vx) in enumerate(par, 1):
            v = yy - (cy + vy * t) + 0.2 * b * np.sin((xx - cx) / a * 2.0 + ph)
            u = xx - (cx + vx * t) + 0.2 * a * np.sin((yy - cy) / b * 2.0 + ph + t * 0.3)
            gt[t][(u / a) ** 2 + (v / b) ** 2 <= 1.0] = o
    pred = np.roll(gt, roll, axis=(1, 2))
    k = int(round(flip * H * W))
    for t in range(T):
        ys, xs = rng.randint(0, H, k), rng.randint(0, W, k)
        pred[t, ys, xs] = rng.randint(0, N + 1, k)
    return gt, pred


def cpu_counts(gt, pred, N, void=None, bound_th=0.008):
    """The six integers of every frame and object with the CPU metric's own building blocks (f_measure's lines, metrics.py)."""
    T, H, W = gt.shape
    fp = M.disk(bound_th if bound_th >= 1 else int(np.ceil(bound_th * np.linalg.norm((H, W)))))
    out = np.zeros((T, N, 6), np.int64)
    for t in range(T):
        v = np.zeros((H, W), bool) if void is None else void[t].astype(bool)
        for o in range(1, N + 1):
            s, g = (pred[t] == o) & ~v, (gt[t] == o) & ~v
            bs, bg = M.seg2bmap(s), M.seg2bmap(g)
            ds, dg = ndimage.binary_dilation(bs, structure=fp), ndimage.binary_dilation(bg, structure=fp)
            out[t, o - 1] = [(s & g).sum(), (s | g).sum(), bs.sum(), bg.sum(), (bs & dg).sum(), (bg & ds).sum()]
    return out


def device_counts(gt, pred, N, void=None, bound_th=0.008):
    c = M.jf_counts_device(torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV), N,
                           void=None if void is None else torch.from_numpy(void).to(DEV), bound_th=bound_th)
    assert c.dtype == torch.int32 and tuple(c.shape) == (gt.shape[0], N, 6) and c.is_cuda
    return c.cpu().numpy().astype(np.int64)


def flagship_case():
    """480x854, T = 6, N = 3, with an object absent from a frame in the prediction only, in the annotation only and in both."""
    gt, pred = make_maps(6, 480, 854, 3, seed=1)
    pred[1][pred[1] == 2] = 0
    gt[2][gt[2] == 3] = 0
    gt[3][gt[3] == 1] = 0
    pred[3][pred[3] == 1] = 0
    return gt, pred


def assert_counts_equal(dev, cpu, what):
    bad = np.argwhere(dev != cpu)
    assert bad.size == 0, '%s: %d of %d counts differ, first at (frame, object, count) %s: device %d, CPU %d' % (
        what, len(bad), cpu.size, tuple(bad[0]), dev[tuple(bad[0])], cpu[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------------------------- tests
def test_counts_equal_cpu_flagship_shape(lib):
    gt, pred = flagship_case()
    cpu = cpu_counts(gt, pred, 3)
    # the case is not vacuous: partial matches in both directions, and all three kinds of absent object
    n_fg, n_gt, fg_m, gt_m = cpu[..., 2], cpu[..., 3], cpu[..., 4], cpu[..., 5]
    assert ((0 < fg_m) & (fg_m < n_fg)).any() and ((0 < gt_m) & (gt_m < n_gt)).any()
    has_p = np.array([[(pred[t] == o).any() for o in (1, 2, 3)] for t in range(6)])
    has_g = np.array([[(gt[t] == o).any() for o in (1, 2, 3)] for t in range(6)])
    assert (~has_p & has_g).any() and (has_p & ~has_g).any() and (~has_p & ~has_g).any() and (has_p & has_g).any()
    print('480x854 CPU counts, frame 0 object 1 (inter, union, n_fg, n_gt, fg_match, gt_match):', cpu[0, 0].tolist())
    assert_counts_equal(device_counts(gt, pred, 3), cpu, '480x854')


@pytest.mark.parametrize('T,H,W,N', [(3, 480, 864, 2), (3, 200, 200, 2), (3, 33, 70, 2), (3, 64, 64, 2), (3, 65, 129, 2),
                                     (3, 7, 5, 1), (3, 1, 300, 1), (3, 300, 1, 1), (3, 200, 200, 1), (3, 200, 200, 10)],
                         ids=lambda v: str(v))
def test_counts_equal_cpu_shapes(lib, T, H, W, N):
    """Word edges (64, 65, 129 columns), an image smaller than the disk, single rows and columns, one and ten objects."""
    gt, pred = make_maps(T, H, W, N, seed=H * 1000 + W + N, roll=(min(2, H - 1), -min(3, W - 1)))
    dev = device_counts(gt, pred, N)
    assert_counts_equal(dev, cpu_counts(gt, pred, N), '%dx%d N=%d' % (H, W, N))
    # ... and the scores against the CPU functions themselves, not only against their building blocks
    j, f = M.jf_from_counts(dev)
    for t in range(T):
        for o in range(1, N + 1):
            assert j[t, o - 1] == M.db_eval_iou(gt[t] == o, pred[t] == o), (t, o)
            assert f[t, o - 1] == M.f_measure(pred[t] == o, gt[t] == o), (t, o)


def test_borders_full_frame_and_foreign_ids(lib):
    """_seg2bmap's last-row / last-column / corner rules: objects on all four borders, a mask that is the whole frame, and
    an id above N in both maps (ignored, as `map == o` ignores it)."""
    H, W = 96, 150
    gt = np.zeros((4, H, W), np.uint8)
    gt[0, :20, :30] = 1            # top-left corner
    gt[0, -25:, -40:] = 2          # bottom-right corner
    gt[1, :, :7] = 1               # the whole left border
    gt[1, -3:, :] = 2              # the whole last rows
    gt[2] = 1                      # the full frame
    gt[3, :5, :] = 1               # the whole top rows
    gt[3, :, -2:] = 2              # the whole last columns
    pred = np.roll(gt, (2, 3), axis=(1, 2))
    pred[2] = 1
    pred[0, 40:50, 60:70] = 7      # ids above N
    gt[0, 42:52, 62:80] = 200
    assert_counts_equal(device_counts(gt, pred, 2), cpu_counts(gt, pred, 2), 'borders')
    full = cpu_counts(gt, pred, 2)[2, 0]
    assert full.tolist() == [H * W, H * W, 0, 0, 0, 0]      # a full frame has no boundary at all


@pytest.mark.parametrize('r', [1, 3, 8])
def test_matches_equal_brute_force(lib, r):
    """Independent of scipy: a boundary pixel matches iff a boundary pixel of the other map lies at squared distance <= r*r."""
    gt, pred = make_maps(2, 48, 80, 2, seed=77 + r, roll=(3, -4), flip=2e-3)
    dev = device_counts(gt, pred, 2, bound_th=r)
    for t in range(2):
        for o in (1, 2):
            bf, bg = np.argwhere(M.seg2bmap(pred[t] == o)), np.argwhere(M.seg2bmap(gt[t] == o))
            d2 = ((bf[:, None, :] - bg[None, :, :]) ** 2).sum(-1)
            fg_match = int((d2 <= r * r).any(1).sum()) if len(bg) else 0
            gt_match = int((d2 <= r * r).any(0).sum()) if len(bf) else 0
            assert len(bf) and len(bg)
            assert dev[t, o - 1, 2:].tolist() == [len(bf), len(bg), fg_match, gt_match], (t, o)


def test_void_masks_kat_on_the_device(lib):
    """The reference toolkit's known-answer test (evaluation/pytest/test_evaluation.py:118-128) through the device path."""
    gt = np.zeros((2, 200, 200), np.uint8)
    mask = np.zeros((2, 200, 200), np.uint8)
    void = np.zeros((2, 200, 200), np.uint8)
    gt[:, 100:150, 100:150] = 1
    void[:, 50:100, 100:150] = 1
    mask[:, 50:150, 100:150] = 1
    counts = device_counts(gt, mask, 1, void=void)
    j, f = M.jf_from_counts(counts)
    assert np.mean(j) == 1 and np.mean(f) == 1
    assert_counts_equal(counts, cpu_counts(gt, mask, 1, void=void), 'void KAT')


def test_evaluate_semisupervised_device_equals_cpu(lib):
    gt, pred = make_maps(12, 240, 432, 2, seed=5, roll=(4, -6), flip=5e-4)
    cpu = M.evaluate_semisupervised(gt, pred)
    for dtype in (torch.uint8, torch.int64):
        dev = M.evaluate_semisupervised_device(torch.from_numpy(gt).to(DEV, dtype), torch.from_numpy(pred).to(DEV, dtype))
        assert sorted(dev) == sorted(cpu) == ['F', 'J', 'J&F-Mean']
        assert dev['J&F-Mean'] == cpu['J&F-Mean'] and 0.3 < cpu['J&F-Mean'] < 1.0
        for k in ('J', 'F'):
            assert len(dev[k]) == len(cpu[k]) == 2
            for a, b in zip(dev[k], cpu[k]):
                assert tuple(a) == tuple(b), (k, a, b)


def test_meter_end_to_end(lib):
    """A short clip through evaluate_davis_seq, scored against a synthetic annotation by JFMeter (current stream and fed from a
    side stream) and by the CPU functions on the copied-back maps."""
    from oracle import swem_oracle as O
    from swem_amd import evaluator, synth
    from tests import helpers as H
    cfg = O.make_cfg(BACKBONE='resnet18', NUM_BASES=64, NUM_EM_ITERS=4, SINGLE_OBJ=False)
    model, _ = H.make_model_and_sd(cfg, wseed=3, device=DEV)
    clips = []
    for s in (2, 9):
        frames, masks = synth.make_clip(t=6, h=128, w=192, n_obj=2, seed=s, all_masks=True)
        clips.append(('clip%d' % s, frames.to(DEV), masks[0].to(DEV), torch.cat([m.argmax(1) for m in masks], 0)))
    side = torch.cuda.Stream()
    meters = [M.JFMeter(), M.JFMeter(stream=side)]
    maps = []
    with torch.no_grad():
        for name, frames, m0, gt in clips:
            preds, _ = evaluator.evaluate_davis_seq(model, frames, [m0] + [None] * 5, (128, 192))
            assert len(preds) == 5 and preds[0].shape == (1, 128, 192)
            meters[0].add(name, gt, preds)
            meters[1].add(name, gt.to(DEV), preds, num_objects=2)
            maps.append((name, gt.numpy(), torch.cat(preds, 0).cpu().numpy()))
    # a third sequence with scores away from 0 (the seeded random weights above predict little of the annotation): generator maps
    # in the shape the evaluator returns them
    gt3, pred3 = make_maps(6, 128, 192, 2, seed=8, roll=(1, -1), flip=1e-3)
    preds3 = [torch.from_numpy(pred3[i:i + 1].astype(np.int64)).to(DEV) for i in range(1, 6)]
    for m in meters:
        m.add('maps', gt3, preds3)
    maps.append(('maps', gt3, pred3[1:]))
    got = [m.results() for m in meters]
    # the CPU side: evaluation.py:301-316 and basic_evaluator.py:290-294 with the CPU metric
    J, F, per = {'M': [], 'R': [], 'D': []}, {'M': [], 'R': [], 'D': []}, {}
    for name, gt, pr in maps:
        g, p = gt[1:-1], pr[:-1]                  # frames 1..T-2; preds[0] is frame 1
        for o in (1, 2):
            js, fs = M.db_statistics(M.db_eval_iou(g == o, p == o)), M.db_statistics(M.db_eval_boundary(g == o, p == o))
            for acc, st in ((J, js), (F, fs)):
                for key, v in zip('MRD', st):
                    acc[key].append(v)
            per['%s_%d' % (name, o)] = {'J-Mean': js[0], 'F-Mean': fs[0]}
    want = {'J&F-Mean': (np.mean(J['M']) + np.mean(F['M'])) / 2., 'J-Mean': np.mean(J['M']), 'J-Recall': np.mean(J['R']),
            'J-Decay': np.mean(J['D']), 'F-Mean': np.mean(F['M']), 'F-Recall': np.mean(F['R']), 'F-Decay': np.mean(F['D'])}
    print('JFMeter:', {k: got[0][k] for k in M.G_MEASURES})
    for res in got:
        assert sorted(res) == sorted(list(want) + ['per_object'])
        for k in M.G_MEASURES:
            assert res[k] == want[k], (k, res[k], want[k])
        assert res['per_object'] == per and len(per) == 6
    assert want['J-Recall'] > 0 and want['F-Recall'] > 0 and 0 < want['J&F-Mean'] < 1
    assert got[0] == got[1]
