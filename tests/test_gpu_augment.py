"""GPU: the device augmentation of training clips (swem_amd.augment.ClipAugmenter, csrc/augment.hip) against its float64 numpy
restatement (tests/augment_ref.py, itself anchored to torch's resize in tests/test_augment_host.py).

Labels, region codes, presence sets, masks, label, valid_obj and the count are compared for EQUALITY outside the exclusion set
(pixels whose float64 coordinate lies within 1e-3 px of a threshold).  The image tolerance is measured, not chosen: the
restatement in float32 against float64 on the test's own inputs, times 4 (FMA contraction and another summation order of the 16
taps and 16 TPS terms change roundings, not magnitudes) -- read from profiles/augment_parity.json (tools/augment_parity.py) for
the drawn parity cases, measured in the test for the hand-made parameter blocks.

Measured on an MI355X (max |device - float64| outside the exclusion set, against the bar):
    small_24x40  7.1e-06 / 3.6e-05      small_17x23  7.5e-06 / 4.7e-05      full_384  1.5e-04 / 7.2e-04
    regions  4.4e-06 / 2.0e-05      colour  4.0e-06 / 3.5e-05      identity case against torch's float64 bicubic  2.5e-06 / 3.6e-05"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from swem_amd import augment as A
from tests import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = R.MAX_NOBJ
FIELDS = ('frames', 'masks', 'valid', 'label', 'found')
BARS = json.load(open(os.path.join(os.path.dirname(__file__), '..', 'profiles', 'augment_parity.json')))['cases']


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_device(src, lab, clips, out_hw, max_nobj=N, aug=None):
    B, T = lab.shape[:2]
    aug = aug or A.ClipAugmenter(out_hw, max_nobj, T, device=DEV)
    out = aug(to_dev(src), to_dev(lab), clips)
    res = {k: v.cpu().numpy() for k, v in zip(FIELDS, out)}
    res.update(wlabel=aug.warped_labels(B).cpu().numpy(), region=aug.regions(B).cpu().numpy(),
               presence=aug.presence(B).cpu().numpy())
    return res


def measured_bar(src, lab, clips, max_nobj=N):
    """(float64 restatement, 4 x max |fp32 restatement - float64 restatement| outside the exclusion set) on these inputs."""
    r64, r32 = R.augment(src, lab, clips, max_nobj, np.float64), R.augment(src, lab, clips, max_nobj, np.float32)
    err = np.abs(r32['frames'].astype(np.float64) - r64['frames']).max(axis=2)
    return r64, 4.0 * float(err[~r64['exclude']].max())


def check_against(dev, ref, bar, what):
    """Everything the device returns against the float64 restatement; returns the image error outside the exclusion set."""
    keep = ~ref['exclude']
    frac = ref['exclude'].mean(axis=(2, 3)).max()
    err = np.abs(dev['frames'].astype(np.float64) - ref['frames']).max(axis=2)
    print('%s: excluded %.3f %% of the pixels (worst frame), image max |device - float64| outside = %.3e, bar = %.3e'
          % (what, 100 * frac, err[keep].max(), bar))
    assert frac <= R.EXCLUSION_CAP
    assert np.array_equal(dev['wlabel'][keep], ref['wlabel'][keep]), what
    assert np.array_equal(dev['region'][keep], ref['region'][keep]), what
    assert np.array_equal(dev['presence'], ref['presence']), what
    k5 = np.broadcast_to(keep[:, :, None], ref['masks'].shape)
    assert np.array_equal(dev['masks'][k5], ref['masks'][k5]), what
    assert np.array_equal(dev['label'][keep], ref['label'][keep]), what
    assert np.array_equal(dev['valid'], ref['valid']) and np.array_equal(dev['found'], ref['found']), what
    assert err[keep].max() <= bar, what
    return err[keep].max()


@functools.lru_cache(maxsize=None)
def parity_case(name):
    src, lab, clips = R.drawn_case(name)
    return src, lab, clips, R.augment(src, lab, clips, N, np.float64)


# ------------------------------------------------------------------------------------------- 1. parity with drawn parameters
@pytest.mark.parametrize('name', ['small_24x40', 'small_17x23', 'full_384'])
def test_parity_with_drawn_parameters(name):
    src, lab, clips, ref = parity_case(name)
    blocks = A.pack_params(clips)[:len(clips) * 3 * 64].reshape(-1, 64)
    assert len({b.tobytes() for b in blocks}) == len(blocks)            # a different parameter block per clip and frame
    assert set(np.unique(lab)) <= set(R.LABEL_VALUES) and ref['found'].min() >= 1
    dev = run_device(src, lab, clips, R.CASES[name][4])
    check_against(dev, ref, BARS[name]['bar'], name)
    assert dev['frames'].min() >= 0.0 and dev['frames'].max() <= 1.0    # the bicubic overshoots on white noise; a drawn chain ends in a clamp


# ---------------------------------------------------------------------------------------------- 2. every region on purpose
def test_fill_and_outside_tps_regions():
    src, lab = R.make_inputs(11, 2, 3, (37, 53))
    out_hw = (24, 40)
    base = dict(src_hw=(37, 53), out_hw=out_hw, crop=(2, 4, 30, 44), flip=False, factors=(1.3, 0.8, 1.2),
                order=(A.CONTRAST, A.BRIGHTNESS, A.SATURATION))
    frame = dict(factors=(0.8, 1.2, 0.7), order=(A.SATURATION, A.BRIGHTNESS, A.CONTRAST))
    clips = [dict(base, frames=[dict(frame, angle=15.0, shear=10.0) for _ in range(3)]),
             # every anchor shifted by +0.3 -- the sampler never draws this
             dict(base, flip=True, frames=[dict(frame, angle=0.0, shear=0.0, tps_on=True, tps_Y=A.TPS_ANCHORS + 0.3)
                                           for _ in range(3)])]
    ref, bar = measured_bar(src, lab, clips)
    assert (ref['region'][0] == A.REGION_FILL).mean() >= 0.05
    assert (ref['region'][1] == A.REGION_OUTSIDE_TPS).mean() >= 0.05
    dev = run_device(src, lab, clips, out_hw)
    check_against(dev, ref, bar, 'regions')
    keep = ~ref['exclude']
    # fill pixels: im_mean / 255 through the frame-level ops only (float64, with the frame's own contrast mean)
    fill = (dev['region'] == A.REGION_FILL) & keep
    assert fill[0].sum() >= 0.04 * fill[0].size
    for t in range(3):
        want = R.jitter(np.array(A.IM_MEAN, np.float64)[:, None] / 255, frame['factors'], frame['order'], ref['mean'][0, t],
                        np.float64)[:, 0]
        got = dev['frames'][0, t][:, fill[0, t]]
        assert np.abs(got - want[:, None]).max() <= bar
        assert np.all(got == got[:, :1])                                 # one colour
    assert np.all(dev['wlabel'][fill] == 0)
    # outside-TPS pixels: exactly 0 in image and label, background in the masks
    outside = (dev['region'] == A.REGION_OUTSIDE_TPS) & keep
    assert outside[1].sum() >= 0.04 * outside[1].size
    o5 = np.broadcast_to(outside[:, :, None], dev['frames'].shape)
    assert np.all(dev['frames'][o5] == 0.0) and np.all(dev['wlabel'][outside] == 0) and np.all(dev['label'][outside] == 0)
    assert np.all(dev['masks'][:, :, 0][outside] == 1.0)


# ------------------------------------------------------------------------------------------ 3. independent anchor on the device
def test_identity_case_equals_torch_bicubic_on_the_cpu():
    src, lab = R.make_inputs(4, 1, 1, (37, 53))
    clip = {'out_hw': (24, 40), 'crop': (0, 0, 37, 53), 'flip': False, 'frames': [{'angle': 0.0, 'shear': 0.0}]}
    dev = run_device(src, lab, [clip], (24, 40))
    x = torch.from_numpy(src[0, 0].astype(np.float64) / 255).permute(2, 0, 1)[None]
    want = F.interpolate(x, size=(24, 40), mode='bicubic', align_corners=False)[0].numpy()
    err = np.abs(dev['frames'][0, 0] - want).max()
    print('identity case: max |device - torch float64 bicubic| = %.3e, bar = %.3e' % (err, BARS['small_24x40']['bar']))
    assert err <= BARS['small_24x40']['bar']
    wl = F.interpolate(torch.from_numpy(lab[0, 0].astype(np.float64))[None, None], size=(24, 40), mode='nearest-exact')[0, 0]
    assert np.array_equal(dev['wlabel'][0, 0], wl.numpy().astype(np.uint8)) and not dev['region'].any()


# -------------------------------------------------------------------------------------------------------- 4. object choice
def _prio(first):
    """A priority permutation under which the labels of `first` come first, in that order."""
    order = list(first) + [l for l in range(256) if l not in first]
    prio = np.empty(256, np.int64)
    prio[order] = np.arange(256)
    return prio


def test_object_choice():
    Hs, Ws, out_hw = 36, 54, (24, 40)
    rng = np.random.default_rng(12)
    src = rng.integers(0, 256, size=(4, 3, Hs, Ws, 3), dtype=np.uint8)
    lab = np.zeros((4, 3, Hs, Ws), np.uint8)
    lab[0, 0] = R.block_labels(rng, (Hs, Ws), 6, (0, 255))              # clip 0: nothing in frame 0 ...
    lab[0, 1:] = R.block_labels(rng, (2, Hs, Ws), 6, (0, 3, 255))       # ... label 3 in the later frames only
    lab[1] = R.block_labels(rng, (3, Hs, Ws), 6, (0, 7, 255))           # clip 1: one label
    lab[2] = R.block_labels(rng, (3, Hs, Ws), 6, (0, 3, 7, 12, 20, 31, 255))   # clip 2: five labels, N = 2
    lab[3] = R.block_labels(rng, (3, Hs, Ws), 6, (3, 7))                # clip 3: a label that frame 0 lacks
    lab[3, 0][lab[3, 0] == 7] = 3
    plain = dict(src_hw=(Hs, Ws), out_hw=out_hw, crop=(0, 0, Hs, Ws), flip=False, frames=[{} for _ in range(3)])
    clips = [dict(plain, prio=_prio([3, 255, 0])), dict(plain, prio=_prio([255, 0, 7])),
             dict(plain, prio=_prio([255, 12, 0, 3, 31, 7, 20])), dict(plain, prio=_prio([7, 3]))]
    for b, n in enumerate((0, 1, 5, 1)):
        assert len(set(np.unique(lab[b, 0]).tolist()) - {0, 255}) == n
    ref = R.augment(src, lab, clips, N)
    assert ref['found'].tolist() == [0, 1, 5, 1]
    dev = run_device(src, lab, clips, out_hw)
    assert not ref['exclude'].any()            # (x + 0.5) * 54 / 40 and (y + 0.5) * 36 / 24 stay 0.025 px or more off every integer
    for k in ('wlabel', 'region', 'presence', 'masks', 'label', 'valid', 'found'):
        assert np.array_equal(dev[k], ref[k]), k
    wl = dev['wlabel']
    assert dev['found'].tolist() == [0, 1, 5, 1]
    assert dev['valid'].tolist() == [[1, 1, 0], [1, 1, 0], [1, 1, 1], [1, 1, 0]]
    # none found: all background, also where the later frames carry label 3
    assert (wl[0, 1:] == 3).any() and np.all(dev['masks'][0, :, 0] == 1) and not dev['masks'][0, :, 1:].any()
    # one label
    assert np.array_equal(dev['masks'][1, :, 1], (wl[1] == 7).astype(np.float32)) and not dev['masks'][1, :, 2].any()
    # five labels: the two of lowest priority in priority order; 255 (lowest of all) and 0 are never chosen
    assert np.array_equal(dev['masks'][2, :, 1], (wl[2] == 12).astype(np.float32))
    assert np.array_equal(dev['masks'][2, :, 2], (wl[2] == 3).astype(np.float32))
    assert (wl[2] == 255).any() and np.all(dev['label'][2][wl[2] == 255] == 0)
    # label 7 has the lowest priority but is missing in frame 0: never chosen, its pixels are background
    assert (wl[3, 1:] == 7).any() and np.all(dev['label'][3][wl[3] == 7] == 0) and np.all(dev['masks'][3, :, 0][wl[3] == 7] == 1)
    assert np.array_equal(dev['masks'][3, :, 1], (wl[3] == 3).astype(np.float32))


# ---------------------------------------------------------------------------------------------- 5. colour ops one at a time
def test_colour_ops_one_at_a_time():
    chains = []
    for op in (A.BRIGHTNESS, A.CONTRAST, A.SATURATION):
        for fac in (0.5, 1.5):
            f = [1.0, 1.0, 1.0]
            f[op] = fac
            chains.append(dict(factors=tuple(f), order=(op, A.NO_OP, A.NO_OP)))                # clip-level, alone
            chains.append(dict(frame=dict(factors=tuple(f), order=(A.NO_OP, op, A.NO_OP))))    # frame-level, alone
            chains.append(dict(factors=tuple(f), order=(0, 1, 2)))                              # the others at factor 1
    chains.append(dict(gray=True))
    chains.append(dict(gray=True, factors=(1.5, 0.5, 1.5), order=(1, 2, 0), frame=dict(factors=(1.5, 1.5, 0.5), order=(2, 0, 1))))
    for order in ((0, 1, 2), (2, 1, 0)):                                                        # both op orders
        chains.append(dict(factors=(1.5, 0.5, 1.5), order=order))
        chains.append(dict(frame=dict(factors=(0.5, 1.5, 0.5), order=order)))
    B = len(chains)
    src, lab = R.make_inputs(13, B, 1, (37, 53))
    clips = []
    for c in chains:
        c = dict(c)
        fr = dict(c.pop('frame', {}), angle=12.0, shear=-6.0)             # (with fill pixels: they take the frame-level ops only)
        clips.append(dict(dict(src_hw=(37, 53), out_hw=(17, 23), crop=(1, 3, 33, 47), flip=False, frames=[fr]), **c))
    ref, bar = measured_bar(src, lab, clips)
    dev = run_device(src, lab, clips, (17, 23))
    check_against(dev, ref, bar, 'colour')
    # the ops did what their names say: each chain differs from the uncoloured frame, the clamps engage, gray is gray
    assert all(np.abs(ref['frames'][b] - ref['pre'][b]).max() > 0.05 for b in range(B))
    for b, c in enumerate(chains[:18]):     # one op: a factor of 1.5 pushes white noise past 1 (0.5 on contrast or saturation need not)
        if 1.5 in tuple(c.get('factors', ())) + tuple(c.get('frame', {}).get('factors', ())):
            assert ((ref['frames'][b] == 0) | (ref['frames'][b] == 1)).any(), c
    img = dev['region'][B - 6, 0] == A.REGION_IMAGE
    g = dev['frames'][B - 6, 0][:, img]
    assert np.all(g[0] == g[1]) and np.all(g[1] == g[2])
    # each clip on its own against the float64 chain of its own frame: no clip reads a neighbour's parameters
    per_clip = np.abs(dev['frames'].astype(np.float64) - ref['frames']).max(axis=2)
    for b in range(B):
        assert per_clip[b][~ref['exclude'][b]].max() <= bar, chains[b]


# ------------------------------------------------------------------------------------------------------ 6. reproducibility
def test_eager_calls_and_graph_replays_are_bit_identical():
    src, lab, clips, _ = parity_case('small_24x40')
    other = [A.draw_params(np.random.default_rng(77), 3, (37, 53), (24, 40)) for _ in range(len(clips))]
    s, l = to_dev(src), to_dev(lab)
    aug = A.ClipAugmenter((24, 40), N, 3, device=DEV)
    eager = {}
    for key, p in (('a', clips), ('b', other)):
        first = [t.clone() for t in aug(s, l, p)]
        second = aug(s, l, p)
        assert all(torch.equal(x, y) for x, y in zip(first, second)), key
        eager[key] = first
    assert not torch.equal(eager['a'][0], eager['b'][0])
    # captured once on a single stream, no side branches; the parameters enter through the static buffer
    static = aug.empty_out(len(clips))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        aug(s, l, None, out=static)
    for key, p in (('b', other), ('a', clips), ('b', other)):
        aug.set_params(p)
        for t in static:
            t.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(static, eager[key])), key


# ------------------------------------------------------------------------------------------------------------------ 7. slots
def test_filling_two_slots_of_a_larger_batch_leaves_the_others_alone():
    src, lab, clips, _ = parity_case('small_24x40')
    s, l = to_dev(src), to_dev(lab)
    aug = A.ClipAugmenter((24, 40), N, 3, device=DEV)
    direct = aug(s, l, clips)
    out = aug.empty_out(4)
    for t in out:
        t.fill_(-7)
    got = aug(s, l, clips, out=out, b0=1)
    assert all(g is o for g, o in zip(got, out))
    for name, o, d in zip(FIELDS, out, direct):
        assert torch.equal(o[1:3], d), name
        assert bool((o[0] == -7).all()) and bool((o[3] == -7).all()), name
    with pytest.raises(Exception, match='do not fit'):
        aug(s, l, clips, out=out, b0=3)


# ------------------------------------------------------------------------------------------------------ 8. trainer contract
def test_outputs_are_what_one_step_takes():
    src, lab, clips, _ = parity_case('small_24x40')
    B, T, (Ho, Wo) = 2, 3, (24, 40)
    aug = A.ClipAugmenter((Ho, Wo), N, T, device=DEV)
    frames, masks, valid_obj, label, found = aug(to_dev(src), to_dev(lab), clips)
    for t, shape, dt in ((frames, (B, T, 3, Ho, Wo), torch.float32), (masks, (B, T, N + 1, Ho, Wo), torch.float32),
                         (valid_obj, (B, N + 1), torch.float32), (label, (B, T, Ho, Wo), torch.int64), (found, (B,), torch.int32)):
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous() and t.device == torch.device(DEV)
    assert bool((masks.sum(2) == 1).all()) and bool(((masks == 0) | (masks == 1)).all())
    assert torch.equal(label, masks.argmax(2))
    init_mask = masks[:, 0]
    assert init_mask.data_ptr() == masks.data_ptr() and init_mask._base is masks and tuple(init_mask.shape) == (B, N + 1, Ho, Wo)
    assert float(frames.min()) >= 0.0 and float(frames.max()) <= 1.0       # the drawn chain ends in a clamp
    assert bool(((valid_obj == 0) | (valid_obj == 1)).all()) and bool((valid_obj[:, :2] == 1).all())
