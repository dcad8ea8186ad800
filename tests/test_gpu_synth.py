"""GPU: stage-0 training clips from static images (swem_amd.augment.StaticClipSynthesizer; csrc/synth.hip and the static form of
csrc/augment.hip) against the float64 numpy restatement tests/synth_ref.py (pinned to torch's resize, colorsys and section 8's
identity case in tests/test_synth_host.py).

Statistics and the placement table are EQUAL.  Composite labels and colours are EQUAL outside the pixels whose float64 colour lies
within 1e-3 of k + 0.5 (mask coordinates and rectangle edges are integer arithmetic on both sides: nothing to exclude).  The
static chain is checked on the DEVICE's composites: labels, region codes, presence, masks, label, valid_obj and the count EQUAL
outside section 8's exclusion set extended by the source bounds; the image within the measured bar -- the restatement in float32
against float64 on the test's own inputs, times 4: read from profiles/synth_parity.json (tools/synth_parity.py) for the drawn
cases, measured in the test for the hand-made parameter blocks.  Both exclusion sets stay under 3 % of a frame.

Measured on an MI355X (max |device - float64| outside the exclusion set, against the bar):
    n2_24x40  9.9e-06 / 5.7e-05      n3_17x23  7.9e-06 / 4.2e-05      fill regions  3.1e-06 / 2.5e-05      identity  2.6e-06 / 1.1e-05
    hue  7.6e-06 / 3.1e-05      seven images  7.5e-06 / 5.5e-05      composite bytes differing, inside the exclusion set included: 0"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from swem_amd import _lib, augment as A
from tests import augment_ref as R
from tests import synth_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIELDS = ('frames', 'masks', 'valid', 'label', 'found')
BARS = json.load(open(os.path.join(os.path.dirname(__file__), '..', 'profiles', 'synth_parity.json')))['cases']
SIZES3 = [(37, 53), (29, 41), (45, 33)]


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_device(imgs, masks, clips, out_hw, N, syn=None):
    B, T = len(clips), len(clips[0]['frames'])
    syn = syn or A.StaticClipSynthesizer(out_hw, N, T, imgs.shape[2:4], device=DEV)
    out = syn(to_dev(imgs), to_dev(masks), clips)
    res = {k: v.cpu().numpy() for k, v in zip(FIELDS, out)}
    comp, comp_lab = syn.composites(B)
    res.update(wlabel=syn.warped_labels(B).cpu().numpy(), region=syn.regions(B).cpu().numpy(),
               presence=syn.presence(B).cpu().numpy(), comp=comp.cpu().numpy(), comp_lab=comp_lab.cpu().numpy(),
               stats=syn.stats(B).cpu().numpy(), plan=syn.plan(B).cpu().numpy())
    return res


def check_stats_and_plan(dev, cref, clips, N, what):
    for b, (c, clip) in enumerate(zip(cref, clips)):
        want = S.stats_table(c['stats'], N)
        got = dev['stats'][b]
        assert np.array_equal(got[:, 4:], want[:, 4:]), (what, b)
        has = want[:, 4] > 0
        assert np.array_equal(got[has, :4], want[has, :4]), (what, b)
        if c['plan'] is not None:
            n = len(clip['sizes'])
            assert np.array_equal(dev['plan'][b][:, :n], c['plan']), (what, b)
            assert not dev['plan'][b][:, n:, 5].any()
            raw = np.array(c['raw_sizes'])
            assert raw.size == 0 or np.abs(raw - np.floor(raw) - 0.5).min() >= S.HALF_MARGIN


def check_composite(dev, cref, clips, what):
    """Labels and colours EQUAL outside the exclusion set; returns the number of bytes that differ inside it."""
    inside = 0
    for b, (c, clip) in enumerate(zip(cref, clips)):
        h0, w0 = clip['sizes'][0]
        keep = ~c['exclude']
        frac = c['exclude'].mean(axis=(1, 2)).max()
        assert frac <= S.EXCLUSION_CAP, (what, b, frac)
        got, lab = dev['comp'][b][:, :h0, :w0], dev['comp_lab'][b][:, :h0, :w0]
        assert np.array_equal(lab, c['labels']), (what, b)                     # (labels: integer arithmetic, no exclusion needed)
        assert np.array_equal(got[keep], c['frames'][keep]), (what, b)
        inside += int((got != c['frames']).sum())
    return inside


def chain_reference(dev, clips, N, bar=None):
    """The float64 static chain on the DEVICE's composites, and the bar (measured on these inputs unless given)."""
    r64 = S.static_batch(dev['comp'], dev['comp_lab'], clips, N, np.float64)
    if bar is None:
        r32 = S.static_batch(dev['comp'], dev['comp_lab'], clips, N, np.float32)
        err = np.abs(r32['frames'].astype(np.float64) - r64['frames']).max(axis=2)
        bar = 4.0 * float(err[~r64['exclude']].max())
    return r64, bar


def check_chain(dev, ref, bar, what):
    keep = ~ref['exclude']
    frac = ref['exclude'].mean(axis=(2, 3)).max()
    err = np.abs(dev['frames'].astype(np.float64) - ref['frames']).max(axis=2)
    print('%s: excluded %.3f %% of the pixels (worst frame), image max |device - float64| outside = %.3e, bar = %.3e'
          % (what, 100 * frac, err[keep].max(), bar))
    assert frac <= S.EXCLUSION_CAP
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
    """(imgs, masks, clips, float64 composites, device results) of a drawn case: one device run shared by the tests."""
    imgs, masks, clips = S.drawn_case(name)
    _seed, N, out_hw, _sizes = S.CASES[name]
    return imgs, masks, clips, S.composite_case(imgs, masks, clips), run_device(imgs, masks, clips, out_hw, N)


# --------------------------------------------------------------------------------------------------- 1. statistics and plan
@pytest.mark.parametrize('name', sorted(S.CASES))
def test_stats_and_plan_of_the_drawn_cases_equal_the_restatement(name):
    _imgs, _masks, clips, cref, dev = parity_case(name)
    check_stats_and_plan(dev, cref, clips, S.CASES[name][1], name)
    assert any(len({tuple(r) for r in c['plan'][:, k]}) == S.T for c in cref if c['plan'] is not None
               for k in range(c['plan'].shape[1]))                      # a different placement per frame


def _hand_masks():
    """Clip 0: an empty mask (image 1), a one-pixel mask (image 2).  Clip 1: a mask touching all four borders (image 0), an object
    larger than the frame (image 1: area 4 of a full-size box), cut at right and bottom."""
    imgs, masks = S.make_slots(21, [SIZES3, SIZES3], 3)
    masks[0, 1, :29, :41] = 0
    masks[0, 2, :45, :33] = 0
    masks[0, 2, 17, 9] = 5
    masks[1, 0, :37, :53] = 0
    masks[1, 0, 0, 20], masks[1, 0, 36, 3], masks[1, 0, 11, 0], masks[1, 0, 30, 52] = 1, 2, 3, 4
    masks[1, 1, :29, :41] = 1
    rng = np.random.default_rng(22)
    clips = [A.draw_static_params(rng, S.T, SIZES3, (24, 40)) for _ in range(2)]
    for fr in clips[1]['frames']:
        fr['objects'][1] = (4.03, 1.01, 0.37, 0.81)                       # 69 x 70 on a 37 x 53 frame
        fr['paste'] = [0, 2, 1]                                          # (the large one last: on top)
    return imgs, masks, clips


def test_stats_and_plan_edge_masks():
    imgs, masks, clips = _hand_masks()
    cref = S.composite_case(imgs, masks, clips)
    assert cref[0]['stats'][1]['count'] == 0 and cref[0]['stats'][2]['count'] == 1 and cref[0]['stats'][2]['box'] == (17, 9, 18, 10)
    assert cref[1]['stats'][0]['box'] == (0, 0, 37, 53) and cref[1]['stats'][0]['count'] == 4
    big = cref[1]['plan'][:, 1]
    assert np.all(big[:, 0] > 37) and np.all(big[:, 1] > 53) and np.all(big[:, 2:4] == 0)      # cut at right and bottom
    dev = run_device(imgs, masks, clips, (24, 40), 3)
    check_stats_and_plan(dev, cref, clips, 3, 'edge masks')
    assert dev['plan'][0][:, 1, 5].tolist() == [0, 0, 0] and not (dev['comp_lab'][0] == clips[0]['ids'][1]).any()   # dropped
    check_composite(dev, cref, clips, 'edge masks')
    assert np.all(dev['comp_lab'][1][:, :37, :53] == clips[1]['ids'][1])                       # the large object covers the frame
    # the slot padding (0xFF) was never read, the composites never written outside image 0's size
    assert not dev['comp'][:, :, 37:].any() and not dev['comp'][:, :, :, 53:].any() and not dev['comp_lab'][:, :, 37:].any()


# ------------------------------------------------------------------------------------------------------------ 2. composite
@pytest.mark.parametrize('name', sorted(S.CASES))
def test_composites_of_the_drawn_cases_equal_the_restatement(name):
    _imgs, _masks, clips, cref, dev = parity_case(name)
    inside = check_composite(dev, cref, clips, name)
    print('%s: %d composite bytes differ, all inside the exclusion set' % (name, inside))
    for c, clip in zip(cref, clips):
        assert set(np.unique(c['labels'])) - {0} == set(clip['ids'])      # every object shows


def test_unit_resize_pastes_byte_copies_and_one_image_is_copied():
    sizes = [[(37, 53), (29, 41)], [(45, 33)]]
    imgs, masks = S.make_slots(23, sizes, 2)
    masks[0, 1, :29, :41] = 7                                             # a full box of 29 x 41
    unit = np.array([[0.5, 1.0, 0.5, 0.5], [1.0, 41.0 / 29.0, 0.4, 0.6]], np.float32)      # object 1: rh = hc, rw = wc
    clips = [{'sizes': sizes[0], 'out_hw': (24, 40), 'ids': [2, 1], 'frames': [{'objects': unit, 'paste': [0, 1]} for _ in range(S.T)]},
             {'sizes': sizes[1], 'out_hw': (24, 40), 'frames': [{} for _ in range(S.T)]}]
    cref = S.composite_case(imgs, masks, clips)
    assert cref[0]['plan'][0, 1, :2].tolist() == [29, 41]
    dev = run_device(imgs, masks, clips, (24, 40), 2)
    check_stats_and_plan(dev, cref, clips, 2, 'unit resize')
    check_composite(dev, cref, clips, 'unit resize')
    _rh, _rw, tx, ty = cref[0]['plan'][0, 1, :4]
    hv, wv = min(29, 37 - ty), min(41, 53 - tx)
    for t in range(S.T):
        assert np.array_equal(dev['comp'][0, t, ty:ty + hv, tx:tx + wv], imgs[0, 1, :hv, :wv])
        assert np.all(dev['comp_lab'][0, t, ty:ty + hv, tx:tx + wv] == 1)
        assert np.array_equal(dev['comp'][1, t, :45, :33], imgs[1, 0, :45, :33])              # n_img == 1: image and mask bytes
        assert np.array_equal(dev['comp_lab'][1, t, :45, :33], masks[1, 0, :45, :33])


# --------------------------------------------------------------------------------------------------------- 3. static chain
@pytest.mark.parametrize('name', sorted(S.CASES))
def test_static_chain_of_the_drawn_cases(name):
    _imgs, _masks, clips, _cref, dev = parity_case(name)
    blocks = A.pack_static_params(clips)[1][:len(clips) * S.T * 64].reshape(-1, 64)
    assert len({b.tobytes() for b in blocks}) == len(blocks)             # a different record per clip and frame
    ref, _ = chain_reference(dev, clips, S.CASES[name][1], BARS[name]['bar'])
    check_chain(dev, ref, BARS[name]['bar'], name)
    assert dev['frames'].min() >= 0.0 and dev['frames'].max() <= 1.0


def _plain_clips(sizes, out_hw, **over):
    """Clips whose synthesis is drawn and whose chain is hand-made: the identity unless `over` says otherwise."""
    rng = np.random.default_rng(31)
    clips = []
    for s in sizes:
        d = A.draw_static_params(rng, S.T, s, out_hw)
        clip = {k: d[k] for k in ('sizes', 'out_hw', 'ids')}
        clip['frames'] = [{'objects': f['objects'], 'paste': f['paste']} for f in d['frames']]
        clip.update(over)
        clips.append(clip)
    return clips


def test_both_fill_regions_at_clip_scale_0_8():
    sizes = S.CASES['n2_24x40'][3]
    imgs, masks = S.make_slots(24, sizes, 2)
    clips = _plain_clips(sizes, (24, 40), s1=0.8, flip=True)
    for clip in clips:
        for fr in clip['frames']:
            fr.update(angle=20.0, shear=10.0, s2=0.9, factors=(0.8, 1.2, 0.7), order=(A.SATURATION, A.BRIGHTNESS, A.CONTRAST))
    dev = run_device(imgs, masks, clips, (24, 40), 2)
    ref, bar = chain_reference(dev, clips, 2)
    only1, only2 = ref['fill1'] & ~ref['fill2'], ref['fill2'] & ~ref['fill1']
    assert (ref['fill1'][0].sum() >= 10 and ref['fill2'][0].sum() >= 10 and only2[0].sum() >= 10)     # both non-empty, and differ
    assert not np.array_equal(ref['fill1'], ref['fill2'])
    check_chain(dev, ref, bar, 'fill regions')
    keep = ~ref['exclude']
    for reg in (ref['fill1'] & keep, only2 & keep):
        assert np.all(dev['region'][reg] == A.REGION_FILL) and np.all(dev['wlabel'][reg] == 0)
    # without the flag the second test is off: the taps clamp at the source border, as in section 8
    dev2 = run_device(imgs, masks, [dict(c, src_fill=False) for c in clips], (24, 40), 2)
    assert np.all(dev2['region'][only2 & keep] == A.REGION_IMAGE) and np.all(dev2['region'][ref['fill1'] & keep] == A.REGION_FILL)


def test_identity_chain():
    sizes = S.CASES['n2_24x40'][3]
    imgs, masks = S.make_slots(25, sizes, 2)
    clips = _plain_clips(sizes, (24, 40))
    dev = run_device(imgs, masks, clips, (24, 40), 2)
    ref, bar = chain_reference(dev, clips, 2)
    check_chain(dev, ref, bar, 'identity')
    assert not dev['region'].any()
    # clip 0: 37 x 53 -> 24 x 40 at r = 40 / 53: the top-left 31.8 x 53 of the composite, resized
    h0, w0 = sizes[0][0]
    r = 40.0 / 53.0
    ys = np.floor((np.arange(24) + 0.5) / r).astype(int)
    xs = np.floor((np.arange(40) + 0.5) / r).astype(int)
    assert np.array_equal(dev['wlabel'][0, 0], dev['comp_lab'][0, 0][ys][:, xs]) and ys.max() < h0 and xs.max() < w0


def test_hue_alone_and_in_each_of_the_four_positions():
    sizes = [S.CASES['n2_24x40'][3][0]] * 6
    imgs, masks = S.make_slots(26, sizes, 2)
    clips = _plain_clips(sizes, (17, 23))
    clips[0].update(hue=0.05)                                             # the hue op alone
    clips[1].update(hue=-0.05)
    for k in range(4):                                                    # among the three others, in each position
        clips[2 + k].update(hue=0.05, hue_before=k, factors=(1.3, 0.8, 1.2), order=(A.CONTRAST, A.BRIGHTNESS, A.SATURATION))
    for clip in clips:
        for fr in clip['frames']:
            fr.update(angle=12.0, shear=-6.0)                             # (with fill pixels: they take no clip-level op)
    dev = run_device(imgs, masks, clips, (17, 23), 2)
    ref, bar = chain_reference(dev, clips, 2)
    check_chain(dev, ref, bar, 'hue')
    per_clip = np.abs(dev['frames'].astype(np.float64) - ref['frames']).max(axis=2)
    for b in range(6):
        assert per_clip[b][~ref['exclude'][b]].max() <= bar, b
        assert np.abs(ref['frames'][b] - ref['pre'][b]).max() > 0.02      # the op did something
    for a in range(2, 6):
        for b in range(a + 1, 6):
            assert np.abs(ref['frames'][a] - ref['frames'][b]).max() > 1e-3       # the position matters


def test_hue_shift_zero_is_bit_identical_to_no_hue_op():
    sizes = S.CASES['n2_24x40'][3]
    imgs, masks = S.make_slots(27, sizes, 2)
    base = _plain_clips(sizes, (24, 40), factors=(1.3, 0.8, 1.2), order=(A.CONTRAST, A.BRIGHTNESS, A.SATURATION), gray=False)
    a = run_device(imgs, masks, base, (24, 40), 2)
    b = run_device(imgs, masks, [dict(c, hue=0.0, hue_before=2) for c in base], (24, 40), 2)
    c = run_device(imgs, masks, [dict(c, hue=0.05, hue_before=2) for c in base], (24, 40), 2)
    assert all(np.array_equal(a[k], b[k]) for k in FIELDS + ('comp', 'comp_lab', 'region'))
    assert not np.array_equal(a['frames'], c['frames'])


# --------------------------------------------------------------------------------------------------------- 4. compatibility
def test_static_entry_with_words_60_to_63_zero_equals_the_clip_entry_bit_for_bit():
    src, lab, clips = R.drawn_case('small_24x40')
    block = A.pack_params(clips)
    assert not block[:len(clips) * 3 * 64].reshape(-1, 64)[:, 60:].any()
    aug = A.ClipAugmenter((24, 40), 2, 3, device=DEV)
    want = aug(to_dev(src), to_dev(lab), block)
    syn = A.StaticClipSynthesizer((24, 40), 2, 3, (37, 53), device=DEV)
    synth_block = np.zeros(len(clips) * (32 + 3 * 64), np.int32)
    got = syn.warp(to_dev(src), to_dev(lab), (synth_block, block))
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert torch.equal(syn.regions(2), aug.regions(2)) and torch.equal(syn.warped_labels(2), aug.warped_labels(2))


# -------------------------------------------------------------------------------------------------------------- 5. plumbing
def test_eager_calls_and_graph_replays_are_bit_identical():
    imgs, masks, clips, _cref, _dev = parity_case('n2_24x40')
    sizes = S.CASES['n2_24x40'][3]
    rng = np.random.default_rng(77)
    other = [A.draw_static_params(rng, S.T, s, (24, 40)) for s in sizes]
    i, m = to_dev(imgs), to_dev(masks)
    syn = A.StaticClipSynthesizer((24, 40), 2, S.T, S.SLOT_HW, device=DEV)
    eager = {}
    for key, p in (('a', clips), ('b', other)):
        first = [t.clone() for t in syn(i, m, p)] + [t.clone() for t in syn.composites(2)]
        second = list(syn(i, m, p)) + list(syn.composites(2))
        assert all(torch.equal(x, y) for x, y in zip(first, second)), key
        eager[key] = first
    assert not torch.equal(eager['a'][0], eager['b'][0])
    static = syn.empty_out(2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        syn(i, m, None, out=static)
    for key, p in (('b', other), ('a', clips), ('b', other)):
        syn.set_params(p)
        for t in static:
            t.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(list(static) + list(syn.composites(2)), eager[key])), key


def test_graph_replay_of_four_clips_equals_the_eager_call():
    """B = 4, N = 2: the batch at which a captured call that cleared its words with memset nodes replayed with a buffer mis-filled
    (csrc/image_sample.h, clear_words_kernel).  The replay is compared without refilling the parameters, statistics and table included."""
    sizes = S.CASES['n2_24x40'][3] * 2
    imgs, masks = S.make_slots(28, sizes, 2)
    rng = np.random.default_rng(29)
    clips = [A.draw_static_params(rng, S.T, s, (24, 40)) for s in sizes]
    i, m = to_dev(imgs), to_dev(masks)
    syn = A.StaticClipSynthesizer((24, 40), 2, S.T, S.SLOT_HW, device=DEV)
    out = syn.empty_out(4)

    def state():
        torch.cuda.synchronize()
        return [t.clone() for t in out] + [t.clone() for t in syn.composites(4)] + [syn.stats(4).clone(), syn.plan(4).clone()]
    syn(i, m, clips, out=out)
    eager = state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        syn(i, m, None, out=out)
    for rounds in (1, 20):                                                # one replay, then replays back to back
        for t in out:
            t.fill_(-3)
        for _ in range(rounds):
            graph.replay()
        assert all(torch.equal(x, y) for x, y in zip(state(), eager)), rounds
    for _ in range(20):                                                   # and eager calls back to back
        syn(i, m, None, out=out)
    assert all(torch.equal(x, y) for x, y in zip(state(), eager))


def test_filling_two_slots_of_a_larger_batch_leaves_the_others_alone():
    imgs, masks, clips, _cref, _dev = parity_case('n2_24x40')
    i, m = to_dev(imgs), to_dev(masks)
    syn = A.StaticClipSynthesizer((24, 40), 2, S.T, S.SLOT_HW, device=DEV)
    direct = syn(i, m, clips)
    out = syn.empty_out(4)
    for t in out:
        t.fill_(-7)
    got = syn(i, m, clips, out=out, b0=1)
    assert all(g is o for g, o in zip(got, out))
    for name, o, d in zip(FIELDS, out, direct):
        assert torch.equal(o[1:3], d), name
        assert bool((o[0] == -7).all()) and bool((o[3] == -7).all()), name
    with pytest.raises(Exception, match='do not fit'):
        syn(i, m, clips, out=out, b0=3)


def test_outputs_are_what_one_step_takes():
    imgs, masks, clips, _cref, _dev = parity_case('n3_17x23')
    B, T, N, (Ho, Wo) = 2, S.T, 3, (17, 23)
    syn = A.StaticClipSynthesizer((Ho, Wo), N, T, S.SLOT_HW, device=DEV)
    frames, mks, valid_obj, label, found = syn(to_dev(imgs), to_dev(masks), clips)
    for t, shape, dt in ((frames, (B, T, 3, Ho, Wo), torch.float32), (mks, (B, T, N + 1, Ho, Wo), torch.float32),
                         (valid_obj, (B, N + 1), torch.float32), (label, (B, T, Ho, Wo), torch.int64), (found, (B,), torch.int32)):
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous() and t.device == torch.device(DEV)
    assert bool((mks.sum(2) == 1).all()) and bool(((mks == 0) | (mks == 1)).all())
    assert torch.equal(label, mks.argmax(2))
    init_mask = mks[:, 0]
    assert init_mask.data_ptr() == mks.data_ptr() and init_mask._base is mks and tuple(init_mask.shape) == (B, N + 1, Ho, Wo)
    assert float(frames.min()) >= 0.0 and float(frames.max()) <= 1.0
    assert bool(((valid_obj == 0) | (valid_obj == 1)).all()) and bool((valid_obj[:, :2] == 1).all())


# ---------------------------------------------------------------------------------------------------- 6. ranges and errors
def test_smallest_sizes_and_seven_images_return_results():
    rng = np.random.default_rng(41)
    # 1 x 1 images, a 2 x 2 output
    sizes = [[(1, 1), (1, 1)]]
    imgs, masks = S.make_slots(42, sizes, 2, cell=1, values=(1,))
    clips = [A.draw_static_params(rng, S.T, sizes[0], (2, 2))]
    dev = run_device(imgs, masks, clips, (2, 2), 2)
    cref = S.composite_case(imgs, masks, clips)
    check_stats_and_plan(dev, cref, clips, 2, '1x1')
    check_composite(dev, cref, clips, '1x1')
    assert np.isfinite(dev['frames']).all() and dev['stats'][0, :, 4].tolist() == [1, 1]
    # n_img = N = 7 (eight mask channels)
    sizes = [[(37, 53), (29, 41), (45, 33), (29, 41), (37, 53), (45, 33), (29, 41)]]
    imgs, masks = S.make_slots(43, sizes, 7)
    clips = [A.draw_static_params(rng, S.T, sizes[0], (17, 23))]
    dev = run_device(imgs, masks, clips, (17, 23), 7)
    cref = S.composite_case(imgs, masks, clips)
    check_stats_and_plan(dev, cref, clips, 7, 'seven images')
    check_composite(dev, cref, clips, 'seven images')
    ref, bar = chain_reference(dev, clips, 7)
    check_chain(dev, ref, bar, 'seven images')
    assert dev['masks'].shape == (1, S.T, 8, 17, 23)


def test_wrong_arguments_and_wrong_blocks_give_errors_or_pictures():
    imgs, masks, clips, _cref, _dev = parity_case('n2_24x40')
    i, m = to_dev(imgs), to_dev(masks)
    with pytest.raises(ValueError):
        A.StaticClipSynthesizer((24, 40), 8, S.T, S.SLOT_HW, device=DEV)
    syn = A.StaticClipSynthesizer((24, 40), 2, S.T, S.SLOT_HW, device=DEV)
    with pytest.raises(ValueError):
        syn(i[:, :1], m[:, :1], clips)
    with pytest.raises(_lib.SwemHipError):
        syn(i.float(), m, clips)
    with pytest.raises(_lib.SwemHipError, match='at least 2x2'):
        A.StaticClipSynthesizer((1, 40), 2, S.T, S.SLOT_HW, device=DEV)(i, m, clips)
    # a block whose sizes, counts, orders and numbers are out of range: every one is clamped on the device
    synth, block = A.pack_static_params(clips)
    bad = synth.copy()
    bad[0], bad[32] = 99, -5                                             # n_img
    bad[2:6] = [10 ** 6, -3, 0, 2 ** 30]                                 # sizes
    fr = bad[64:].reshape(-1, 64)
    fr[:, :7] = [1, 1, -1, 9, 0, 2 ** 30, 3]                             # paste order
    fl = fr.view(np.float32)
    fl[:, 8:12] = [np.nan, 0.0, np.inf, -1e30]
    fl[:, 12:16] = [1e30, 1e-30, 7.0, np.nan]
    blk = block.copy()
    rec = blk[:2 * S.T * 64].reshape(-1, 64)
    rec[:, 61], rec[:, 62] = 10 ** 6, -4                                 # out of range: the call's Hs, Ws
    out = syn(i, m, (bad, blk))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in out)
    comp, comp_lab = syn.composites(2)
    assert int(syn.plan(2)[..., :2].max()) <= 4 * 56 and int(syn.plan(2)[..., 2:4].min()) >= 0
