"""CPU: the stage-0 path's yardstick (tests/synth_ref.py) pinned to things outside this package -- torch's bicubic / nearest
resize, the stdlib's colorsys, section 8's identity case --, the host side (swem_amd/augment.py: draw_static_params,
static_frame_matrices, pack_static_params), the conditions the GPU cases must meet, and the argument validation of the new C
entry points."""
import colorsys
import ctypes
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from swem_amd import augment as A
from tests import augment_ref as R
from tests import synth_ref as S


# ------------------------------------------------------------------------------------ the object resize against torch's own
def test_object_resize_equals_torch_bicubic_and_nearest():
    """Box sizes 37x53 against coprime targets, down and up: no nearest coordinate but 0 is an integer (torch computes its
    nearest index with an fp32 scale)."""
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    mask = R.block_labels(rng, (37, 53), 6, S.MASK_VALUES)
    for rh, rw in ((23, 31), (41, 59), (1, 1), (36, 60)):
        col, m = S.resize_object(img, mask, rh, rw)
        x = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
        want = F.interpolate(x, size=(rh, rw), mode='bicubic', align_corners=False)[0].permute(1, 2, 0).numpy()
        assert np.abs(col - want).max() < 1e-12 * 255, (rh, rw)
        wm = F.interpolate(torch.from_numpy(mask.astype(np.float64))[None, None], size=(rh, rw), mode='nearest')[0, 0].numpy()
        assert np.array_equal(m, wm.astype(np.uint8)), (rh, rw)
    # unit resize: byte copies
    col, m = S.resize_object(img, mask, 37, 53)
    assert np.array_equal(col, img.astype(np.float64)) and np.array_equal(m, mask)


# ----------------------------------------------------------------------------------------------- the hue op against colorsys
def test_hue_op_equals_colorsys():
    rng = np.random.default_rng(1)
    x = rng.random((3, 500))
    x[:, :20] = x[:1, :20]                      # gray pixels
    x[1, 20:40] = x[0, 20:40]                   # ties of the maximum
    x[:, 40:44] = [[0, 1, 0, 1], [0, 1, 1, 0], [0, 1, 0, 0]]
    for shift in (0.05, -0.05, 0.31, -0.5, 0.5):
        got = S.hue(x, shift)
        for n in range(x.shape[1]):
            h, s, v = colorsys.rgb_to_hsv(*x[:, n])
            want = colorsys.hsv_to_rgb((h + shift) % 1.0, s, v)
            assert np.abs(got[:, n] - np.array(want)).max() < 1e-12, (shift, n)
    assert np.abs(S.hue(x, 0.05) - x).max() > 0.01
    # fp32 form: same formulas, the tolerance of the device tests is measured with it
    assert np.abs(S.hue(x.astype(np.float32), 0.05, np.float32) - S.hue(x, 0.05)).max() < 1e-4


# -------------------------------------------------------------------------------------------------- the chain: identity case
def _identity_inputs():
    src, lab = R.make_inputs(4, 1, 1, (36, 60))       # the aspect of the 24x40 output: r = 2/3 on both axes
    return src[0], lab[0]


def test_identity_static_chain_equals_section_8_identity_case():
    src, lab = _identity_inputs()
    static = {'sizes': [(36, 60)], 'out_hw': (24, 40), 'frames': [{}]}
    plain = {'out_hw': (24, 40), 'crop': (0, 0, 36, 60), 'flip': False, 'frames': [{}]}
    a, b = S.static_chain(src, lab, static, 2), R.augment_clip(src, lab, plain, 2)
    assert np.abs(a['frames'] - b['frames']).max() < 1e-12 and np.array_equal(a['wlabel'], b['wlabel'])
    assert not a['region'].any() and np.array_equal(a['masks'], b['masks']) and np.array_equal(a['valid'], b['valid'])
    x = torch.from_numpy(src[0].astype(np.float64) / 255).permute(2, 0, 1)[None]
    want = F.interpolate(x, size=(24, 40), mode='bicubic', align_corners=False)[0].numpy()
    assert np.abs(a['frames'][0] - want).max() < 1e-12
    # the packed records agree too: words 0..59 are section 8's, 60..63 name the source size and the second fill test
    _synth, block = A.pack_static_params([static])
    old = A.pack_params([plain])
    assert np.allclose(block.view(np.float32)[:12], old.view(np.float32)[:12], atol=1e-6)
    assert np.array_equal(block[12:60], old[12:60]) and block[60:64].tolist() == [1, 36, 60, 0]


def test_packed_matrices_are_the_chain():
    """static_frame_matrices (what the kernels evaluate) against the step-by-step chain of the restatement, TPS off."""
    rng = np.random.default_rng(3)
    for flip in (False, True):
        clip = A.draw_static_params(rng, 2, [(45, 33), (29, 41)], (24, 40))
        clip['flip'] = flip
        for fr in clip['frames']:
            g = S.static_geometry(clip, dict(fr, tps_on=False))
            M_aff, M_src = A.static_frame_matrices(clip, fr)
            i, j = np.meshgrid(np.arange(40) + 0.5, np.arange(24) + 0.5)
            xa = M_aff[0, 0] * i + M_aff[0, 1] * j + M_aff[0, 2]
            ya = M_aff[1, 0] * i + M_aff[1, 1] * j + M_aff[1, 2]
            assert np.abs(xa - g['px'] * 40 / 33).max() < 1e-9 and np.abs(ya - g['py'] * 24 / 45).max() < 1e-9
            assert np.abs(M_src[0, 0] * i + M_src[0, 1] * j + M_src[0, 2] - g['sx']).max() < 1e-9
            assert np.abs(M_src[1, 0] * i + M_src[1, 1] * j + M_src[1, 2] - g['sy']).max() < 1e-9
    # frame_matrices passes a frame's own M_src through, and keeps composing where there is none
    M = np.arange(6.0).reshape(2, 3)
    clip = {'out_hw': (24, 40), 'crop': (1, 2, 30, 44), 'flip': True}
    assert np.array_equal(A.frame_matrices(clip, {'M_src': M})[1], M)
    assert np.array_equal(A.frame_matrices(clip, {})[1], A.compose(A.inverse_affine(0, 0, (24, 40)), clip['crop'], True, (24, 40)))


def test_both_fill_tests_fire_for_a_clip_scale_below_one():
    src, lab = R.make_inputs(5, 1, 1, (37, 53))
    clip = {'sizes': [(37, 53)], 'out_hw': (24, 40), 's1': 0.8, 'frames': [{'angle': 20.0, 'shear': 10.0, 's2': 0.9}]}
    ref = S.static_chain(src[0], lab[0], clip, 2)
    f1, f2 = ref['fill1'][0], ref['fill2'][0]
    assert f1.sum() >= 10 and f2.sum() >= 10 and (f2 & ~f1).sum() >= 10 and (f1 & ~f2).sum() >= 0
    assert np.array_equal(ref['region'][0] == A.REGION_FILL, f1 | f2)
    fillc = np.array(A.IM_MEAN) / 255.0
    assert np.abs(ref['frames'][0][:, f2 & ~f1] - fillc[:, None]).max() < 1e-12 and not ref['wlabel'][0][f1 | f2].any()
    # with s1 >= 1 the source covers image 0: the second test never fires
    ref = S.static_chain(src[0], lab[0], dict(clip, s1=1.2), 2)
    assert not (ref['fill2'][0] & ~ref['fill1'][0]).any()


# ---------------------------------------------------------------------------------------------------------------- the sampler
def test_draw_static_params_stays_inside_its_ranges():
    rng = np.random.default_rng(6)
    sizes, out_hw = [(300, 500), (480, 640), (333, 250)], (384, 384)
    seen_before, seen_flip = set(), set()
    for _ in range(200):
        p = A.draw_static_params(rng, 3, sizes, out_hw)
        assert 0.8 <= p['s1'] < 1.5 and abs(p['hue']) <= 0.05 and 0.9 <= p['factors'][0] <= 1.1
        assert all(0.95 <= v <= 1.05 for v in p['factors'][1:]) and sorted(p['order']) == [0, 1, 2] and 0 <= p['hue_before'] <= 3
        assert len(set(p['ids'])) == 3 and all(1 <= i <= 4 for i in p['ids'])
        assert sorted(p['prio'].tolist()) == list(range(256))
        seen_before.add(p['hue_before'])
        seen_flip.add(p['flip'])
        r = A.static_scale(sizes[0], out_hw)
        for f in p['frames']:
            assert abs(f['angle']) <= 20 and abs(f['shear']) <= 10 and 0.9 <= f['s2'] < 1.1
            assert 0 <= f['top'] <= int(np.floor(r * 300)) - 384 and 0 <= f['left'] <= int(np.floor(r * 500)) - 384
            assert 0.9 <= f['factors'][0] <= 1.1 and all(0.95 <= v <= 1.05 for v in f['factors'][1:])
            assert sorted(f['order']) == [0, 1, 2] and sorted(f['paste']) == [0, 1, 2]
            o = f['objects']
            assert o.dtype == np.float32 and o.shape == (3, 4)
            assert np.all((o[:, 0] >= np.float32(0.16)) & (o[:, 0] < np.float32(0.81)))
            assert np.all((o[:, 1] >= np.float32(0.75)) & (o[:, 1] <= np.float32(4.0 / 3.0) * (1 + 1e-6)))
            assert np.all((o[:, 2:] >= 0) & (o[:, 2:] < 1))
            assert np.abs(f['tps_Y'] - A.TPS_ANCHORS).max() <= 0.15 and np.all(f['tps_Y'][[0, 3, 12, 15]] == A.TPS_ANCHORS[[0, 3, 12, 15]])
    assert seen_before == {0, 1, 2, 3} and seen_flip == {False, True}
    # the packed blocks: sizes, ids, paste order, hue word
    p = A.draw_static_params(rng, 3, sizes[:2], out_hw)
    synth, block = A.pack_static_params([p])
    assert synth.size == 32 + 3 * 64 and block.size == 3 * 64 + 256
    assert synth[0] == 2 and synth[2:6].tolist() == [300, 500, 480, 640] and synth[16:18].tolist() == p['ids']
    fr = synth[32:].reshape(3, 64)
    assert all(fr[t, :2].tolist() == p['frames'][t]['paste'] and fr[t, 2:7].tolist() == [-1] * 5 for t in range(3))
    assert np.array_equal(fr[:, 8:16].view(np.float32), np.stack([f['objects'].reshape(-1) for f in p['frames']]))
    rec = block[:3 * 64].reshape(3, 64)
    assert np.all(rec[:, 60] == (1 | (p['hue_before'] << 4))) and np.all(rec[:, 61] == 300) and np.all(rec[:, 62] == 500)
    assert np.all(rec[:, 63].view(np.float32) == np.float32(p['hue']))


# ------------------------------------------------------------------------------------------- compositing: the restatement
def test_composite_restatement_edge_cases():
    imgs, masks = S.make_slots(7, [[(37, 53), (29, 41), (45, 33)]], 3)
    im, mk = S.unslot(imgs, masks, 0, [(37, 53), (29, 41), (45, 33)])
    mk[1][:] = 0                                              # an empty mask: dropped
    objs = np.array([[0.5, 1.0, 0.3, 0.6]] * 3, np.float32)
    clip = {'sizes': [(37, 53), (29, 41), (45, 33)], 'out_hw': (24, 40), 'ids': [3, 1, 2],
            'frames': [{'objects': objs, 'paste': [2, 1, 0]}]}
    c = S.composite(im, mk, clip)
    assert c['plan'][0, 1].tolist() == [0, 0, 0, 0, 1, 0] and set(np.unique(c['labels'])) <= {0, 2, 3} and (c['labels'] == 3).any()
    # background: image 0 outside its mask, the mean colour inside
    bg = (c['labels'][0] == 0)
    st = c['stats'][0]
    mean = np.floor(st['sums'] / (st['count'] + 1e-8) + 0.5).astype(np.uint8)
    assert np.array_equal(c['frames'][0][bg & (mk[0] == 0)], im[0][bg & (mk[0] == 0)])
    assert np.all(c['frames'][0][bg & (mk[0] != 0)] == mean)
    # one image: image and mask bytes
    one = S.composite(im[:1], mk[:1], {'sizes': [(37, 53)], 'out_hw': (24, 40), 'frames': [{}, {}]})
    assert np.array_equal(one['frames'][1], im[0]) and np.array_equal(one['labels'][0], mk[0])


# ---------------------------------------------------------------------------------------------- what the GPU cases must meet
def test_cases_meet_their_conditions_and_the_recorded_bars_are_current():
    """Seeds are chosen on the restatement alone: no object size within 1e-6 of a half-integer, both exclusion sets (the
    composite's colours near k + 0.5, the chain's coordinates near a threshold) under 3 % of a frame; the bars the device tests
    read are 4x the recorded fp32-against-float64 maximum and a re-measurement here stays inside them."""
    rec = json.load(open(os.path.join(os.path.dirname(__file__), '..', 'profiles', 'synth_parity.json')))
    for name in S.CASES:
        row, now = rec['cases'][name], S.measure_bar(name)
        assert row['bar'] == 4.0 * row['fp32_vs_fp64_max'] and row['seed'] == S.CASES[name][0]
        assert now['half_integer_margin'] >= S.HALF_MARGIN
        assert now['excluded_fraction_max_per_frame'] <= S.EXCLUSION_CAP
        assert now['composite_excluded_fraction_max_per_frame'] <= S.EXCLUSION_CAP
        assert now['label_or_region_differences_outside'] == 0
        assert now['fp32_vs_fp64_max'] <= row['bar'] and 1e-6 < row['fp32_vs_fp64_max'] < 1e-4


# ---------------------------------------------------------------------------------------------- C ABI: argument validation
def test_synth_entry_points_validate_before_any_hip_call(lib):
    assert lib.swem_synth_workspace(0, 3, 2) == 0 and lib.swem_synth_workspace(2, 3, -1) == 0
    assert lib.swem_synth_workspace(2, 3, 3) == 256 + 768            # 2*3*8*4 = 192 -> 256; 2*3*3*8*4 = 576 -> 768
    p = ctypes.c_void_p(4096)                                        # non-null, aligned; never dereferenced

    def synth(imgs=p, masks=p, params=p, comp=p, comp_lab=p, B=2, T=3, N=2, Hmax=48, Wmax=56, ws=p, ws_bytes=1 << 30):
        return lib.swem_synth_frames_u8(None, imgs, masks, params, comp, comp_lab, B, T, N, Hmax, Wmax, ws, ws_bytes)
    for name in ('imgs', 'masks', 'params', 'comp', 'comp_lab', 'ws'):
        assert synth(**{name: None}) == -4 and b'null pointer' in lib.swem_last_error(), name
    assert synth(params=ctypes.c_void_p(4098)) == -4 and b'aligned' in lib.swem_last_error()
    for kw in (dict(B=0), dict(T=-1), dict(Hmax=0), dict(Wmax=0)):
        assert synth(**kw) == -1 and b'need B, T, Hmax, Wmax > 0' in lib.swem_last_error(), kw
    for kw in (dict(N=0), dict(N=8)):
        assert synth(**kw) == -1 and b'1 <= N <= 7' in lib.swem_last_error(), kw
    assert synth(Hmax=4097) == -1 and b'4096' in lib.swem_last_error()
    assert synth(ws_bytes=lib.swem_synth_workspace(2, 3, 2) - 1) == -2 and b'workspace' in lib.swem_last_error()

    def static(src=p, lab=p, params=p, frames=p, masks=p, valid=p, label=p, found=p, B=2, T=3, Hs=48, Ws=56, Ho=24, Wo=40, N=2,
               ws=p, ws_bytes=1 << 30):
        return lib.swem_augment_static_u8(None, src, lab, params, frames, masks, valid, label, found, B, T, Hs, Ws, Ho, Wo, N,
                                          ws, ws_bytes)
    for name in ('src', 'lab', 'params', 'frames', 'masks', 'valid', 'label', 'found', 'ws'):
        assert static(**{name: None}) == -4 and b'augment_static: null pointer' in lib.swem_last_error(), name
    assert static(label=ctypes.c_void_p(4100)) == -4 and b'aligned' in lib.swem_last_error()
    for kw in (dict(B=0), dict(Hs=0)):
        assert static(**kw) == -1 and b'need B, T, Hs, Ws > 0' in lib.swem_last_error(), kw
    assert static(Wo=1) == -1 and b'at least 2x2' in lib.swem_last_error()
    assert static(N=8) == -1 and b'N + 1 <= 8' in lib.swem_last_error()
    assert static(ws_bytes=lib.swem_augment_workspace(2, 3, 24, 40) - 1) == -2 and b'workspace' in lib.swem_last_error()
