"""CPU: the host side of the device augmentation (swem_amd/augment.py) -- TPS coefficients, affine maths, the sampler's ranges --,
the anchor of the float64 restatement (tests/augment_ref.py) against torch's own bicubic / nearest-exact resize, and the
argument validation of the C entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from swem_amd import augment as A
from tests import augment_ref as R


# ------------------------------------------------------------------------------------------------------ TPS coefficients
def test_tps_reproduces_its_anchors():
    rng = np.random.default_rng(0)
    for _ in range(5):
        Y = A.TPS_ANCHORS.copy()
        Y[A.TPS_INNER] += (rng.random((4, 2)) - 0.5) * 0.25
        Aff, W = A.tps_coefficients(Y)
        assert Aff.shape == (3, 2) and W.shape == (16, 2)
        assert np.abs(A.tps_eval(Aff, W, A.TPS_ANCHORS) - Y).max() < 1e-9
    # all anchors shifted (never drawn): still interpolated
    Aff, W = A.tps_coefficients(A.TPS_ANCHORS + 0.3)
    assert np.abs(A.tps_eval(Aff, W, A.TPS_ANCHORS) - (A.TPS_ANCHORS + 0.3)).max() < 1e-9


def test_tps_of_undisturbed_anchors_is_the_identity():
    Aff, W = A.tps_coefficients(A.TPS_ANCHORS)
    assert np.abs(W).max() < 1e-9
    assert np.abs(Aff - np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])).max() < 1e-9


def test_anchor_table_is_the_row_major_4x4_grid():
    lin = np.linspace(-1, 1, 4)
    for k in range(16):
        assert tuple(A.TPS_ANCHORS[k]) == (lin[k % 4], lin[k // 4])
    assert A.TPS_INNER == [k for k in range(16) if 0 < k % 4 < 3 and 0 < k // 4 < 3]


# ------------------------------------------------------------------------------------------------------------ affine maths
def test_compose_whole_image_is_the_pure_scale():
    out_hw, src_hw = (24, 40), (37, 53)
    M = A.compose(A.inverse_affine(0.0, 0.0, out_hw), (0, 0) + src_hw, False, out_hw)
    assert np.abs(M - np.array([[53 / 40, 0, 0], [0, 37 / 24, 0]])).max() < 1e-12


def test_compose_flip_mirrors_x():
    out_hw = (24, 40)
    crop = (3, 5, 20, 31)
    rng = np.random.default_rng(1)
    M_aff = A.inverse_affine(11.0, -7.0, out_hw)
    plain, flipped = A.compose(M_aff, crop, False, out_hw), A.compose(M_aff, crop, True, out_hw)
    mirror = np.array([[-1.0, 0.0, 40.0], [0.0, 1.0, 0.0]])            # x' -> Wo - x'
    want = A.compose(mirror @ np.concatenate([M_aff, [[0, 0, 1.0]]]), crop, False, out_hw)
    assert np.abs(flipped - want).max() < 1e-12
    for x, y in rng.random((5, 2)) * (40, 24):
        xa, ya = M_aff @ (x, y, 1.0)
        assert abs((flipped @ (x, y, 1.0))[0] - (5 + (40 - xa) * 31 / 40)) < 1e-11
        assert abs((plain @ (x, y, 1.0))[0] - (5 + xa * 31 / 40)) < 1e-11
        assert abs((plain @ (x, y, 1.0))[1] - (3 + ya * 20 / 24)) < 1e-11


def test_inverse_affine_inverts_the_forward_matrix():
    eye = np.eye(3)
    for angle, shear, out_hw in ((15.0, 10.0, (384, 384)), (-15.0, -10.0, (24, 40)), (3.3, 9.1, (17, 23)), (0.0, 0.0, (2, 2))):
        inv = np.concatenate([A.inverse_affine(angle, shear, out_hw), [[0, 0, 1.0]]])
        fwd = np.concatenate([A.affine_forward(angle, shear, out_hw), [[0, 0, 1.0]]])
        assert np.abs(inv @ fwd - eye).max() < 1e-12
        ctr = np.array([out_hw[1] / 2, out_hw[0] / 2, 1.0])
        assert np.abs(inv @ ctr - ctr).max() < 1e-12
    # the stated entries: a = cos r, b = -cos r tan s - sin r, c = sin r, d = -sin r tan s + cos r; inverse [[d, -b], [-c, a]]
    r, s = np.deg2rad(15.0), np.deg2rad(10.0)
    a, b, c, d = np.cos(r), -np.cos(r) * np.tan(s) - np.sin(r), np.sin(r), -np.sin(r) * np.tan(s) + np.cos(r)
    assert np.abs(A.inverse_affine(15.0, 10.0, (384, 384))[:, :2] - np.array([[d, -b], [-c, a]])).max() < 1e-15


def test_centred_form_is_the_same_map():
    out_hw = (17, 23)
    M = A.compose(A.inverse_affine(-9.0, 4.0, out_hw), (1, 2, 30, 41), True, out_hw)
    Mc = A.centred(M, out_hw)
    for x, y in ((0.5, 0.5), (22.5, 16.5), (7.25, 3.0)):
        assert np.abs(M @ (x, y, 1.0) - Mc @ (x - 23 / 2, y - 17 / 2, 1.0)).max() < 1e-12


# ----------------------------------------------------------------------------------------------------------- draw_params
def test_draw_params_is_a_function_of_the_seed():
    a = A.pack_params([A.draw_params(np.random.default_rng(5), 3, (480, 854), (384, 384)) for _ in range(2)])
    b = A.pack_params([A.draw_params(np.random.default_rng(5), 3, (480, 854), (384, 384)) for _ in range(2)])
    c = A.pack_params([A.draw_params(np.random.default_rng(6), 3, (480, 854), (384, 384)) for _ in range(2)])
    assert a.dtype == np.int32 and a.size == 2 * 3 * 64 + 2 * 256
    assert np.array_equal(a, b) and not np.array_equal(a, c)


@pytest.mark.parametrize('is_bl', [False, True])
def test_draws_lie_in_the_stated_ranges(is_bl):
    rng = np.random.default_rng(7)
    H, W = 480, 854
    flips = grays = 0
    orders = set()
    for _ in range(2000):
        p = A.draw_params(rng, 3, (H, W), (384, 384), is_bl=is_bl)
        top, left, ch, cw = p['crop']
        assert 0 <= top and 0 <= left and ch > 0 and cw > 0 and top + ch <= H and left + cw <= W
        assert (0.25 if is_bl else 0.36) * H * W * 0.98 <= ch * cw <= H * W
        assert 3 / 4 * 0.98 <= cw / ch <= 4 / 3 * 1.02
        b, c, s = p['factors']
        assert 0.9 <= b <= 1.1 and 0.97 <= c <= 1.03 and 0.97 <= s <= 1.03
        assert sorted(p['order']) == [0, 1, 2]
        assert sorted(p['prio'].tolist()) == list(range(256))
        flips += p['flip']
        grays += p['gray']
        orders.add(p['order'])
        assert len(p['frames']) == 3
        for f in p['frames']:
            assert -15 <= f['angle'] <= 15 and -10 <= f['shear'] <= 10
            assert all(0.99 <= v <= 1.01 for v in f['factors']) and sorted(f['order']) == [0, 1, 2]
            assert f['tps_on'] is True
            d = f['tps_Y'] - A.TPS_ANCHORS
            assert np.abs(d).max() <= 0.125 and np.all(d[[k for k in range(16) if k not in A.TPS_INNER]] == 0)
            assert np.all(d[A.TPS_INNER] != 0)
    assert 900 < flips < 1100 and 60 < grays < 145 and len(orders) == 6        # p = 0.5, p = 0.05 (+- 4 sigma), 3! orders


def test_crop_falls_back_to_the_centre_crop():
    # a 10x100 strip: no box of ratio 3/4..4/3 and 36 % of the area fits (it would be at least 16 high) -> centre crop at ratio 4/3
    p = A.draw_params(np.random.default_rng(0), 1, (10, 100), (8, 8))
    assert p['crop'] == (0, (100 - 13) // 2, 10, 13)
    p = A.draw_params(np.random.default_rng(0), 1, (100, 10), (8, 8))
    assert p['crop'] == ((100 - 13) // 2, 0, 13, 10)


def test_clip_level_fields_repeat_and_frame_level_fields_differ():
    T = 3
    block = A.pack_params([A.draw_params(np.random.default_rng(8), T, (480, 854), (384, 384))])
    rec = block[:T * 64].reshape(T, 64)
    fl = rec.view(np.float32)
    assert np.all(rec[:, 57] == rec[0, 57]) and np.all(rec[:, 58] == rec[0, 58]) and np.all(fl[:, 50:53] == fl[0, 50:53])
    assert np.all(rec[:, 56] == 1) and np.all(rec[:, 60:] == 0)
    for t in range(1, T):
        for lo, hi in ((0, 6), (6, 12), (12, 18), (18, 50), (53, 56)):
            assert not np.array_equal(fl[t, lo:hi], fl[0, lo:hi]), (t, lo)
    # the label order is the inverse of the priority permutation
    p = A.draw_params(np.random.default_rng(8), T, (480, 854), (384, 384))
    order = A.pack_params([p])[T * 64:]
    assert np.array_equal(p['prio'][order], np.arange(256))
    with pytest.raises(ValueError):
        A.label_order(np.zeros(256, int))


# ------------------------------------------------------------------------------- the restatement against torch's own resize
def test_restatement_identity_case_equals_torch_resize():
    """No TPS, identity affine, whole-image crop: the single resample IS a plain resize.  This ties the yardstick of the device
    tests to something outside this package."""
    src, lab = R.make_inputs(4, 1, 1, (37, 53))
    clip = {'out_hw': (24, 40), 'crop': (0, 0, 37, 53), 'flip': False, 'frames': [{'angle': 0.0, 'shear': 0.0}]}
    ref = R.augment_clip(src[0], lab[0], clip, 2, np.float64)
    assert not ref['region'].any()
    x = torch.from_numpy(src[0, 0].astype(np.float64) / 255).permute(2, 0, 1)[None]
    want = F.interpolate(x, size=(24, 40), mode='bicubic', align_corners=False)[0].numpy()
    assert np.abs(ref['frames'][0] - want).max() < 1e-12
    assert np.abs(ref['pre'][0] - want).max() < 1e-12
    wl = F.interpolate(torch.from_numpy(lab[0, 0].astype(np.float64))[None, None], size=(24, 40), mode='nearest-exact')[0, 0]
    assert np.array_equal(ref['wlabel'][0], wl.numpy().astype(np.uint8))


def test_restatement_flip_of_the_identity_case_is_the_mirrored_resize():
    src, lab = R.make_inputs(4, 1, 1, (37, 53))
    clip = {'out_hw': (24, 40), 'crop': (0, 0, 37, 53), 'flip': False, 'frames': [{}]}
    a = R.augment_clip(src[0], lab[0], clip, 2)
    b = R.augment_clip(src[0], lab[0], dict(clip, flip=True), 2)
    assert np.abs(a['frames'][..., ::-1] - b['frames']).max() < 1e-12 and np.array_equal(a['wlabel'][..., ::-1], b['wlabel'])


def test_parity_cases_keep_the_exclusion_set_under_the_cap_and_the_recorded_bars_are_current():
    """The seeds are chosen on the restatement alone; the bars the device tests read are 4x the recorded fp32-against-float64
    maximum, and a re-measurement here stays inside them (numpy's float32 log may differ in the last bit between machines: the
    recorded figure itself is not compared)."""
    rec = json.load(open(os.path.join(os.path.dirname(__file__), '..', 'profiles', 'augment_parity.json')))
    for name in ('small_24x40', 'small_17x23'):
        row, now = rec['cases'][name], R.measure_bar(name)
        assert row['bar'] == 4.0 * row['fp32_vs_fp64_max'] and row['seed'] == R.CASES[name][0]
        assert now['excluded_fraction_max_per_frame'] <= R.EXCLUSION_CAP
        assert now['label_or_region_differences_outside'] == 0
        assert now['fp32_vs_fp64_max'] <= row['bar']
        assert 1e-6 < row['fp32_vs_fp64_max'] < 1e-4       # a few fp32 roundings of a coordinate of ~50 px on white noise
    assert 4.0 * rec['cases']['full_384']['fp32_vs_fp64_max'] == rec['cases']['full_384']['bar']


# ---------------------------------------------------------------------------------------------- workspace layouts
def test_python_layouts_end_where_the_workspace_queries_do(lib):
    """augment_layout / synth_layout restate aug_layout (csrc/augment.hip) and synth_layout (csrc/synth.hip): the totals are the
    C side's, the fields ascend, and the aligned ones sit on 256 bytes.  2x2: the smallest output; 21x40 and 24x33: partial tiles
    on either axis."""
    for B in (1, 2, 3):
        for T in (1, 2, 3):
            for Ho, Wo in ((2, 2), (21, 40), (24, 33)):
                lay = A.augment_layout(B, T, Ho, Wo)
                assert lay['total'] == lib.swem_augment_workspace(B, T, Ho, Wo), (B, T, Ho, Wo)
                assert lay['wlab'] == 0 and lay['wreg'] == B * T * Ho * Wo
                assert 2 * lay['wreg'] <= lay['presence'] < lay['partial'] < lay['total']
                assert lay['presence'] % 256 == 0 and lay['partial'] % 256 == 0
            for N in (1, 3, 7):
                lay = A.synth_layout(B, T, N)
                assert lay['total'] == lib.swem_synth_workspace(B, T, N), (B, T, N)
                assert lay['stats'] == 0 and B * N * 32 <= lay['plan'] < lay['total'] and lay['plan'] % 256 == 0


# ---------------------------------------------------------------------------------------------- C ABI: argument validation
def test_augment_entry_points_validate_before_any_hip_call(lib):
    assert lib.swem_augment_workspace(0, 3, 24, 40) == 0 and lib.swem_augment_workspace(2, 3, 24, -1) == 0
    px = 2 * 3 * 24 * 40
    tiles = 2 * 3                                        # ceil(40/32) * ceil(24/8)
    assert lib.swem_augment_workspace(2, 3, 24, 40) == 2 * px + 256 + (2 * 3 * tiles * 4 + 255) // 256 * 256 + \
        ((-2 * px) % 256)
    p = ctypes.c_void_p(4096)                            # non-null, aligned; never dereferenced: validation comes first

    def call(src=p, lab=p, params=p, frames=p, masks=p, valid=p, label=p, found=p, B=2, T=3, Hs=37, Ws=53, Ho=24, Wo=40, N=2,
             ws=p, ws_bytes=1 << 30):
        return lib.swem_augment_clips_u8(None, src, lab, params, frames, masks, valid, label, found, B, T, Hs, Ws, Ho, Wo, N, ws,
                                         ws_bytes)
    for name in ('src', 'lab', 'params', 'frames', 'masks', 'valid', 'label', 'found', 'ws'):
        assert call(**{name: None}) == -4 and b'null pointer' in lib.swem_last_error(), name
    assert call(params=ctypes.c_void_p(4098)) == -4 and b'aligned' in lib.swem_last_error()
    for kw in (dict(B=0), dict(T=-1), dict(Hs=0), dict(Ws=0)):
        assert call(**kw) == -1 and b'need B, T, Hs, Ws > 0' in lib.swem_last_error(), kw
    for kw in (dict(Ho=0), dict(Wo=1)):
        assert call(**kw) == -1 and b'at least 2x2' in lib.swem_last_error(), kw
    assert call(N=8) == -1 and b'N + 1 <= 8' in lib.swem_last_error()
    assert call(N=0) == -1 and b'1 <= N' in lib.swem_last_error()
    need = lib.swem_augment_workspace(2, 3, 24, 40)
    assert call(ws_bytes=need - 1) == -2 and b'workspace' in lib.swem_last_error()
