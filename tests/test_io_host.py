"""CPU: the host side of evaluation staging from decoded bytes (swem_amd/io.py, include/swem_hip_io.h).
  * tests/io_ref.py (the yardstick of tests/test_gpu_io.py) against what the reference's own functions gave (g10_io.npz,
    tests/golden/make_golden_io.py);
  * the channel / id tables and the YouTube-VOS input size against io_ref, the fixture and hand-derived sizes;
  * every new entry point refuses null pointers and bad shapes before any HIP call;
  * the per-pixel closed form of the overlay against the sequential loop."""
import ctypes
import os

import numpy as np
import pytest

from swem_amd import _lib, io
from tests import io_ref

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'g10_io.npz')


@pytest.fixture(scope='module')
def fx():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_io_ref_overlay_equals_the_reference(fx):
    assert int(fx['ov_n']) >= 8
    for k in range(int(fx['ov_n'])):
        img, mask, want, alpha = fx['ov%d_img' % k], fx['ov%d_mask' % k], fx['ov%d_out' % k], float(fx['ov%d_alpha' % k])
        assert np.array_equal(io_ref.add_overlay(img, mask, fx['palette'], alpha), want), k
        assert np.array_equal(io_ref.overlay_closed(img, mask, fx['palette'], alpha), want), k


def test_io_ref_onehot_and_tables_equal_the_reference(fx):
    assert int(fx['oh_n']) >= 10
    for k in range(int(fx['oh_n'])):
        mask, single, want = fx['oh%d_mask' % k], bool(fx['oh%d_single' % k]), fx['oh%d_out' % k].astype(np.float32)
        assert np.array_equal(io_ref.onehot_davis(mask, single), want), k
        table, obj_n = io.davis_table(mask, single)
        assert obj_n == want.shape[0] and table.dtype == np.uint8 and table.shape == (256,)
        assert np.array_equal(io_ref.apply_table(mask, table, obj_n), want), k


def test_davis_table_compacts_and_sends_unlisted_labels_to_the_background():
    mask = np.array([[0, 1, 3, 3], [1, 0, 0, 3]], np.uint8)
    table, obj_n = io.davis_table(mask)
    assert obj_n == 4 and table[1] == 1 and table[3] == 2 and table[2] == 0 and table[255] == 0 and table[0] == 0
    # a later map with labels the first frame did not have: the reference's background is "1 - sum", so they are background
    other = np.array([[2, 255, 3, 7]], np.uint8)
    got = io_ref.apply_table(other, table, obj_n)
    assert np.array_equal(got[:, 0], np.array([[1, 1, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]], np.float32))
    ts, ns = io.davis_table(mask, single_obj=True)
    assert ns == 2 and ts[0] == 0 and (ts[1:] == 1).all()
    t0, n0 = io.davis_table(np.zeros((2, 2), np.uint8), single_obj=True)
    assert n0 == 1 and not t0.any()
    with pytest.raises(ValueError):
        io.davis_table(np.array([[0, 255]], np.uint8))
    with pytest.raises(TypeError):
        io.davis_table(np.array([[0, 1]], np.int64))


def test_ytvos_tables_against_io_ref():
    rng = np.random.default_rng(5)
    mask = rng.choice(np.array([0, 1, 2, 4, 7, 255], np.uint8), size=(7, 9))
    for ids in ([2], [4, 1], [7, 2, 1, 4]):
        table = io.ytvos_table(ids)
        assert table[0] == 0 and table[255] == 255 and table[3] == 255
        want = io_ref.onehot_ytvos(mask, ids)
        assert np.array_equal(io_ref.apply_table(mask, table, len(ids) + 1), want)
        assert want.sum(0).min() == 0            # labels of objects annotated earlier sit in no channel
    ann = {4: (mask, [7]), 0: (mask, [4, 1]), 2: (mask, [2])}
    assert io.ytvos_id_table(ann).tolist() == io_ref.id_list(ann) == [0, 4, 1, 2, 7]
    assert io.ytvos_id_table(ann).dtype == np.uint8
    idx = rng.integers(0, 7, (5, 6))
    want = io_ref.map_mask(idx, io_ref.id_list(ann))
    assert want.max() == 7 and (want[idx >= 5] == 0).all()
    for bad in ([0], [3, 3], [256], list(range(1, 256))):
        with pytest.raises(ValueError):
            io.ytvos_table(bad)


def test_ytvos_input_size(fx):
    for s, want in zip(fx['suit_in'].tolist(), fx['suit_out'].tolist()):
        assert io.get_suit_size(s) == want == io_ref.suit_size(s)
    assert io.get_suit_size(495) == 496
    assert io.ytvos_input_size(720, 1280) == (496, 880)
    assert io.ytvos_input_size(1280, 720) == (880, 496)
    assert io.ytvos_input_size(360, 640) == (368, 640)
    rng = np.random.default_rng(9)
    for _ in range(400):
        h, w, ss = int(rng.integers(17, 2200)), int(rng.integers(17, 2200)), int(rng.choice([495, 480, 360, 600]))
        got = io.ytvos_input_size(h, w, ss)
        assert got == io_ref.input_size(h, w, ss) and got[0] % 16 == 0 and got[1] % 16 == 0
    assert io.ytvos_input_size(500, 500) == io_ref.input_size(500, 500) == (496, 496)


def test_closed_form_overlay_equals_the_sequential_loop():
    rng = np.random.default_rng(77)
    pal = np.asarray(io.default_palette(), np.uint8).reshape(256, 3)
    for n in range(200):
        h, w = int(rng.integers(1, 16)), int(rng.integers(1, 16))
        labels = rng.choice(np.arange(0, 9), size=int(rng.integers(1, 6)), replace=False)
        mask = rng.choice(labels, size=(h, w)).astype(np.uint8)
        if n % 3 == 0:                     # larger blobs: interiors that blend, not only contours
            mask = np.repeat(np.repeat(mask, 3, 0), 3, 1)[:h, :w]
        img = rng.integers(0, 256, mask.shape + (3,), dtype=np.uint8)
        alpha = float(rng.choice([0.4, 0.25, 0.7, 0.0, 1.0]))
        assert np.array_equal(io_ref.overlay_closed(img, mask, pal, alpha), io_ref.add_overlay(img, mask, pal, alpha)), n


def test_stage_frames_ref_identity_and_range():
    u8 = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3)
    same = io_ref.stage_frames64(u8, (16, 16))
    assert np.array_equal(same[0, 0], np.arange(256).reshape(16, 16) / 255.0)
    up = io_ref.stage_frames64(np.full((1, 5, 7, 3), 200, np.uint8), (8, 12))
    assert np.abs(up - 200 / 255.0).max() < 1e-15      # the weights sum to one


def test_entry_points_check_their_arguments_without_a_gpu(lib):
    buf = (ctypes.c_ubyte * 4096)()
    p = ctypes.addressof(buf)
    tab = bytes(256)
    pal = bytes(768)
    f = lib.swem_stage_frames_u8
    assert f(None, None, p, 1, 4, 4, 4, 4) == -4 and b'null pointer' in lib.swem_last_error()
    assert f(None, p, None, 1, 4, 4, 4, 4) == -4
    assert f(None, p, p, 0, 4, 4, 4, 4) == -1 and b'stage_frames' in lib.swem_last_error()
    assert f(None, p, p, 1, 4, 4, 0, 4) == -1 and f(None, p, p, 1, 4, -1, 4, 4) == -1
    g = lib.swem_labels_onehot_u8
    assert g(None, None, tab, p, 2, 4, 4) == -4 and g(None, p, None, p, 2, 4, 4) == -4 and g(None, p, tab, None, 2, 4, 4) == -4
    assert b'null pointer' in lib.swem_last_error()
    assert g(None, p, tab, p, 0, 4, 4) == -1 and g(None, p, tab, p, 256, 4, 4) == -1 and g(None, p, tab, p, 2, 0, 4) == -1
    assert b'labels_onehot' in lib.swem_last_error()
    h = lib.swem_pack_u8_lut_i64
    p16 = (p + 15) // 16 * 16
    assert h(None, None, p16, 4, tab, 2) == -4 and h(None, p16, None, 4, tab, 2) == -4 and h(None, p16, p16, 4, None, 2) == -4
    assert h(None, p16, p16 + 1, 4, tab, 2) == -4 and b'aligned' in lib.swem_last_error()
    assert h(None, p16, p16, 0, tab, 2) == -1 and h(None, p16, p16, 4, tab, 0) == -1 and h(None, p16, p16, 4, tab, 257) == -1
    assert lib.swem_overlay_workspace(0) == 0 and lib.swem_overlay_workspace(-3) == 0 and lib.swem_overlay_workspace(70) >= 280
    o = lib.swem_overlay_u8
    a, b = ctypes.c_double(0.4), ctypes.c_double(1 - 0.4)
    assert o(None, None, p, pal, a, b, p, 1, 4, 4, p16, 64) == -4 and o(None, p, None, pal, a, b, p, 1, 4, 4, p16, 64) == -4
    assert o(None, p, p, None, a, b, p, 1, 4, 4, p16, 64) == -4 and o(None, p, p, pal, a, b, None, 1, 4, 4, p16, 64) == -4
    assert o(None, p, p, pal, a, b, p, 1, 4, 4, None, 64) == -4
    assert o(None, p, p, pal, ctypes.c_double(1.5), b, p, 1, 4, 4, p16, 64) == -4 and b'alpha' in lib.swem_last_error()
    assert o(None, p, p, pal, ctypes.c_double(float('nan')), b, p, 1, 4, 4, p16, 64) == -4
    assert o(None, p, p, pal, a, b, p, 0, 4, 4, p16, 64) == -1 and o(None, p, p, pal, a, b, p, 1, 0, 4, p16, 64) == -1
    assert o(None, p, p, pal, a, b, p, 70000, 4, 4, p16, 1 << 20) == -1
    assert o(None, p, p, pal, a, b, p, 2, 4, 4, p16, 4) == -2 and b'workspace' in lib.swem_last_error()
    with pytest.raises(_lib.SwemHipError, match='null pointer'):
        _lib.call('swem_stage_frames_u8', None, None, None, 1, 4, 4, 4, 4)
