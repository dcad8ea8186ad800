"""GPU: evaluation staging from decoded bytes (csrc/stage.hip, include/swem_hip_io.h, swem_amd/io.py) against tests/io_ref.py.
Frames: within 2 ulp of 1.0 of what today's path (resize_planes(u8.float() / 255, 'bicubic')) leaves against float64, and exact
where the resize is the identity.  One-hot masks, id-mapped index maps and overlay pictures: equal byte for byte."""
import os

import numpy as np
import pytest
import torch

from swem_amd import io, ops
from tests import io_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP1 = 2.0 ** -23            # one ulp of 1.0 in fp32 (1.19e-7)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def record(key, data):
    from tests import helpers as H
    H.record_parity('io_' + key, data)


# ------------------------------------------------------------------------------------------------------------- frames
def stage_case(T, hs, ws, ho, wo, seed):
    """The new kernel and today's path on the same bytes, both against float64: the figures of profiles/io_device.json."""
    u8 = np.random.default_rng(seed).integers(0, 256, (T, hs, ws, 3), dtype=np.uint8)
    ref = io_ref.stage_frames64(u8, (ho, wo))
    d = dev(u8)
    new = ops.stage_frames_u8(d, (ho, wo))
    old = ops.resize_planes((d.permute(0, 3, 1, 2).float() / 255).contiguous(), (ho, wo), 'bicubic')
    assert new.shape == old.shape == (T, 3, ho, wo) and new.dtype == torch.float32
    e_new = float(np.abs(new.cpu().numpy().astype(np.float64) - ref).max())
    e_old = float(np.abs(old.cpu().numpy().astype(np.float64) - ref).max())
    return {'case': 'T=%d %dx%d -> %dx%d' % (T, hs, ws, ho, wo), 'max_abs_err_new': e_new, 'max_abs_err_today': e_old,
            'bit_equal': bool(torch.equal(new, old))}


STAGE_CASES = [(2, 5, 7, 8, 12), (2, 9, 13, 4, 6), (2, 480, 854, 480, 864)]


@pytest.mark.parametrize('T,hs,ws,ho,wo', STAGE_CASES, ids=['up_5x7', 'down_9x13', 'davis_480x854'])
def test_stage_frames_vs_float64(lib, T, hs, ws, ho, wo):
    row = stage_case(T, hs, ws, ho, wo, seed=hs * 100 + ws)
    print(row)
    record('stage_%dx%d' % (hs, ws), row)
    assert row['max_abs_err_new'] <= row['max_abs_err_today'] + 2 * ULP1, row
    # the yardstick itself is the same resize (a wrong one would show here).  What separates fp32 from float64 is mostly the
    # SOURCE COORDINATE, which ATen's convention forms in fp32: two roundings at up to one ulp of the largest coordinate, times
    # the interpolant's slope (at most 2 per pixel on data in [0,1]); the tap sum adds a few ulp of 1.0
    coord_ulp = float(np.spacing(np.float32(max(hs, ws) - 1)))
    assert row['max_abs_err_today'] < 2 * 2 * coord_ulp + 1e-5, row


def test_stage_frames_identity_pins_the_division(lib):
    """6x10 -> 6x10: the weights are (0,1,0,0) exactly, so every output is fp32(b) / fp32(255), correctly rounded."""
    u8 = (np.arange(2 * 6 * 10 * 3) % 256).astype(np.uint8).reshape(2, 6, 10, 3)
    assert len(np.unique(u8)) == 256
    got = ops.stage_frames_u8(dev(u8), (6, 10)).cpu().numpy()
    want = (np.arange(256, dtype=np.float32) / 255)[u8].transpose(0, 3, 1, 2)
    assert want.dtype == np.float32 and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------- one-hot
def _label_map(rng, h, w, labels):
    m = rng.choice(np.asarray(labels, np.uint8), size=(h, w))
    m.reshape(-1)[:len(labels)] = labels          # every label at least once (h * w >= len(labels))
    return m


@pytest.mark.parametrize('h,w', [(3, 5), (7, 9), (8, 12)], ids=['3x5', '7x9', '8x12_vector'])
def test_onehot_equals_io_ref(lib, h, w):
    rng = np.random.default_rng(h * 31 + w)
    # DAVIS tables: C = 2, a gap in the ids (C = 4), single_obj, C = 12
    for labels, single in (([0, 1], False), ([0, 1, 3], False), ([0, 1, 3, 5], True), ([0, 2, 5, 11], False),
                           (list(range(12)), False)):
        first = _label_map(rng, h, w, labels)
        table, obj_n = io.davis_table(first, single)
        got = ops.labels_onehot_u8(dev(first), table, obj_n).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, io_ref.onehot_davis(first, single)), (labels, single)
        other = _label_map(rng, h, w, labels + [7, 200, 255])          # unlisted ids and 255: background
        got = ops.labels_onehot_u8(dev(other), table, obj_n).cpu().numpy()
        assert np.array_equal(got, io_ref.apply_table(other, table, obj_n)) and np.array_equal(got.sum(0), np.ones((h, w)))
    # YouTube-VOS tables: C = 2 and C = 12; labels of objects annotated earlier, unlisted ids and 255 in no channel
    for ids in ([3], [9, 2, 4, 1, 5, 6, 7, 8, 10, 11, 12]):
        lab = _label_map(rng, h, w, [0] + ids[:3] + [13, 200, 255])
        got = ops.labels_onehot_u8(dev(lab), io.ytvos_table(ids), len(ids) + 1).cpu().numpy()
        want = io_ref.onehot_ytvos(lab, ids)
        assert got.shape == (len(ids) + 1, h, w) and np.array_equal(got, want) and want.sum(0).min() == 0


# ------------------------------------------------------------------------------------------------------------- LUT pack
@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 1023, 1024, 1027])
def test_pack_lut_equals_map_mask(lib, n):
    rng = np.random.default_rng(n)
    # (tables of up to 32 ids are looked up in registers, longer ones in memory: both sides of that threshold)
    for ids in ([0, 4, 1, 2, 7], [0], list(range(40, 72)), list(range(40, 73)), list(range(255, -1, -1))):
        idx = rng.integers(0, len(ids) + 3, n).astype(np.int64)
        idx[0] = len(ids)                                  # the first index beyond the table
        want = io_ref.map_mask(idx, ids)
        assert (want[idx >= len(ids)] == 0).all()
        got = ops.pack_u8_lut(dev(idx), np.asarray(ids, np.uint8)).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want), (n, ids[:5])


# ------------------------------------------------------------------------------------------------------------- overlay
PAL = np.asarray(io.default_palette(), np.uint8).reshape(256, 3)


def overlay_equal(frames, labels, pal=PAL, alpha=0.4):
    got = ops.overlay_u8(dev(frames), dev(labels), pal, alpha).cpu().numpy()
    for t in range(frames.shape[0]):
        want = io_ref.add_overlay(frames[t], labels[t], pal, alpha)
        assert np.array_equal(got[t], want), (t, np.argwhere(got[t] != want)[:5])
    return got


def test_overlay_every_byte_and_colour_pair(lib):
    """(a) 256x1024, 4-column stripes of labels 0..255, the image byte = the row: all 65,536 (byte, colour byte) pairs are
    blended at pixels that are no contour -- the float64, uncontracted blend is pinned pair by pair."""
    lab = np.repeat(np.arange(256, dtype=np.uint8), 4)[None].repeat(256, 0)                    # (256, 1024)
    img = np.arange(256, dtype=np.uint8)[:, None, None].repeat(1024, 1).repeat(3, 2)          # byte = row
    L = np.arange(256)
    pal = np.stack([(L + 1) % 256, (L * 7 + 3) % 256, 255 - L], 1).astype(np.uint8)
    got = overlay_equal(img[None], lab[None], pal)[0]
    blended = np.zeros(lab.shape, bool)
    blended[:, 4:] = (np.arange(4, 1024) % 4 != 3)[None]           # label 0 is the smallest: untouched; column 3 of a stripe
    blended[:, 1023] = True                                         # is the next object's contour, but nothing follows 255
    assert (got[~blended & (lab > 0)] == 0).all() and (got[:, 3] == 0).all() and np.array_equal(got[:, :3], img[:, :3])
    pairs = set()
    for c in range(3):
        pairs.update((img[..., c][blended].astype(np.int64) * 256 + pal[lab[blended], c]).tolist())
    assert len(pairs) == 65536


def test_overlay_shapes_of_objects(lib):
    """(b) two touching objects in both id orders, an object on all four image edges, a single-pixel object."""
    rng = np.random.default_rng(3)
    lab = np.zeros((2, 13, 18), np.uint8)
    for t, (a, b) in enumerate(((1, 2), (2, 1))):
        lab[t, 3:8, 2:7] = a
        lab[t, 3:8, 7:12] = b                  # touching along a column
        lab[t, 8:10, 4:9] = b                  # and along a row
        lab[t, 0, :] = lab[t, -1, :] = lab[t, :, 0] = lab[t, :, -1] = 3        # a ring on all four edges
        lab[t, 5, 15] = 4                      # one pixel
        lab[t, 11, 9] = 4
    img = rng.integers(0, 256, lab.shape + (3,), dtype=np.uint8)
    got = overlay_equal(img, lab)
    assert (got[0, 5, 14] == 0).all() and not np.array_equal(got[0, 5, 15], img[0, 5, 15])


@pytest.mark.parametrize('h,w', [(1, 1), (1, 7), (1, 12), (5, 1)])
def test_overlay_thin_frames(lib, h, w):
    """(c) 1x1 and 1xW frames (and Hx1): no neighbour above or below, the scalar tail only."""
    rng = np.random.default_rng(h * 10 + w)
    lab = rng.choice(np.array([0, 1, 2], np.uint8), size=(2, h, w))
    lab[1] = 2 if h * w == 1 else lab[1]
    overlay_equal(rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8), lab)


def test_overlay_without_background_and_differing_smallest_labels(lib):
    """(d) a frame with no label 0: the smallest OBJECT is what ids[1:] skips.  (e) T = 2 frames whose smallest labels
    differ, at a frame size that is a multiple of four (word path) and one that is not (byte path)."""
    rng = np.random.default_rng(11)
    for h, w in ((10, 12), (9, 7)):
        lab = np.zeros((2, h, w), np.uint8)
        lab[0] = np.repeat(np.repeat(rng.choice(np.array([2, 3, 5], np.uint8), size=(4, 4)), 3, 0), 3, 1)[:h, :w]
        lab[1] = np.repeat(np.repeat(rng.choice(np.array([0, 2, 3], np.uint8), size=(4, 4)), 3, 0), 3, 1)[:h, :w]
        lab[0, 0, 0], lab[1, 0, 0] = 2, 0
        assert lab[0].min() == 2 and lab[1].min() == 0
        img = rng.integers(0, 256, lab.shape + (3,), dtype=np.uint8)
        got = overlay_equal(img, lab)
        inner = lab[0] == 2                     # label 2 is frame 0's smallest: never blended there, blended in frame 1
        assert ((got[0][inner] == img[0][inner]).all(1) | (got[0][inner] == 0).all(1)).all()
        overlay_equal(img, lab, alpha=0.25)
        # frame 1 alone as a device view: at 9x7 it starts off a word boundary and takes the byte path
        alone = ops.overlay_u8(dev(img)[1:], dev(lab)[1:], PAL, 0.4).cpu().numpy()
        assert np.array_equal(alone[0], got[1])


# ------------------------------------------------------------------------------------------------------------- end to end
def _model(wseed):
    from oracle import swem_oracle as O
    from tests import helpers as H
    cfg = O.make_cfg(BACKBONE='resnet18', NUM_BASES=64, NUM_EM_ITERS=3, SINGLE_OBJ=False)
    model, _ = H.make_model_and_sd(cfg, wseed, device=DEV)
    return model


def test_davis_loop_from_bytes_writes_maps_and_overlays(lib, tmp_path):
    """Plumbing only: davis_sequence_u8 -> evaluate_davis_seq -> submit(overlay_frames_u8=): the files exist and decode."""
    from PIL import Image
    from swem_amd import evaluator
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, (3, 64, 96, 3), dtype=np.uint8)
    first = np.zeros((64, 96), np.uint8)
    first[10:40, 12:50] = 1
    first[30:60, 55:90] = 3                    # a gap in the ids: obj_n = 4, id 3 in channel 2
    in_frames, in_masks, obj_n = io.davis_sequence_u8(frames, first, size=(64, 96))
    assert obj_n == 4 and in_frames.shape == (1, 3, 3, 64, 96) and in_masks[0].shape == (1, 4, 64, 96) and in_masks[1] is None
    assert np.array_equal(in_masks[0][0].cpu().numpy(), io_ref.onehot_davis(first))
    model = _model(5)
    with torch.no_grad():
        torch.manual_seed(3)
        preds, _ = evaluator.evaluate_davis_seq(model, in_frames, in_masks, (64, 96))
    w = io.IndexMapWriter(str(tmp_path))
    w.submit('seq', preds, overlay_frames_u8=frames)
    w.save_first('seq', in_masks[0], overlay_frame_u8=frames[0])
    assert w.close() == 2
    for t in range(3):
        m = np.array(Image.open(str(tmp_path / 'seq' / ('%05d.png' % t))))
        o = np.array(Image.open(str(tmp_path / 'overlay' / 'seq' / ('%05d.png' % t))))
        assert m.shape == (64, 96) and m.dtype == np.uint8 and o.shape == (64, 96, 3) and o.dtype == np.uint8
        if t > 0:
            assert np.array_equal(m, preds[t - 1][0].cpu().numpy().astype(np.uint8))
        assert np.array_equal(o, io_ref.add_overlay(frames[t], m, PAL))
    assert sorted(os.listdir(str(tmp_path / 'overlay' / 'seq'))) == ['00000.png', '00001.png', '00002.png']


def test_ytvos_loop_from_bytes_writes_the_kept_names_with_object_ids(lib, tmp_path):
    """Plumbing only: ytvos_sequence_u8 with an object that first appears at frame 1 -> evaluate_ytvos_seq ->
    submit(id_table=, names=, keep=): only the kept basenames, pixel values drawn from the id table."""
    from PIL import Image
    from swem_amd import evaluator
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (3, 60, 100, 3), dtype=np.uint8)
    lab0 = np.zeros((60, 100), np.uint8)
    lab0[8:30, 10:45] = 2
    lab1 = lab0.copy()                          # the earlier object is still in the later annotation: no channel there
    lab1[35:55, 50:90] = 5
    ann = {0: (lab0, [2]), 1: (lab1, [5])}
    in_frames, init_masks, id_table = io.ytvos_sequence_u8(frames, ann)
    assert in_frames.shape == (1, 3, 3, 64, 96) and id_table.tolist() == [0, 2, 5]
    assert init_masks[0].shape == (1, 2, 60, 100) and init_masks[1].shape == (1, 2, 60, 100) and init_masks[2] is None
    assert np.array_equal(init_masks[1][0].cpu().numpy(), io_ref.onehot_ytvos(lab1, [5]))
    model = _model(6)
    with torch.no_grad():
        torch.manual_seed(3)
        preds = evaluator.evaluate_ytvos_seq(model, in_frames, init_masks, (60, 100))
    names = ['00000', '00005', '00010']
    w = io.IndexMapWriter(str(tmp_path))
    w.save_first('vid', init_masks[0], id_table=id_table, name=names[0])
    w.submit('vid', preds, id_table=id_table, names=names, keep=['00000', '00010'], overlay_frames_u8=frames)
    assert w.close() == 1
    assert sorted(os.listdir(str(tmp_path / 'vid'))) == ['00000.png', '00010.png']
    assert sorted(os.listdir(str(tmp_path / 'overlay' / 'vid'))) == ['00005.png', '00010.png']
    first = np.array(Image.open(str(tmp_path / 'vid' / '00000.png')))
    assert np.array_equal(first, lab0)
    last = np.array(Image.open(str(tmp_path / 'vid' / '00010.png')))
    assert last.shape == (60, 100) and set(np.unique(last).tolist()) <= {0, 2, 5}
    assert np.array_equal(last, io_ref.map_mask(preds[1][0].cpu().numpy(), id_table.tolist()))
    o = np.array(Image.open(str(tmp_path / 'overlay' / 'vid' / '00010.png')))
    assert np.array_equal(o, io_ref.add_overlay(frames[2], last, PAL))
