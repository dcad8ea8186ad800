"""GPU: result PNGs encoded on the device (include/swem_hip_io.h, csrc/png.hip).  No tolerance anywhere:
the strict reader of tests/png_ref.py and PIL must both give back the map and the palette that went in, byte for byte.  Every
blob has 64 guard bytes of 0xA5 behind its capacity, checked after every call."""
import io as pyio
import os

import numpy as np
import pytest
import torch
from PIL import Image

from swem_amd import io, ops
from tests import png_ref

pytestmark = pytest.mark.gpu

# (T, H, W): one pixel; a few bytes; a row of 260 bytes, just past one maximal match; more rows than one segment of 16 and a
# ragged last one; several segments of long rows
SHAPES = [(1, 1, 1), (2, 3, 5), (2, 17, 259), (3, 33, 300), (2, 70, 854)]
KINDS = ['zeros', 'full', 'labels3', 'noise256', 'blobs', 'ladder']
LADDER = [1, 2, 3, 4, 5, 257, 258, 259, 260, 261, 262, 516, 517, 518, 519]
GUARD = 64


def make_map(kind, H, W, seed=0):
    rng = np.random.RandomState(seed)
    if kind == 'zeros':
        return np.zeros((H, W), np.uint8)
    if kind == 'full':
        return np.full((H, W), 255, np.uint8)
    if kind == 'labels3':
        return rng.randint(0, 3, (H, W)).astype(np.uint8)
    if kind == 'noise256':
        return rng.randint(0, 256, (H, W)).astype(np.uint8)
    if kind == 'blobs':
        # two discs whose edges are roughened row by row and pixel by pixel
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        m = np.zeros((H, W), np.uint8)
        for label, (cy, cx, r) in enumerate([(0.4, 0.3, 0.30), (0.6, 0.7, 0.25)], 1):
            rough = rng.uniform(-0.04, 0.04, (H, 1)) + rng.uniform(-0.02, 0.02, (H, W))
            m[np.hypot((y / max(H, 1) - cy), (x / max(W, 1) - cx)) < r + rough] = label
        return m
    if kind == 'ladder':
        # runs of the LADDER lengths over the flattened rows, alternating 7 / 200, repeated until the map is full: remainders
        # of 1 and 2 after a maximal match, runs across rows and segments, 8- and 9-bit literals
        flat = np.empty(H * W, np.uint8)
        pos, k = 0, 0
        while pos < flat.size:
            n = LADDER[k % len(LADDER)]
            flat[pos:pos + n] = 7 if k % 2 == 0 else 200
            pos += n
            k += 1
        return flat.reshape(H, W)
    raise KeyError(kind)


def calls_of(shape):
    """The calls that put every kind of content through a shape, a different one in each frame of a call: [(kinds, maps)]."""
    T, H, W = shape
    out = []
    for k0 in range(0, len(KINDS), T):
        kinds = [KINDS[(k0 + f) % len(KINDS)] for f in range(T)]
        out.append((kinds, np.stack([make_map(k, H, W, seed=17 * k0 + f) for f, k in enumerate(kinds)])))
    return out


def encode(maps_np, palette):
    """ops.png_encode_u8 into a guarded blob -> (files as bytes, offsets as a list)."""
    T, H, W = maps_np.shape
    cap = io.png_capacity(H, W)
    buf = torch.full((T * cap + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    blob, offsets = ops.png_encode_u8(torch.from_numpy(maps_np).cuda(), palette, blob=buf[:T * cap])
    assert blob.data_ptr() == buf.data_ptr()
    offs = offsets.cpu().tolist()
    host = buf.cpu().numpy()
    assert (host[T * cap:] == 0xA5).all(), 'the encoder wrote behind the blob'
    assert len(offs) == T + 1
    return [host[offs[t]:offs[t + 1]].tobytes() for t in range(T)], offs


_cache = {}


def encoded(shape, with_palette):
    """Every call of a shape, encoded once and shared by the tests below."""
    key = (shape, with_palette)
    if key not in _cache:
        pal = np.asarray(io.default_palette(), np.uint8) if with_palette else None
        _cache[key] = [(kinds, maps) + encode(maps, pal) for kinds, maps in calls_of(shape)]
    return _cache[key]


@pytest.mark.parametrize('with_palette', [True, False], ids=['palette', 'gray'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_round_trip_byte_for_byte(lib, shape, with_palette):
    T, H, W = shape
    pal = np.asarray(io.default_palette(), np.uint8).reshape(256, 3)
    seen = set()
    for kinds, maps, files, _offs in encoded(shape, with_palette):
        for t in range(T):
            got, got_pal, n_idat, sizes = png_ref.parse_png(files[t])
            assert np.array_equal(got, maps[t]), (kinds[t], shape)
            assert sizes['raw'] == H * (W + 1) and n_idat >= 2
            img = Image.open(pyio.BytesIO(files[t]))
            img.load()
            if with_palette:
                assert np.array_equal(got_pal, pal)
                assert img.mode == 'P' and np.array_equal(np.asarray(img.getpalette(), np.uint8).reshape(-1, 3), pal)
            else:
                assert got_pal is None and img.mode == 'L'
            assert np.array_equal(np.asarray(img), maps[t]), (kinds[t], shape)
            seen.add(kinds[t])
    assert seen == set(KINDS)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_offsets_sizes_and_determinism(lib, shape):
    T, H, W = shape
    cap = io.png_capacity(H, W)
    pal = np.asarray(io.default_palette(), np.uint8)
    for _kinds, maps, files, offs in encoded(shape, True):
        assert offs[0] == 0 and all(b >= a for a, b in zip(offs, offs[1:]))
        assert all(0 < len(f) <= cap for f in files)
        again, offs2 = encode(maps, pal)
        assert offs2 == offs and again == files


def test_run_length_coding_is_real(lib):
    """One constant 480x854 map is at most 1/50 of its stored size (13 bits per 258 bytes would give ~2.6 KB + 0.8 KB of
    headers; one segment per row ~13.8 KB, which fails); 256-value noise stays within the capacity, its stored form."""
    H, W = 480, 854
    pal = np.asarray(io.default_palette(), np.uint8)
    for value in (0, 255, 1):
        (f,), _ = encode(np.full((1, H, W), value, np.uint8), pal)
        print('constant %d: %d bytes' % (value, len(f)))
        assert len(f) <= H * (W + 1) // 50 == 8208
        assert np.array_equal(png_ref.parse_png(f)[0], np.full((H, W), value, np.uint8))
    noise = make_map('noise256', H, W, seed=3)[None]
    (f,), _ = encode(noise, pal)
    print('noise: %d bytes, capacity %d' % (len(f), io.png_capacity(H, W)))
    assert H * (W + 1) < len(f) <= io.png_capacity(H, W)
    assert np.array_equal(png_ref.parse_png(f)[0], noise[0])


def _read_dir(d):
    out = {}
    for name in sorted(os.listdir(d)):
        img = Image.open(os.path.join(d, name))
        img.load()
        out[name] = (img.mode, np.asarray(img).copy(), img.getpalette())
    return out


def test_writer_device_files_equal_host_files(lib, tmp_path):
    H, W, n = 20, 30, 4
    rng = np.random.RandomState(5)
    preds = [torch.from_numpy(rng.randint(0, 3, (1, H, W)).astype(np.int64)).cuda() for _ in range(n)]
    preds[1][:, 5:15, 3:25] = 2                       # some runs among the noise
    first = torch.zeros(1, 3, H, W, device='cuda')
    first[0, 0] = 1
    first[0, 0, 4:9, 6:20] = 0
    first[0, 2, 4:9, 6:20] = 1
    id_table = np.array([0, 5, 9], np.uint8)
    names = ['f%03d' % (3 * k) for k in range(8)]
    keep = {names[2], names[4], names[5]}
    frames = rng.randint(0, 256, (n + 1, H, W, 3)).astype(np.uint8)
    counts, dirs = {}, {}
    for mode in ('host', 'device'):
        w = io.IndexMapWriter(str(tmp_path / mode), encode=mode)
        w.save_first('seq', first, id_table=id_table, name=names[0])
        w.submit('seq', preds, first_index=2, id_table=id_table, names=names, keep=keep)
        w.save_first('all', first, overlay_frame_u8=frames[0])
        w.submit('all', preds, first_index=1, keep={1, 2, 4}, overlay_frames_u8=frames)
        w.submit('run', preds, keep={2, 3})               # neighbours: a slice of the maps; 'every': all of them as they are
        w.submit('every', preds)
        counts[mode] = w.close()
        dirs[mode] = {s: _read_dir(str(tmp_path / mode / s)) for s in ('seq', 'all', 'run', 'every', os.path.join('overlay', 'all'))}
    assert counts['device'] == counts['host'] == 3 + 3 + 2 + n
    assert sorted(dirs['host']['run']) == ['00002.png', '00003.png'] and len(dirs['host']['every']) == n
    assert sorted(dirs['host']['seq']) == [names[0] + '.png'] + sorted(k + '.png' for k in keep)
    assert sorted(dirs['host']['all']) == ['00000.png', '00001.png', '00002.png', '00004.png']
    assert sorted(dirs['host'][os.path.join('overlay', 'all')]) == ['%05d.png' % t for t in range(n + 1)]
    for s in dirs['host']:
        assert sorted(dirs['device'][s]) == sorted(dirs['host'][s])
        for name, (mode, arr, pal) in dirs['host'][s].items():
            dmode, darr, dpal = dirs['device'][s][name]
            assert dmode == mode == ('RGB' if 'overlay' in s else 'P') and np.array_equal(darr, arr) and dpal == pal, (s, name)
    assert set(np.unique(dirs['device']['seq'][names[2] + '.png'][1])) <= {0, 5, 9}
    # the device files are the encoder's own: the strict reader takes them too
    with open(str(tmp_path / 'device' / 'seq' / (names[0] + '.png')), 'rb') as f:
        got = png_ref.parse_png(f.read())[0]
    assert np.array_equal(got, dirs['host']['seq'][names[0] + '.png'][1])


def test_capture_and_replay_on_new_maps(lib):
    T, H, W = 2, 33, 300
    pal = np.asarray(io.default_palette(), np.uint8)
    a = np.stack([make_map('blobs', H, W, 1), make_map('ladder', H, W)])
    b = np.stack([make_map('noise256', H, W, 2), make_map('labels3', H, W, 3)])
    static = torch.from_numpy(a).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.png_encode_u8(static, pal)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, **ops.graph_capture_kwargs()):
        blob, offsets = ops.png_encode_u8(static, pal)
    for maps in (a, b):
        static.copy_(torch.from_numpy(maps).cuda())
        g.replay()
        torch.cuda.synchronize()
        offs = offsets.cpu().tolist()
        host = blob.cpu().numpy()
        eager, eoffs = encode(maps, pal)
        assert offs == eoffs
        for t in range(T):
            assert host[offs[t]:offs[t + 1]].tobytes() == eager[t]
            assert np.array_equal(png_ref.parse_png(eager[t])[0], maps[t])
