"""GPU: the second form of the device PNG encoder (swem_png_encode_px_u8, csrc/png.hip: dynamic Huffman tables per segment,
truecolour pictures with adaptive scanline filters).  No tolerance: the strict reader of
tests/png_ref_px.py and PIL give back what went in, byte for byte; the files equal those of the host program
(tests/png_dyn_host.cpp) and, for one-channel fixed codes, those of the first entry point.  Every blob has 64 guard bytes of
0xA5 behind its capacity, checked after every call."""
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from swem_amd import _lib, io, ops
from tests import png_dyn_cases as C
from tests import png_ref_px
from tests.test_gpu_png import SHAPES, calls_of, make_map

pytestmark = pytest.mark.gpu

GUARD = 64


def encode_px(px_np, palette, codes):
    """swem_png_encode_px_u8 itself (ops.png_encode_u8 sends its default call to the first entry point) into a guarded blob ->
    (files as bytes, offsets as a list)."""
    T, H, W = px_np.shape[:3]
    channels = 3 if px_np.ndim == 4 else 1
    cap = io.png_capacity(H, W, channels)
    px = torch.from_numpy(px_np).cuda()
    buf = torch.full((T * cap + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    offsets = torch.empty(T + 1, dtype=torch.int64, device='cuda')
    nbytes = _lib.query('swem_png_workspace_px', T, H, W, channels)
    ws = ops.workspace(nbytes, px.device)
    pal = None if palette is None else np.asarray(palette, np.uint8).tobytes()
    _lib.call('swem_png_encode_px_u8', ops._stream(), px.data_ptr(), channels, pal, ops.PNG_CODES[codes], buf.data_ptr(), T * cap,
              offsets.data_ptr(), T, H, W, ws.data_ptr(), nbytes)
    offs = offsets.cpu().tolist()
    host = buf.cpu().numpy()
    assert (host[T * cap:] == 0xA5).all(), 'the encoder wrote behind the blob'
    assert len(offs) == T + 1 and offs[0] == 0 and all(b > a for a, b in zip(offs, offs[1:])) and offs[-1] <= T * cap
    return [host[offs[t]:offs[t + 1]].tobytes() for t in range(T)], offs


def calls(shape, channels):
    pal = np.asarray(io.default_palette(), np.uint8)
    if channels == 1:
        return [(kinds, maps, pal if k % 2 == 0 else None) for k, (kinds, maps) in enumerate(calls_of(shape))]
    return [(kinds, px, None) for kinds, px in C.picture_calls_of(shape)]


_cache = {}


def encoded(shape, channels, codes):
    """Every call of a shape, encoded once and shared by the tests below: [(kinds, pixels, palette, files, offsets)]."""
    key = (shape, channels, codes)
    if key not in _cache:
        _cache[key] = [(kinds, px, pal) + encode_px(px, pal, codes) for kinds, px, pal in calls(shape, channels)]
    return _cache[key]


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp('png_dyn_host')
    return C.compile_host(d), d


@pytest.mark.parametrize('codes', C.CODES)
@pytest.mark.parametrize('channels', [1, 3])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_round_trip_byte_for_byte(lib, shape, channels, codes):
    T, H, W = shape
    cap = io.png_capacity(H, W, channels)
    seen = set()
    for kinds, px, pal, files, offs in encoded(shape, channels, codes):
        for t in range(T):
            C.check_file(files[t], px[t], pal)
            assert 0 < len(files[t]) <= cap
            seen.add(kinds[t])
        again, offs2 = encode_px(px, pal, codes)
        assert offs2 == offs and again == files
    assert len(seen) == (6 if channels == 1 else 4)


@pytest.mark.parametrize('codes', C.CODES)
def test_widest_row(lib, codes):
    """3 W + 1 = 65533: one scanline per segment, the tables of the dynamic form behind 65536 bytes of LDS."""
    H, W = 2, 21844
    px = np.stack([C.make_picture('gradient', 1, W, 1)[0], C.make_picture('noise256', 1, W, 2)[0]])[None]
    assert px.shape == (1, H, W, 3)
    (f,), _ = encode_px(px, None, codes)
    C.check_file(f, px[0])
    print('widest row, %s: %d bytes of %d' % (codes, len(f), px.size))
    if codes == 'dynamic':
        assert len(f) < 0.85 * px.size                 # the gradient row is coded: stored, the file is 131 154 bytes


@pytest.mark.parametrize('shape', SHAPES[:3], ids=lambda s: '%dx%dx%d' % s)
def test_device_files_equal_the_host_program_s(lib, host, shape):
    exe, d = host
    for channels in (1, 3):
        for codes in C.CODES:
            for kinds, px, pal, files, _offs in encoded(shape, channels, codes):
                assert C.run_host(exe, d, px, codes, pal) == files, (shape, channels, codes, kinds)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_one_channel_fixed_equals_the_first_entry_point(lib, shape):
    for kinds, maps, pal, files, offs in encoded(shape, 1, 'fixed'):
        blob, offsets = ops.png_encode_u8(torch.from_numpy(maps).cuda(), pal)
        assert offsets.cpu().tolist() == offs
        assert blob[:offs[-1]].cpu().numpy().tobytes() == b''.join(files), (shape, kinds)


@pytest.mark.parametrize('channels', [1, 3])
def test_dynamic_is_never_larger(lib, channels):
    for shape in SHAPES:
        for (kinds, _px, _pal, fixed, _o), (_k, _p, _q, dynamic, _o2) in zip(encoded(shape, channels, 'fixed'),
                                                                           encoded(shape, channels, 'dynamic')):
            for t in range(shape[0]):
                assert len(dynamic[t]) <= len(fixed[t]), (shape, channels, kinds[t])
    (fixed,), _ = encode_px(np.full((1, 70, 854), 7, np.uint8), None, 'fixed')
    (dynamic,), _ = encode_px(np.full((1, 70, 854), 7, np.uint8), None, 'dynamic')
    assert len(dynamic) < len(fixed)


def test_size_against_zlib(lib):
    H, W = 480, 854
    m = make_map('blobs', H, W, seed=0)
    (f,), _ = encode_px(m[None], np.asarray(io.default_palette(), np.uint8), 'dynamic')
    sizes = C.check_file(f, m, io.default_palette())
    z = len(zlib.compress(b''.join(b'\0' + m[y].tobytes() for y in range(H)), 6))
    print('blobs 480x854: IDAT %d bytes, zlib level 6 %d bytes, ratio %.4f' % (sizes['idat'], z, sizes['idat'] / z))
    assert sizes['idat'] <= 1.05 * C.BLOBS_IDAT_OVER_ZLIB6 * z


def test_capture_and_replay_on_new_contents(lib):
    T, H, W = 2, 33, 300
    pal = np.asarray(io.default_palette(), np.uint8)
    for channels in (1, 3):
        if channels == 1:
            a = np.stack([make_map('blobs', H, W, 1), make_map('ladder', H, W)])
            b = np.stack([make_map('noise256', H, W, 2), make_map('labels3', H, W, 3)])
        else:
            a = np.stack([C.make_picture('blend', H, W, 1), C.make_picture('constant', H, W)])
            b = np.stack([C.make_picture('noise256', H, W, 2), C.make_picture('gradient', H, W, 3)])
        palette = pal if channels == 1 else None
        static = torch.from_numpy(a).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.png_encode_u8(static, palette, codes='dynamic')
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, **ops.graph_capture_kwargs()):
            blob, offsets = ops.png_encode_u8(static, palette, codes='dynamic')
        for px in (a, b):
            static.copy_(torch.from_numpy(px).cuda())
            g.replay()
            torch.cuda.synchronize()
            offs = offsets.cpu().tolist()
            host = blob.cpu().numpy()
            eager, eoffs = encode_px(px, palette, 'dynamic')
            assert offs == eoffs
            for t in range(T):
                assert host[offs[t]:offs[t + 1]].tobytes() == eager[t]
                C.check_file(eager[t], px[t], palette)


def _read_dir(d):
    out = {}
    for name in sorted(os.listdir(d)):
        img = Image.open(os.path.join(d, name))
        img.load()
        out[name] = (img.mode, np.asarray(img).copy(), img.getpalette())
    return out


def test_writer_device_files_decode_to_the_host_files(lib, tmp_path):
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
    y, x = np.mgrid[0:H, 0:W]
    frames = np.stack([np.stack([(7 * x + 3 * t) % 256, (9 * y + t) % 256, (x + y) * 5 % 256], -1) for t in range(n + 1)]).astype(np.uint8)
    counts, dirs = {}, {}
    for mode, kw in (('host', dict(encode='host')), ('device', dict(encode='device', codes='dynamic', overlay_encode='device'))):
        w = io.IndexMapWriter(str(tmp_path / mode), **kw)
        w.save_first('seq', first, id_table=id_table, name=names[0])
        w.submit('seq', preds, first_index=2, id_table=id_table, names=names, keep=keep)
        w.save_first('all', first, overlay_frame_u8=frames[0])
        w.submit('all', preds, first_index=1, keep={1, 2, 4}, overlay_frames_u8=frames)
        w.submit('every', preds)
        counts[mode] = w.close()
        dirs[mode] = {s: _read_dir(str(tmp_path / mode / s)) for s in ('seq', 'all', 'every', os.path.join('overlay', 'all'))}
    assert counts['device'] == counts['host'] == 3 + 3 + n
    assert sorted(dirs['host'][os.path.join('overlay', 'all')]) == ['%05d.png' % t for t in range(n + 1)]
    for s in dirs['host']:
        assert sorted(dirs['device'][s]) == sorted(dirs['host'][s])
        for name, (mode, arr, pal) in dirs['host'][s].items():
            dmode, darr, dpal = dirs['device'][s][name]
            assert dmode == mode == ('RGB' if 'overlay' in s else 'P') and np.array_equal(darr, arr) and dpal == pal, (s, name)
    # the device's overlay files are the encoder's own truecolour files: the strict reader takes them too
    with open(str(tmp_path / 'device' / 'overlay' / 'all' / '00002.png'), 'rb') as f:
        got = png_ref_px.parse_png(f.read())[0]
    assert got.shape == (H, W, 3) and np.array_equal(got, dirs['host'][os.path.join('overlay', 'all')]['00002.png'][1])
