"""GPU: PNG files decoded on the device (swem_png_decode_u8, csrc/png_decode.hip, csrc/inflate_core.h).
Equality of bytes throughout: with the host program (tests/png_decode_host.cpp), with the strict readers, with PIL, and with
what went into the project's own encoder.  Pixels, workspace, sizes, status and palettes each lie between 64 guard bytes of
0xA5, checked after every call.  The mutation sweep stays on the CPU (tests/test_png_decode_host.py); the malformed files run
here are the named ones, each of which has passed the sanitizer build there."""
import io as pyio

import numpy as np
import pytest
import torch
from PIL import Image

from swem_amd import _lib, io, metrics, ops
from tests import png_decode_cases as D
from tests import png_dyn_cases as C
from tests.test_gpu_png import SHAPES, calls_of, make_map

pytestmark = pytest.mark.gpu

GUARD = 64


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    return buf, buf[GUARD:GUARD + nbytes]


def decode(files, slot_hw, channels, offsets=None):
    """swem_png_decode_u8 itself with every output and the workspace between guard bytes -> the dict tests/png_decode_cases.py's
    run_host gives."""
    T, (Hs, Ws) = len(files), slot_hw
    offs = np.cumsum([0] + [len(f) for f in files]).astype(np.int64) if offsets is None else np.asarray(offsets, np.int64)
    blob = torch.from_numpy(np.frombuffer(bytearray(b''.join(files)), np.uint8)).cuda()
    offsets_d = torch.from_numpy(offs).cuda()
    nbytes = _lib.query('swem_png_decode_workspace', T, Hs, Ws, channels, blob.numel())
    assert nbytes > 0
    sizes = {'pixels': T * Hs * Ws * channels, 'sizes': 8 * T, 'palettes': 768 * T, 'npal': 4 * T, 'status': 4 * T, 'ws': nbytes}
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    _lib.call('swem_png_decode_u8', ops._stream(), blob.data_ptr(), blob.numel(), offsets_d.data_ptr(), T, Hs, Ws, channels,
              bufs['pixels'][1].data_ptr(), bufs['sizes'][1].data_ptr(), bufs['palettes'][1].data_ptr(), bufs['npal'][1].data_ptr(),
              bufs['status'][1].data_ptr(), bufs['ws'][1].data_ptr(), nbytes)
    host = {k: b[0].cpu().numpy() for k, b in bufs.items()}
    for k, h in host.items():
        assert (h[:GUARD] == 0xA5).all() and (h[-GUARD:] == 0xA5).all(), 'the decoder wrote outside `%s`' % k
    body = {k: h[GUARD:-GUARD] for k, h in host.items()}
    return {'pixels': body['pixels'].reshape((T, Hs, Ws, 3) if channels == 3 else (T, Hs, Ws)),
            'sizes': body['sizes'].view('<i4').reshape(T, 2), 'palettes': body['palettes'].reshape(T, 768),
            'npal': body['npal'].view('<i4'), 'status': body['status'].view('<i4')}


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp('png_decode_host')
    return D.compile_host(d), d


def same(res, ref):
    for k in ref:
        assert np.array_equal(res[k], ref[k]), k


@pytest.mark.parametrize('part', range(4))
def test_good_files_equal_the_host_program_and_the_strict_readers(lib, host, part):
    exe, d = host
    calls = D.calls_of_cases(D.good_cases())
    for channels, slot, group in calls[part::4]:
        files = [c['data'] for c in group]
        res = decode(files, slot, channels)
        for t, c in enumerate(group):
            D.check_result(res, t, c, slot)
        same(res, D.run_host(exe, d, files, slot, channels))


def test_fifteen_bit_codes(lib, tmp_path):
    c = D.fibonacci_case(C.compile_host(tmp_path), tmp_path)
    D.check_result(decode([c['data']], c['want'].shape, 1), 0, c, c['want'].shape)


@pytest.mark.parametrize('codes', C.CODES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_device_to_device_round_trip(lib, shape, codes):
    """ops.png_encode_u8's blob and offsets go straight into ops.png_decode_u8 and give back the input."""
    T, H, W = shape
    pal = np.asarray(io.default_palette(), np.uint8)
    calls = [(maps, pal if k % 2 == 0 else None) for k, (_kinds, maps) in enumerate(calls_of(shape))]
    calls += [(px, None) for _kinds, px in C.picture_calls_of(shape)]
    for px, palette in calls:
        src = torch.from_numpy(px).cuda()
        blob, offsets = ops.png_encode_u8(src, palette, codes=codes)
        pixels, sizes, palettes, npal, status = ops.png_decode_u8(blob, offsets, (H, W), 3 if px.ndim == 4 else 1, want_palette=True)
        assert not status.any().item()
        assert torch.equal(pixels, src)
        assert sizes.cpu().tolist() == [[H, W]] * T
        assert npal.cpu().tolist() == [256 if palette is not None else 0] * T
        want = pal if palette is not None else np.zeros(768, np.uint8)
        assert all(np.array_equal(p, want) for p in palettes.cpu().numpy())


@pytest.mark.parametrize('optimize', [False, True])
def test_pil_files(lib, optimize):
    rng = np.random.RandomState(8)
    y, x = np.mgrid[0:33, 0:300]
    pictures = [('P', make_map('blobs', 33, 300, 1)), ('P', rng.randint(0, 200, (33, 300)).astype(np.uint8)),
                ('L', ((x * 3 + y * 7) % 256).astype(np.uint8)), ('L', make_map('noise256', 33, 300, 2)),
                ('RGB', C.make_picture('gradient', 33, 300, 1)), ('RGB', C.make_picture('blend', 33, 300, 2))]
    for mode, px in pictures:
        img = Image.fromarray(px, mode)
        if mode == 'P':
            img.putpalette(io.default_palette())
        buf = pyio.BytesIO()
        img.save(buf, 'PNG', optimize=optimize)
        back = Image.open(pyio.BytesIO(buf.getvalue()))
        back.load()
        pixels, sizes, palettes, npal, status = io.png_decode([buf.getvalue()], channels=3 if mode == 'RGB' else 1)
        assert tuple(pixels.shape[1:3]) == (33, 300) and sizes.cpu().tolist() == [[33, 300]]
        assert np.array_equal(pixels[0].cpu().numpy(), np.array(back)) and np.array_equal(np.array(back), px)
        if mode == 'P':
            pal = np.asarray(back.getpalette(), np.uint8)
            assert np.array_equal(palettes[0].cpu().numpy()[:pal.size], pal) and int(npal[0]) == pal.size // 3
            assert np.array_equal(io.read_palette(buf.getvalue())[:pal.size], pal)


def test_named_malformed_files(lib, host):
    from tests.test_png_decode_host import check_malformed, malformed_batches
    exe, d = host
    for channels, files, names in malformed_batches():
        res = decode(files, D.BAD_SLOT, channels)
        check_malformed(res, channels, files, names)
        same(res, D.run_host(exe, d, files, D.BAD_SLOT, channels))
        first_bad = next(t for t, (_n, s) in enumerate(names) if s != 'OK')
        with pytest.raises(io.PngDecodeError) as e:
            io.png_decode(files, slot_hw=D.BAD_SLOT, channels=channels)
        assert e.value.index == first_bad and e.value.name == names[first_bad][1]
        status = io.png_decode(files, slot_hw=D.BAD_SLOT, channels=channels, check=False)[4]
        assert status.cpu().tolist() == [D.ST[s] for _n, s in names]
    _m, g, p = D.base_files()
    n, k = len(g), len(p)
    res = decode([g, p, g], D.BAD_SLOT, 1, offsets=[0, n + k, n, n + k + n])
    assert list(res['status']) == [D.ST['TRAILING'], D.ST['OFFSETS'], D.ST['TRAILING']] and not res['pixels'].any()
    res = decode([g, p], D.BAD_SLOT, 1, offsets=[0, n, n + k + 1])
    assert list(res['status']) == [0, D.ST['OFFSETS']]


def test_capture_and_replay_on_new_files(lib):
    H, W = 33, 300
    pal = np.asarray(io.default_palette(), np.uint8)

    def files_of(maps):
        blob, offsets = ops.png_encode_u8(torch.from_numpy(maps).cuda(), pal, codes='dynamic')
        return blob, offsets
    a = np.stack([make_map('blobs', H, W, 1), make_map('ladder', H, W)])
    b = np.stack([make_map('noise256', H, W, 2), make_map('labels3', H, W, 3)])
    blob_a, offs_a = files_of(a)
    static_blob, static_offs = blob_a.clone(), offs_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.png_decode_u8(static_blob, static_offs, (H, W), 1, want_palette=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, **ops.graph_capture_kwargs()):
        out = ops.png_decode_u8(static_blob, static_offs, (H, W), 1, want_palette=True)
    for maps in (a, b):
        blob, offs = files_of(maps)
        static_blob.copy_(blob)
        static_offs.copy_(offs)
        g.replay()
        torch.cuda.synchronize()
        eager = ops.png_decode_u8(blob, offs, (H, W), 1, want_palette=True)
        for x, y in zip(out, eager):
            assert torch.equal(x, y)
        assert np.array_equal(out[0].cpu().numpy(), maps) and not out[4].any().item()


def test_annotations_from_files_to_the_meter_and_the_stager(lib):
    """T = 5 annotation files at 33x300 with two objects: JFMeter fed with io.png_decode(files) returns the table it returns when
    fed PIL-decoded arrays; davis_sequence_u8 with the device-decoded first label equals the one with the PIL-decoded label."""
    T, H, W = 5, 33, 300
    gt = np.stack([make_map('blobs', H, W, seed=t) for t in range(T)])
    assert set(np.unique(gt)) == {0, 1, 2}
    files = []
    for t in range(T):
        img = Image.fromarray(gt[t], 'P')
        img.putpalette(io.default_palette())
        buf = pyio.BytesIO()
        img.save(buf, 'PNG')
        files.append(buf.getvalue())
    pil = np.stack([np.array(Image.open(pyio.BytesIO(f))) for f in files])
    decoded = io.png_decode(files)[0]
    assert np.array_equal(decoded.cpu().numpy(), pil)
    rng = np.random.RandomState(1)
    preds = [torch.from_numpy(np.where(rng.rand(1, H, W) < 0.9, gt[t][None], 0).astype(np.int64)).cuda() for t in range(1, T)]
    tables = []
    for source in (decoded, pil):
        m = metrics.JFMeter()
        m.add('seq', source, preds, num_objects=2)
        tables.append(m.results())
    np.testing.assert_equal(tables[0], tables[1])        # (NaN equals NaN here: three scored frames leave some decays undefined)
    assert 0 < tables[0]['J&F-Mean'] < 1
    frames = rng.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    fa, ma, na = io.davis_sequence_u8(frames, decoded[0], size=(48, 64))
    fb, mb, nb = io.davis_sequence_u8(frames, pil[0], size=(48, 64))
    assert na == nb == 3 and torch.equal(fa, fb) and torch.equal(ma[0], mb[0])
