"""CPU: the host side of the device PNG encoder (include/swem_hip_io.h, csrc/png.hip, swem_amd/io.py).
  * tests/png_ref.py (the yardstick of tests/test_gpu_png.py) against PIL on files PIL wrote, and its strictness;
  * the capacity formula;
  * swem_png_encode_u8 refuses null pointers, bad shapes and short buffers before any HIP call;
  * the writer's `encode` switch."""
import io as pyio
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from swem_amd import io
from tests import png_ref


def pil_png(arr, palette, **kw):
    img = Image.fromarray(arr)
    if palette is not None:
        img.putpalette(palette)
    buf = pyio.BytesIO()
    img.save(buf, format='PNG', **kw)
    return buf.getvalue()


def some_map(H, W, seed):
    rng = np.random.RandomState(seed)
    m = rng.randint(0, 4, (H, W)).astype(np.uint8)
    m[H // 3:H // 3 + max(H // 2, 1), W // 4:W // 4 + max(W // 2, 1)] = 200     # runs, and an index past 143
    return m


@pytest.mark.parametrize('H,W', [(1, 1), (3, 5), (17, 259), (33, 300), (70, 854)])
def test_parse_png_agrees_with_pil(H, W):
    pal = io.default_palette()
    arr = some_map(H, W, H * 1000 + W)
    for palette in (pal, None):
        data = pil_png(arr, palette)
        got, got_pal, n_idat, sizes = png_ref.parse_png(data)
        assert np.array_equal(got, arr)
        assert n_idat >= 1 and sizes['file'] == len(data) and sizes['raw'] == H * (W + 1)
        if palette is None:
            assert got_pal is None
        else:
            assert np.array_equal(got_pal, np.asarray(pal, np.uint8).reshape(-1, 3)[:len(got_pal)]) and len(got_pal) > 200
        back = Image.open(pyio.BytesIO(data))
        assert np.array_equal(np.asarray(back), got)


def test_unfilter_undoes_every_filter_type():
    """Five scanlines, one per filter type, filtered here by the definitions of the PNG specification, section 9.2."""
    rng = np.random.RandomState(2)
    H, W = 5, 37
    arr = rng.randint(0, 256, (H, W)).astype(np.int64)
    raw = bytearray()
    for y in range(H):
        raw.append(y)
        for x in range(W):
            a = arr[y, x - 1] if x else 0
            b = arr[y - 1, x] if y else 0
            c = arr[y - 1, x - 1] if x and y else 0
            pred = [0, a, b, (a + b) // 2, png_ref._paeth(a, b, c)][y]
            raw.append(int(arr[y, x] - pred) & 255)
    assert np.array_equal(png_ref.unfilter(bytes(raw), H, W), arr.astype(np.uint8))
    body = zlib.compress(bytes(raw))

    def chunk(t, b):
        return struct.pack('>I', len(b)) + t + b + struct.pack('>I', zlib.crc32(t + b) & 0xffffffff)
    data = png_ref.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 0, 0, 0, 0)) + chunk(b'IDAT', body[:9]) + \
        chunk(b'IDAT', body[9:]) + chunk(b'IEND', b'')
    got, pal, n_idat, _ = png_ref.parse_png(data)
    assert np.array_equal(got, arr.astype(np.uint8)) and pal is None and n_idat == 2
    assert np.array_equal(np.asarray(Image.open(pyio.BytesIO(data))), got)


def test_parse_png_rejects_one_flipped_byte():
    arr = some_map(12, 40, 1)
    data = pil_png(arr, io.default_palette())
    assert np.array_equal(png_ref.parse_png(data)[0], arr)
    cs = png_ref.chunks(data)
    assert [c[0] for c in cs][0] == b'IHDR'
    idat_at = data.index(b'IDAT') - 4
    idat_len, = struct.unpack('>I', data[idat_at:idat_at + 4])

    def flipped(pos):
        b = bytearray(data)
        b[pos] ^= 0x01
        return bytes(b)

    def refix_crc(b, at):
        """the chunk at `at` with its CRC made right again: the damage is then in the payload alone"""
        n, = struct.unpack('>I', b[at:at + 4])
        return b[:at + 8 + n] + struct.pack('>I', zlib.crc32(b[at + 4:at + 8 + n]) & 0xffffffff) + b[at + 12 + n:]

    with pytest.raises(png_ref.PngError, match='CRC'):
        png_ref.parse_png(flipped(8 + 8 + 13))                    # the first byte of IHDR's CRC
    with pytest.raises(png_ref.PngError, match='CRC'):
        png_ref.parse_png(flipped(8 + 8 + 8))                     # IHDR: the bit depth, CRC left as it was
    with pytest.raises(png_ref.PngError, match='IHDR'):
        png_ref.parse_png(refix_crc(flipped(8 + 8 + 8), 8))       # IHDR: the bit depth, with a CRC that fits it
    adler_pos = idat_at + 8 + idat_len - 1                        # the last byte of the zlib stream (one IDAT: checked below)
    assert [c[0] for c in cs].count(b'IDAT') == 1
    with pytest.raises(png_ref.PngError, match='CRC'):
        png_ref.parse_png(flipped(adler_pos))
    with pytest.raises(png_ref.PngError, match='inflate'):
        png_ref.parse_png(refix_crc(flipped(adler_pos), idat_at))
    with pytest.raises(png_ref.PngError, match='after IEND'):
        png_ref.parse_png(data + b'\0')


def capacity_formula(H, W):
    """include/swem_hip_io.h: all segments stored, plus the headers."""
    rows = min(16, 65535 // (W + 1))
    nseg = -(-H // rows)
    return 8 + 25 + 780 + 2 + H * (W + 1) + 17 * nseg + 21 + 12


def test_capacity_is_the_documented_formula(lib):
    for H, W in [(1, 1), (3, 5), (17, 259), (33, 300), (480, 854), (720, 1280), (40, 5000), (2, 65534), (16, 4095), (17, 4095)]:
        assert io.png_capacity(H, W) == capacity_formula(H, W), (H, W)
    assert io.png_capacity(480, 854) == 8 + 25 + 780 + 2 + 480 * 855 + 17 * 30 + 33 == 411758
    assert io.png_capacity(0, 5) == 0 and io.png_capacity(5, 0) == 0 and io.png_capacity(5, 65535) == 0
    assert lib.swem_png_workspace(2, 33, 300) >= 2 * 3 * (16 * 301 + 5)
    assert lib.swem_png_workspace(0, 33, 300) == 0


def test_encode_checks_its_arguments_before_any_hip_call(lib):
    T, H, W = 2, 33, 300
    cap, ws = lib.swem_png_capacity(H, W), lib.swem_png_workspace(T, H, W)
    p = 0x10000          # never dereferenced: every call below is refused first

    def call(maps=p, pal=None, blob=p, blob_bytes=T * cap, offsets=p, T=T, H=H, W=W, ws_ptr=p, ws_bytes=ws):
        return lib.swem_png_encode_u8(None, maps, pal, blob, blob_bytes, offsets, T, H, W, ws_ptr, ws_bytes)
    assert call(maps=None) == -4 and b'null pointer' in lib.swem_last_error()
    assert call(blob=None) == -4 and call(offsets=None) == -4 and call(ws_ptr=None) == -4
    assert call(ws_ptr=p + 4) == -4 and b'aligned' in lib.swem_last_error()
    assert call(H=0) == -1 and b'65535' in lib.swem_last_error()
    assert call(W=0) == -1 and call(W=65535) == -1 and call(T=0) == -1 and call(T=65536) == -1
    assert call(blob_bytes=T * cap - 1) == -2 and b'insufficient workspace' in lib.swem_last_error()
    assert call(ws_bytes=ws - 1) == -2 and b'insufficient workspace' in lib.swem_last_error()


def test_lane_code_round_trips_on_the_host(tmp_path):
    """csrc/png_core.h -- token codes, bit writer, CRC combine, Adler sums: everything of the encoder but the wavefront joins --
    compiled as plain C++ (tests/png_lanes_host.cpp) on the contents and shapes of tests/test_gpu_png.py, and one row of 65534."""
    import os
    import subprocess
    from swem_amd import build
    from tests.test_gpu_png import SHAPES, calls_of, make_map
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / 'png_lanes_host')
    subprocess.run([build.HIPCC, '-x', 'c++', '-std=c++17', '-O1', '-I', build.CSRC, os.path.join(here, 'png_lanes_host.cpp'),
                    '-o', exe], check=True, capture_output=True, timeout=300)
    pal = np.asarray(io.default_palette(), np.uint8)
    pal.tofile(str(tmp_path / 'pal.raw'))

    def run(maps, palette):
        T, H, W = maps.shape
        maps.tofile(str(tmp_path / 'maps.raw'))
        subprocess.run([exe, str(tmp_path / 'maps.raw'), str(T), str(H), str(W), str(tmp_path / 'pal.raw') if palette else '-',
                        str(tmp_path / 'out')], check=True, timeout=300)
        files = []
        for t in range(T):
            with open(str(tmp_path / ('out.%d.png' % t)), 'rb') as f:
                files.append(f.read())
            got, got_pal, n_idat, sizes = png_ref.parse_png(files[-1])
            assert np.array_equal(got, maps[t]) and n_idat >= 2 and len(files[-1]) <= capacity_formula(H, W)
            assert (np.array_equal(got_pal, pal.reshape(256, 3)) if palette else got_pal is None)
            assert np.array_equal(np.asarray(Image.open(pyio.BytesIO(files[-1]))), maps[t])
        return files

    for shape in SHAPES:
        for k, (_kinds, maps) in enumerate(calls_of(shape)):
            run(maps, palette=k % 2 == 0)
    run(np.stack([make_map('ladder', 2, 65534), make_map('noise256', 2, 65534, 1)]), True)
    (const,) = run(np.full((1, 480, 854), 255, np.uint8), True)
    assert len(const) <= 480 * 855 // 50


def test_writer_refuses_an_unknown_encoder(tmp_path):
    with pytest.raises(ValueError, match='nonsense'):
        io.IndexMapWriter(str(tmp_path), encode='nonsense')
