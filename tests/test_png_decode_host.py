"""CPU: the device PNG decoder's code (csrc/inflate_core.h) run as a loop over 64 lanes by tests/png_decode_host.cpp, against the
strict readers (tests/png_ref.py, tests/png_ref_px.py, tests/inflate_ref.py), zlib and PIL; the named malformed files and the
mutation sweep; the same under AddressSanitizer; the argument checks of swem_png_decode_u8.  Equality of bytes throughout."""
import re
import subprocess

import numpy as np
import pytest

from swem_amd import io
from tests import png_decode_cases as D
from tests import png_dyn_cases as C


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp('png_decode_host')
    return D.compile_host(d), d


@pytest.fixture(scope='module')
def dyn_host(tmp_path_factory):
    d = tmp_path_factory.mktemp('png_dyn_host')
    return C.compile_host(d), d


def test_status_names_are_the_header_s():
    import os
    src = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'swem_hip_io.h')).read()
    defs = {n: int(v) for n, v in re.findall(r'^#define\s+SWEM_PNG_ST_(\w+)\s+(\d+)', src, flags=re.M)}
    assert defs == D.ST and len(defs) == 35 and defs['OK'] == 0
    assert list(io.PNG_STATUS) == sorted(defs, key=defs.get)
    core = open(os.path.join(os.path.dirname(__file__), '..', 'swem_amd', 'csrc', 'inflate_core.h')).read()
    assert {n: int(v) for n, v in re.findall(r'^\s*PNGD_([A-Z_0-9]+) = (\d+),?$', core, flags=re.M)} == defs


def test_good_files(host):
    """(1) every case of the issue's table, depths, filters, container variants and shapes; slots that fit and slots that do not."""
    exe, d = host
    cases = D.good_cases()
    names = {c['name'] for c in cases}
    assert {'level6', 'fixed', 'huffman_only', 'rle', 'level0', 'noise', 'window512', 'sync_flush', 'far_match', 'distance32768',
            'one_byte_idats', 'empty_idats', 'ancillary', 'depth1_w9', 'depth2_w5', 'depth4_w3', 'filter_bpp3_turn3'} <= names
    seen = 0
    for channels, slot, group in D.calls_of_cases(cases):
        res = D.run_host(exe, d, [c['data'] for c in group], slot, channels)
        for t, c in enumerate(group):
            D.check_result(res, t, c, slot)
        sizes = {c['want'].shape[:2] for c in group}
        seen += len(group)
        if slot == (40, 900):
            assert len(sizes) > 10                           # many sizes in one call, all smaller than the slot
    assert seen > len(cases)


def test_fifteen_bit_codes(host, dyn_host):
    exe, d = host
    c = D.fibonacci_case(*dyn_host)
    D.check_result(D.run_host(exe, d, [c['data']], c['want'].shape, 1), 0, c, c['want'].shape)


def test_the_encoder_s_files_decode_to_what_went_in(host, dyn_host):
    """(2) every file of tests/test_png_dyn_host.py's files_of: both code modes, index maps and pictures; (3) png_lanes_host's."""
    from tests.test_png_dyn_host import files_of
    from tests.test_gpu_png import SHAPES
    exe, d = host
    for shape in SHAPES:
        T, H, W = shape
        for kinds, px, pal, by_codes in files_of(dyn_host, shape):
            channels = 3 if px.ndim == 4 else 1
            for codes in C.CODES:
                res = D.run_host(exe, d, by_codes[codes], (H, W), channels)
                for t in range(T):
                    c = {'name': '%s %s %s' % (shape, kinds[t], codes), 'want': px[t],
                         'palette': None if pal is None else np.asarray(pal, np.uint8).reshape(256, 3)}
                    D.check_result(res, t, c, (H, W))
    old = C.compile_host(d, 'png_lanes_host')
    m = np.stack([D.make_map('ladder', 33, 300), D.make_map('blobs', 33, 300, 4)])
    m.tofile(str(d / 'maps.raw'))
    subprocess.run([old, str(d / 'maps.raw'), '2', '33', '300', '-', str(d / 'old')], check=True, timeout=300)
    files = [open(str(d / ('old.%d.png' % t)), 'rb').read() for t in range(2)]
    res = D.run_host(exe, d, files, (33, 300), 1)
    for t in range(2):
        D.check_result(res, t, {'name': 'lanes %d' % t, 'want': m[t], 'palette': None}, (33, 300))


def malformed_batches():
    """[(channels, files, [(name, status)])]: a good file before, between and after the malformed ones."""
    _m, g, p = D.base_files()
    rgb = D.case('rgb', D.R.png_file(3, 2, 8, 2, D.deflate(b'\1' + bytes(range(9)) + b'\2' + bytes(range(9)))))
    out = []
    for channels, good in ((1, [g, p]), (3, [rgb['data']])):
        files, names = [], []
        for k, (name, data, status, ch) in enumerate([b for b in D.malformed_cases() if b[3] == channels]):
            files += [good[k % len(good)], data]
            names += [('good', 'OK'), (name, status)]
        out.append((channels, files + [good[0]], names + [('good', 'OK')]))
    return out


def check_malformed(res, channels, files, names):
    for t, (name, status) in enumerate(names):
        assert int(res['status'][t]) == D.ST[status], (name, io.PNG_STATUS[int(res['status'][t])], status)
        if status != 'OK':
            assert not res['pixels'][t].any() and tuple(res['sizes'][t]) == (0, 0) and not res['palettes'][t].any(), name
            assert int(res['npal'][t]) == 0, name
        else:
            D.check_result(res, t, D.case('good', files[t]), D.BAD_SLOT)


def test_named_malformed_files(host):
    """(4) one file per entry of the refusal list: exactly that status, a zero slot, the neighbours untouched."""
    exe, d = host
    listed = set()
    for channels, files, names in malformed_batches():
        for (name, status), data in zip(names, files):
            if status not in ('OK', 'TOO_LARGE') and name not in ('truecolour_in_one_channel', 'gray_in_three_channels'):
                assert D.strict_accepts(data) is None, name          # the strict reader refuses it too
            listed.add(status)
        check_malformed(D.run_host(exe, d, files, D.BAD_SLOT, channels), channels, files, names)
    assert listed == set(D.ST) - {'OFFSETS'}


def test_offsets_are_checked(host):
    exe, d = host
    _m, g, p = D.base_files()
    n, k = len(g), len(p)
    res = D.run_host(exe, d, [g, p, g], D.BAD_SLOT, 1, offsets=[0, n + k, n, n + k + n])      # file 1 runs backwards
    # (files 0 and 2 are then two files back to back: bytes after IEND)
    assert list(res['status']) == [D.ST['TRAILING'], D.ST['OFFSETS'], D.ST['TRAILING']] and not res['pixels'].any()
    res = D.run_host(exe, d, [g, p], D.BAD_SLOT, 1, offsets=[0, n, n + k + 1])                 # past the blob
    assert list(res['status']) == [0, D.ST['OFFSETS']]
    res = D.run_host(exe, d, [g, p], D.BAD_SLOT, 1, offsets=[-1, n, n + k])
    assert list(res['status']) == [D.ST['OFFSETS'], 0]


_sweep = {}


def sweep(host):
    """The mutation sweep through the plain build, once: [(name, files, result)]."""
    if not _sweep:
        exe, d = host
        _sweep['runs'] = []
        for name, data, _m in D.sweep_bases():
            files = D.sweep_files(data)
            _sweep['runs'].append((name, files, D.run_host(exe, d, files, (12, 40), 1, tag='sweep_' + name)))
    return _sweep['runs']


def test_mutation_sweep(host):
    """(5) every single-byte change at three values and every truncation, of the file and of its zlib stream: refused exactly
    where the strict reader refuses, equal pixels where it accepts."""
    for name, files, res in sweep(host):
        accepted, refused = D.check_sweep(res, files, (12, 40))
        print('%s: %d files, %d accepted, %d refused' % (name, len(files), accepted, refused))
        assert refused > len(files) // 2


def test_sanitizer_build(host, tmp_path):
    """(6) the same program under AddressSanitizer and UndefinedBehaviorSanitizer: the two smallest shapes, every named malformed
    file and the whole sweep, with the plain build's outputs."""
    plain, d = host
    exe = D.compile_host(tmp_path, extra=('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'))

    def same(files, slot, channels, want=None):
        a = D.run_host(exe, tmp_path, files, slot, channels)
        b = D.run_host(plain, tmp_path, files, slot, channels, tag='plain') if want is None else want
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    for channels, slot, group in D.calls_of_cases(D.good_cases()):
        if slot in ((1, 1), (3, 5)) or group[0]['name'].startswith('depth'):
            same([c['data'] for c in group], slot, channels)
    for channels, files, _names in malformed_batches():
        same(files, D.BAD_SLOT, channels)
    for _name, files, res in sweep(host):
        same(files, (12, 40), 1, want=res)


def test_decode_checks_its_arguments_before_any_hip_call(lib):
    T, Hs, Ws, n = 2, 33, 300, 5000
    p = 0x10000          # never dereferenced: every call below is refused first

    def call(blob=p, blob_bytes=n, offsets=p, T=T, Hs=Hs, Ws=Ws, channels=1, pixels=p, sizes=p, palettes=p, npal=p, status=p,
             ws_ptr=p, ws_bytes=None):
        ws = lib.swem_png_decode_workspace(T, Hs, Ws, channels, blob_bytes)
        return lib.swem_png_decode_u8(None, blob, blob_bytes, offsets, T, Hs, Ws, channels, pixels, sizes, palettes, npal, status,
                                      ws_ptr, ws if ws_bytes is None else ws_bytes)
    assert call(blob=None) == -4 and b'null pointer' in lib.swem_last_error()
    assert call(offsets=None) == -4 and call(pixels=None) == -4 and call(sizes=None) == -4 and call(status=None) == -4
    assert call(ws_ptr=None) == -4
    assert call(ws_ptr=p + 8) == -4 and b'aligned' in lib.swem_last_error()
    assert call(offsets=p + 4) == -4 and call(status=p + 2) == -4
    assert call(channels=2) == -4 and b'channels' in lib.swem_last_error()
    assert call(channels=0) == -4 and call(channels=4) == -4
    assert call(T=0) == -1 and call(T=65536) == -1 and call(Hs=0) == -1 and call(Ws=0) == -1
    assert call(Ws=65535) == -1 and b'65535' in lib.swem_last_error()
    assert call(channels=3, Ws=21845) == -1                  # 3 * 21845 + 1 = 65536
    assert call(Hs=40000, Ws=60000) == -1                    # a slot of 2 GiB and more
    assert call(blob_bytes=0) == -1
    ws = lib.swem_png_decode_workspace(T, Hs, Ws, 1, n)
    assert call(ws_bytes=ws - 1) == -2 and b'insufficient workspace' in lib.swem_last_error()
    assert call(channels=3, ws_bytes=ws) == -2


def test_workspace_is_monotone_and_zero_for_refused_shapes(lib):
    q = lib.swem_png_decode_workspace
    base = q(2, 33, 300, 1, 5000)
    assert base >= 5000 + 2 * 33 * 301
    assert q(3, 33, 300, 1, 5000) > base and q(2, 34, 300, 1, 5000) > base and q(2, 33, 301, 1, 5000) > base
    assert q(2, 33, 300, 3, 5000) > base and q(2, 33, 300, 1, 5017) > base
    assert q(1, 1, 1, 1, 1) > 0 and q(65535, 1, 1, 1, 1) > 0
    for bad in ((0, 33, 300, 1, 5000), (65536, 33, 300, 1, 5000), (2, 0, 300, 1, 5000), (2, 33, 0, 1, 5000), (2, 33, 300, 2, 5000),
                (2, 33, 65535, 1, 5000), (2, 33, 21845, 3, 5000), (2, 40000, 60000, 1, 5000), (2, 33, 300, 1, 0)):
        assert q(*bad) == 0, bad


def test_png_decode_refuses_before_it_needs_a_device():
    with pytest.raises(ValueError, match='empty'):
        io.png_decode([])
    with pytest.raises(ValueError, match='channels'):
        io.png_decode([b'x'], channels=2)
    e = io.PngDecodeError(3, D.ST['ADLER'])
    assert (e.index, e.status, e.name) == (3, 32, 'ADLER') and 'file 3' in str(e) and 'ADLER' in str(e)
