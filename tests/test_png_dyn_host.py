"""CPU: the second form of the device PNG encoder (csrc/png_core.h: dynamic Huffman tables, truecolour filters) run as a loop over
64 lanes by tests/png_dyn_host.cpp, read back by the strict reader tests/png_ref_px.py and by PIL; the length builder against a
plain heap Huffman; the argument checks of swem_png_encode_px_u8; the writer's new switches.  No tolerance anywhere."""
from fractions import Fraction

import numpy as np
import pytest

from swem_amd import io
from tests import png_dyn_cases as C
from tests.test_gpu_png import SHAPES, calls_of, make_map

H_BIG, W_BIG = 480, 854


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp('png_dyn_host')
    return C.compile_host(d), d


def capacity_formula(H, W, channels):
    """include/swem_hip_io.h: all segments stored, plus the headers; no PLTE for 3 channels."""
    rw = channels * W + 1
    rows = min(16, 65535 // rw)
    nseg = -(-H // rows)
    return 8 + 25 + (780 if channels == 1 else 0) + 2 + H * rw + 17 * nseg + 21 + 12


def all_calls(shape):
    """[(kinds, pixels, palette)]: the index-map calls of tests/test_gpu_png.py (with and without a palette in turn) and the
    truecolour calls of a shape."""
    pal = np.asarray(io.default_palette(), np.uint8)
    return [(kinds, maps, pal if k % 2 == 0 else None) for k, (kinds, maps) in enumerate(calls_of(shape))] + \
        [(kinds, px, None) for kinds, px in C.picture_calls_of(shape)]


_files = {}


def files_of(host, shape):
    """Every call of a shape through the host program in both modes, once: [(kinds, pixels, palette, {codes: files})]."""
    if shape not in _files:
        exe, d = host
        _files[shape] = [(kinds, px, pal, {c: C.run_host(exe, d, px, c, pal) for c in C.CODES}) for kinds, px, pal in all_calls(shape)]
    return _files[shape]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_round_trip_and_sizes(host, shape):
    """(1) every file decodes to what went in; (5) dynamic <= fixed <= capacity, noise is the stored form in both modes."""
    T, H, W = shape
    seen = set()
    for kinds, px, pal, by_codes in files_of(host, shape):
        channels = 3 if px.ndim == 4 else 1
        cap = capacity_formula(H, W, channels)
        for t in range(T):
            for codes in C.CODES:
                C.check_file(by_codes[codes][t], px[t], pal)
            fixed, dynamic = len(by_codes['fixed'][t]), len(by_codes['dynamic'][t])
            assert dynamic <= fixed <= cap, (kinds[t], shape, dynamic, fixed, cap)
            if kinds[t] == 'noise256':
                # every segment stored: the capacity less the PLTE a grayscale file does not carry
                assert dynamic == fixed == cap - (780 if channels == 1 and pal is None else 0), (shape, channels)
            seen.add((channels, kinds[t]))
    assert len(seen) == 6 + 4


def test_constant_map_dynamic_is_smaller(host):
    exe, d = host
    m = np.full((1, H_BIG, W_BIG), 255, np.uint8)
    (fixed,), (dynamic,) = C.run_host(exe, d, m, 'fixed'), C.run_host(exe, d, m, 'dynamic')
    C.check_file(dynamic, m[0])
    print('constant 480x854: fixed %d, dynamic %d bytes' % (len(fixed), len(dynamic)))
    assert len(dynamic) < len(fixed) <= H_BIG * (W_BIG + 1) // 50


def test_one_channel_fixed_files_are_the_first_encoder_s(host, tmp_path):
    """(6) tests/png_lanes_host.cpp, the host form of png_encode_kernel, writes the same bytes."""
    import subprocess
    old = C.compile_host(tmp_path, 'png_lanes_host')
    pal = np.asarray(io.default_palette(), np.uint8)
    pal.tofile(str(tmp_path / 'pal.raw'))
    for shape in SHAPES:
        T, H, W = shape
        for kinds, px, palette, by_codes in files_of(host, shape):
            if px.ndim == 4:
                continue
            px.tofile(str(tmp_path / 'maps.raw'))
            subprocess.run([old, str(tmp_path / 'maps.raw'), str(T), str(H), str(W),
                            str(tmp_path / 'pal.raw') if palette is not None else '-', str(tmp_path / 'old')], check=True, timeout=300)
            for t in range(T):
                with open(str(tmp_path / ('old.%d.png' % t)), 'rb') as f:
                    assert f.read() == by_codes['fixed'][t], (shape, kinds[t])


def histograms():
    """[(name, freq, maxbits)]: random, all-equal, two-symbol, one-dominant, Fibonacci."""
    rng = np.random.RandomState(11)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    out = []
    for k in range(6):
        f = rng.randint(0, [4, 50, 3000][k % 3], 286)
        f[256] = 1
        out.append(('random286_%d' % k, f, 15))
        g = rng.randint(0, [3, 40, 287][k % 3], 19)
        g[rng.randint(0, 19)] += 1
        out.append(('random19_%d' % k, g, 7))
    f = rng.randint(0, 2, 286) * rng.randint(1, 60000, 286)           # few thousand tokens per symbol, many unused
    f[256] = 1
    out.append(('random286_wide', f, 15))
    out += [('equal286', np.full(286, 7), 15), ('equal19', np.full(19, 3), 7), ('equal5', np.full(5, 1), 15),
            ('equal128_7', np.full(128, 2), 7)]
    two = np.zeros(286, np.int64)
    two[[65, 256]] = [900, 1]
    out.append(('two_symbols', two, 15))
    two19 = np.zeros(19, np.int64)
    two19[[1, 18]] = [2, 5]
    out.append(('two_symbols19', two19, 7))
    dom = rng.randint(1, 4, 286)
    dom[0] = 60000
    out.append(('one_dominant', dom, 15))
    dom19 = rng.randint(1, 3, 19)
    dom19[0] = 280
    out.append(('one_dominant19', dom19, 7))
    one = np.zeros(19, np.int64)
    one[8] = 5
    out.append(('one_symbol19', one, 7))
    out.append(('fibonacci19', np.array(fib[:19]), 7))
    out.append(('fibonacci30', np.array(fib[:30]), 15))
    out.append(('fibonacci30_reversed', np.array(fib[:30][::-1]), 15))
    return out


@pytest.mark.parametrize('name,freq,maxbits', histograms(), ids=[h[0] for h in histograms()])
def test_length_builder(host, name, freq, maxbits):
    """(2) Kraft sum exactly 1, no length past maxbits, length 0 exactly where the frequency is 0, a more frequent symbol never
    has the longer code; (3) whenever a plain heap Huffman stays within maxbits, the builder's cost is its cost (the optimum is
    unique as a cost), and it is never below it."""
    exe, _d = host
    freq = [int(f) for f in freq]
    lens = C.run_lengths(exe, freq, maxbits)
    used = [i for i, f in enumerate(freq) if f > 0]
    assert len(lens) == len(freq) and max(lens) <= maxbits
    assert all((lens[i] == 0) == (freq[i] == 0) for i in range(len(freq)))
    if len(used) >= 2:
        assert sum(Fraction(1, 2 ** lens[i]) for i in used) == 1
    else:
        assert [lens[i] for i in used] == [1]
    by_freq = sorted(used, key=lambda i: freq[i])
    for a, b in zip(by_freq, by_freq[1:]):
        assert freq[a] == freq[b] or lens[a] >= lens[b], (a, b)
    depths = C.huffman_depths(freq)
    cost = sum(freq[i] * lens[i] for i in used)
    best = sum(freq[i] * depths[i] for i in used)
    print('%s: %d used, longest %d (unlimited %d), cost %d (unlimited %d)' % (name, len(used), max(lens), max(depths.values()), cost, best))
    assert cost >= best
    if max(depths.values()) <= maxbits:
        assert cost == best
    if name.startswith('fibonacci'):
        assert max(depths.values()) > maxbits          # (the limit is what these are here for)


def test_a_segment_that_needs_the_15_bit_limit(host):
    """(4) Fibonacci counts in one segment, no two equal neighbours: no matches, so the symbols are the bytes
    (png_dyn_cases.fibonacci_map says how the counts were chosen, and why not F(k), k = 1..21, over 16 rows)."""
    exe, d = host
    m = C.fibonacci_map()
    hist = np.bincount(m.reshape(-1), minlength=286)
    hist[0] += m.shape[0]                              # the filter bytes
    hist[256] += 1                                     # end of block
    depths = C.huffman_depths(hist.tolist())
    assert max(depths.values()) == 21 > 15             # a condition on the input
    (fixed,), (dynamic,) = C.run_host(exe, d, m[None], 'fixed'), C.run_host(exe, d, m[None], 'dynamic')
    C.check_file(dynamic, m)
    C.check_file(fixed, m)
    print('fibonacci map: fixed %d, dynamic %d bytes of %d' % (len(fixed), len(dynamic), m.size))
    # about 2.6 bits a byte under the limited code, 8 under the fixed one; and no more than 1 % over the unlimited code
    assert len(dynamic) < len(fixed) and len(dynamic) < m.size // 2
    unlimited_bits = sum(int(hist[s]) * depth for s, depth in depths.items())
    assert 8 * len(dynamic) <= 1.01 * unlimited_bits + 8 * 400


def test_sanitizer_build(host, tmp_path):
    """(7) the same program under AddressSanitizer and UndefinedBehaviorSanitizer, on the two smallest shapes and on (4); the
    files are those of the plain build."""
    exe = C.compile_host(tmp_path, extra=('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'))
    for shape in SHAPES[:2]:
        for kinds, px, pal, by_codes in files_of(host, shape):
            for codes in C.CODES:
                assert C.run_host(exe, tmp_path, px, codes, pal) == by_codes[codes], (shape, kinds, codes)
    m = C.fibonacci_map()[None]
    plain, _d = host
    assert C.run_host(exe, tmp_path, m, 'dynamic') == C.run_host(plain, tmp_path, m, 'dynamic')
    C.run_lengths(exe, [1] * 286, 15)


def test_encode_px_checks_its_arguments_before_any_hip_call(lib):
    T, H, W = 2, 33, 300
    p = 0x10000          # never dereferenced: every call below is refused first
    pal = bytes(768)

    def call(pixels=p, channels=3, palette=None, codes=1, blob=p, blob_bytes=None, offsets=p, T=T, H=H, W=W, ws_ptr=p, ws_bytes=None):
        cap, ws = lib.swem_png_capacity_px(H, W, channels), lib.swem_png_workspace_px(T, H, W, channels)
        return lib.swem_png_encode_px_u8(None, pixels, channels, palette, codes, blob, T * cap if blob_bytes is None else blob_bytes,
                                         offsets, T, H, W, ws_ptr, ws if ws_bytes is None else ws_bytes)
    assert call(pixels=None) == -4 and b'null pointer' in lib.swem_last_error()
    assert call(blob=None) == -4 and call(offsets=None) == -4 and call(ws_ptr=None) == -4
    assert call(ws_ptr=p + 4) == -4 and b'aligned' in lib.swem_last_error()
    assert call(channels=2) == -4 and b'channels' in lib.swem_last_error()
    assert call(channels=0) == -4 and call(channels=4) == -4
    assert call(palette=pal) == -4 and b'palette' in lib.swem_last_error()
    assert call(codes=2) == -4 and call(codes=-1) == -4
    assert call(W=21845) == -1 and b'65535' in lib.swem_last_error()           # 3 * 21845 + 1 = 65536
    assert call(channels=1, W=65535) == -1 and call(H=0) == -1 and call(W=0) == -1 and call(T=0) == -1 and call(T=65536) == -1
    for channels in (1, 3):
        cap, ws = lib.swem_png_capacity_px(H, W, channels), lib.swem_png_workspace_px(T, H, W, channels)
        assert call(channels=channels, blob_bytes=T * cap - 1) == -2 and b'insufficient workspace' in lib.swem_last_error()
        assert call(channels=channels, ws_bytes=ws - 1) == -2 and b'insufficient workspace' in lib.swem_last_error()


def test_capacity_is_the_documented_formula(lib):
    for H, W in [(1, 1), (3, 5), (17, 259), (33, 300), (480, 854), (720, 1280), (40, 5000), (2, 21844), (16, 1365), (17, 1365)]:
        for channels in (1, 3):
            assert io.png_capacity(H, W, channels) == capacity_formula(H, W, channels), (H, W, channels)
            assert lib.swem_png_capacity_px(H, W, channels) == capacity_formula(H, W, channels)
        assert io.png_capacity(H, W) == lib.swem_png_capacity(H, W) == capacity_formula(H, W, 1)
    assert io.png_capacity(480, 854, 3) == 8 + 25 + 2 + 480 * 2563 + 17 * 30 + 33 == 1230818
    assert io.png_capacity(2, 65534, 1) == capacity_formula(2, 65534, 1) and io.png_capacity(2, 65534, 3) == 0
    assert io.png_capacity(5, 21845, 3) == 0 and io.png_capacity(5, 5, 2) == 0 and io.png_capacity(0, 5, 3) == 0
    assert lib.swem_png_workspace_px(2, 33, 300, 3) >= 2 * 3 * (16 * 901 + 5)
    assert lib.swem_png_workspace_px(2, 33, 300, 1) == lib.swem_png_workspace(2, 33, 300)
    assert lib.swem_png_workspace_px(0, 33, 300, 3) == 0 and lib.swem_png_workspace_px(2, 33, 300, 2) == 0


def test_writer_refuses_unknown_switches(tmp_path):
    with pytest.raises(ValueError, match='nonsense'):
        io.IndexMapWriter(str(tmp_path), encode='device', codes='nonsense')
    with pytest.raises(ValueError, match='nonsense'):
        io.IndexMapWriter(str(tmp_path), overlay_encode='nonsense')
    with pytest.raises(ValueError, match="needs encode='device'"):
        io.IndexMapWriter(str(tmp_path), encode='host', codes='dynamic')


def test_blobs_map_against_zlib(host):
    """The ratio tests/test_gpu_png_dyn.py holds the device to, measured here with the host program: the IDAT bytes of the
    dynamic file of the 480x854 `blobs` map over zlib level 6 on the same scanlines."""
    import zlib
    from tests import png_ref_px
    exe, d = host
    m = make_map('blobs', H_BIG, W_BIG, seed=0)
    (dynamic,) = C.run_host(exe, d, m[None], 'dynamic')
    idat = png_ref_px.parse_png(dynamic)[3]['idat']
    z = len(zlib.compress(b''.join(b'\0' + m[y].tobytes() for y in range(H_BIG)), 6))
    print('blobs 480x854: IDAT %d bytes, zlib level 6 %d bytes, ratio %.4f' % (idat, z, idat / z))
    assert idat <= 1.05 * C.BLOBS_IDAT_OVER_ZLIB6 * z
