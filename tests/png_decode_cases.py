"""What tests/test_png_decode_host.py and tests/test_gpu_png_decode.py share: the good files (every one with the conditions on its
deflate stream asserted through tests/inflate_ref.py), the named malformed files, the mutation sweep, and the host program
(tests/png_decode_host.cpp) compiled and run.  Expected pixels always come from a strict reader or from the source content,
never from the code under test."""
import io as pyio
import os
import struct
import subprocess
import zlib

import numpy as np
from PIL import Image

from swem_amd import io as sio
from tests import inflate_ref as R
from tests import png_dyn_cases as C
from tests import png_ref, png_ref_px
from tests.test_gpu_png import make_map

H0, W0 = 40, 854
SHAPES = [(1, 1, 1), (2, 3, 5), (2, 17, 259), (3, 33, 300), (2, 40, 854)]
# SWEM_PNG_ST_* of include/swem_hip_io.h, by name (swem_amd.io.PNG_STATUS is the package's table; the tests hold them equal)
ST = {n: v for v, n in enumerate(
    ['OK', 'OFFSETS', 'SIGNATURE', 'CHUNK', 'CRC', 'IHDR', 'DIMENSIONS', 'UNSUPPORTED', 'METHOD', 'PLTE', 'IDAT', 'CRITICAL', 'IEND',
     'TRAILING', 'TOO_LARGE', 'ZLIB_CM', 'ZLIB_CINFO', 'ZLIB_FCHECK', 'ZLIB_FDICT', 'BLOCK_TYPE', 'STORED_LEN', 'HLIT_HDIST',
     'REPEAT', 'OVERSUBSCRIBED', 'INCOMPLETE', 'NO_EOB', 'BAD_SYMBOL', 'DISTANCE', 'NO_FINAL', 'TRUNCATED', 'IDAT_LEFT', 'LENGTH',
     'ADLER', 'FILTER', 'INDEX'])}


def compile_host(out_dir, extra=()):
    return C.compile_host(out_dir, 'png_decode_host', extra)


def run_host(exe, work_dir, files, slot_hw, channels, offsets=None, tag='batch'):
    """The files through the host program in one call -> {'pixels' (T,Hs,Ws[,3]), 'sizes' (T,2), 'palettes' (T,768), 'npal' (T,),
    'status' (T,)}.  `offsets`: in the place of the true ones."""
    T, (Hs, Ws) = len(files), slot_hw
    offs = np.cumsum([0] + [len(f) for f in files]).astype('<i8') if offsets is None else np.asarray(offsets, '<i8')
    path, out = os.path.join(str(work_dir), tag + '.bin'), os.path.join(str(work_dir), tag)
    with open(path, 'wb') as f:
        f.write(offs.tobytes() + (b''.join(files) or b'\0'))
    subprocess.run([exe, path, str(T), str(Hs), str(Ws), str(channels), out], check=True, timeout=600)
    shape = (T, Hs, Ws, 3) if channels == 3 else (T, Hs, Ws)
    return {'pixels': np.fromfile(out + '.pixels', np.uint8).reshape(shape), 'sizes': np.fromfile(out + '.sizes', '<i4').reshape(T, 2),
            'palettes': np.fromfile(out + '.palettes', np.uint8).reshape(T, 768), 'npal': np.fromfile(out + '.npal', '<i4'),
            'status': np.fromfile(out + '.status', '<i4')}


def scanlines(m):
    """Filter-0 scanlines of an (H, row_bytes) array."""
    return b''.join(b'\0' + bytes(r) for r in np.asarray(m, np.uint8))


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_every=None):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if flush_every is None:
        return c.compress(raw) + c.flush()
    out = b''
    for k in range(0, len(raw), flush_every):
        out += c.compress(raw[k:k + flush_every]) + c.flush(zlib.Z_SYNC_FLUSH)
    return out + c.flush()


def expect_of(data):
    """(pixels, palette (n,3) or None) of a good file by the strict readers: tests/png_ref_px.py at depth 8, inflate_ref's at
    depths 1, 2 and 4 (and both at depth 8 of one channel: they agree)."""
    depth, colour = data[24], data[25]
    if depth == 8:
        px, pal = png_ref_px.parse_png(data)[:2]
        if colour != 2:
            px2, pal2, _ = R.parse_png_depths(data)
            assert np.array_equal(px, px2) and (pal is None) == (pal2 is None)
        return px, pal
    px, pal, _ = R.parse_png_depths(data)
    return px, pal


def case(name, data, source=None):
    """A good file as the tests carry it; `source`: the content it was made from, which the strict reader must give back."""
    px, pal = expect_of(data)
    if source is not None:
        assert np.array_equal(px, source), name
    return {'name': name, 'data': bytes(data), 'want': px, 'palette': pal, 'channels': 3 if px.ndim == 3 else 1}


PAL = bytes(np.asarray(sio.default_palette(), np.uint8))


def gray(m, stream=None, **kw):
    m = np.asarray(m, np.uint8)
    return R.png_file(m.shape[1], m.shape[0], 8, 0, deflate(scanlines(m)) if stream is None else stream, **kw)


def stream_cases(dyn_host=None):
    """The deflate streams of the issue's table on filter-0 rows of make_map(kind, 40, 854), every condition asserted."""
    blobs, noise = make_map('blobs', H0, W0), make_map('noise256', H0, W0, seed=3)
    raw = scanlines(blobs)
    out = []

    def add(name, m, stream, check, palette=None):
        got, st = R.inflate(stream)
        assert got == scanlines(m), name
        assert check(st), (name, {k: v for k, v in st.items() if k != 'blocks'}, st['blocks'][:8])
        out.append(case(name, R.png_file(m.shape[1], m.shape[0], 8, 3 if palette else 0, stream, palette=palette), m))
    add('level6', blobs, deflate(raw, 6), lambda s: s['blocks'] == ['dynamic'] and s['max_distance'] > 8192 and s['overlaps'] > 0, PAL)
    add('fixed', blobs, deflate(raw, 6, zlib.Z_FIXED), lambda s: s['blocks'] == ['fixed'])
    add('huffman_only', blobs, deflate(raw, 6, zlib.Z_HUFFMAN_ONLY), lambda s: s['matches'] == 0 and set(s['blocks']) == {'dynamic'})
    add('rle', blobs, deflate(raw, 6, zlib.Z_RLE), lambda s: s['max_distance'] == 1 and s['matches'] > 0)
    add('level0', blobs, deflate(raw, 0), lambda s: set(s['blocks']) == {'stored'})
    add('noise', noise, deflate(scanlines(noise), 6), lambda s: set(s['blocks']) == {'stored'})
    small = deflate(raw, 9, wbits=9)
    assert small[0] >> 4 == 1
    add('window512', blobs, small, lambda s: 1 <= s['max_distance'] <= 512)
    add('sync_flush', blobs, deflate(raw, 6, flush_every=1000),
        lambda s: s['empty_stored'] >= 30 and set(s['blocks']) == {'fixed', 'stored', 'dynamic'} and s['blocks'].count('fixed') >= 30)
    far = noise.copy()
    far[38:40] = far[0:2]
    add('far_match', far, deflate(scanlines(far), 9), lambda s: s['max_distance'] == 38 * (W0 + 1))
    # distance 32768, which zlib never emits: a stored block of the first 32768 bytes, then a fixed block whose first token is a
    # match of 258 bytes at that distance.  Byte 32768 is pixel 277 of row 38: the copy stays inside that row.
    edge = noise.copy()
    flat = bytearray(scanlines(edge))
    flat[32768:32768 + 258] = flat[0:258]
    edge = np.frombuffer(bytes(flat), np.uint8).reshape(H0, W0 + 1)[:, 1:].copy()
    assert scanlines(edge) == bytes(flat)
    w = R.BitWriter().stored(flat[:32768]).block(1, 1).fixed_match(258, 32768)
    for b in flat[32768 + 258:]:
        w.fixed_symbol(b)
    w.fixed_symbol(256)
    add('distance32768', edge, R.zlib_wrap(w.getvalue(), flat),
        lambda s: s['max_distance'] == 32768 and s['max_length'] == 258 and s['blocks'] == ['stored', 'fixed'])
    return out


def fibonacci_case(dyn_exe, work_dir):
    """15-bit codes: png_dyn_cases.fibonacci_map() through the project's own dynamic encoder."""
    m = C.fibonacci_map()
    (data,) = C.run_host(dyn_exe, work_dir, m[None], 'dynamic')
    _got, st = R.inflate(R.idat_stream(data))
    assert st['longest_ll'] == 15 and set(st['dist_codes']) == {1}, (st['longest_ll'], st['dist_codes'])
    return case('fibonacci', data, m)


def depth_cases():
    """Depths 1, 2, 4 and 8, grayscale and palette, every number of padding bits; PIL's own choice of depth for palettes of 2, 4,
    16 and 17 entries."""
    rng = np.random.RandomState(4)
    out = []
    for depth in (1, 2, 4, 8):
        for W in list(range(1, 18)) + [70, 131]:
            H = 3
            s = rng.randint(0, 1 << depth, (H, W)).astype(np.uint8)
            rows = R.pack_rows(s, depth)
            types = [(W + y) % 5 for y in range(H)]
            stream = deflate(R.filter_rows(rows, types, 1))
            pal = bytes(rng.randint(0, 256, 3 * (1 << min(depth, 5))).astype(np.uint8)) if W % 2 else None
            if pal is not None and depth == 8:
                s = s % 32
                stream = deflate(R.filter_rows(s, types, 1))
            out.append(case('depth%d_w%d' % (depth, W), R.png_file(W, H, depth, 3 if pal else 0, stream, palette=pal), s))
    for n, depth in ((2, 1), (4, 2), (16, 4), (17, 8)):
        idx = rng.randint(0, n, (9, 21)).astype(np.uint8)
        for optimize in (False, True):
            img = Image.fromarray(idx, 'P')
            img.putpalette(list(range(3 * n)))
            buf = pyio.BytesIO()
            img.save(buf, 'PNG', optimize=optimize)
            data = buf.getvalue()
            assert data[24] == depth, (n, data[24])
            out.append(case('pil_p%d_%d' % (n, optimize), data, idx))
    return out


def filter_cases():
    """Every filter type on every row position (row 0 included) for bpp 1 and 3, rows past 64 bytes, and rows past one tile of
    the serial unfilter; PIL's own L and RGB files."""
    rng = np.random.RandomState(6)
    out = []
    for bpp in (1, 3):
        H, W = 5, 70
        px = rng.randint(0, 256, (H, W, 3) if bpp == 3 else (H, W)).astype(np.uint8)
        rows = px.reshape(H, -1)
        for k in range(5):
            for name, types in (('same', [k] * H), ('turn', [(k + y) % 5 for y in range(H)])):
                raw = R.filter_rows(rows, types, bpp)
                out.append(case('filter_bpp%d_%s%d' % (bpp, name, k), R.png_file(W, H, 8, 2 if bpp == 3 else 0, deflate(raw)), px))
        W = 2200 if bpp == 3 else 6300                       # rows of 6600 and 6300 bytes: past a tile of 6144
        px = rng.randint(0, 256, (3, W, 3) if bpp == 3 else (3, W)).astype(np.uint8)
        for types in ([4, 3, 1], [3, 4, 2]):
            raw = R.filter_rows(px.reshape(3, -1), types, bpp)
            out.append(case('filter_bpp%d_wide%d' % (bpp, types[0]), R.png_file(W, 3, 8, 2 if bpp == 3 else 0, deflate(raw)), px))
    y, x = np.mgrid[0:24, 0:37]
    for mode, px in (('L', ((3 * x + 5 * y) % 256).astype(np.uint8)), ('RGB', C.make_picture('gradient', 24, 37, 2)),
                     ('RGB', C.make_picture('blend', 24, 37, 3))):
        for optimize in (False, True):
            buf = pyio.BytesIO()
            Image.fromarray(px, mode).save(buf, 'PNG', optimize=optimize)
            out.append(case('pil_%s_%d' % (mode, optimize), buf.getvalue(), px))
    return out


def container_cases():
    """One stream cut into IDAT chunks of one byte, zero-length IDAT chunks, ancillary chunks before, between and after."""
    m = make_map('blobs', 17, 59, seed=2)
    stream = deflate(scanlines(m))
    n = len(stream)
    anc = [R.chunk(b'gAMA', struct.pack('>I', 45455)), R.chunk(b'tEXt', b'Comment\0a test'), R.chunk(b'tIME', bytes(7))]
    return [case('one_byte_idats', R.png_file(59, 17, 8, 3, stream, palette=PAL, cuts=list(range(1, n))), m),
            case('empty_idats', R.png_file(59, 17, 8, 0, stream, cuts=[0, 0, 5, 5, 5, n // 2, n, n]), m),
            case('ancillary', R.png_file(59, 17, 8, 3, stream, palette=PAL[:30], cuts=[7], before=anc[:1], between=anc[1:2], after=anc), m)]


def shape_cases():
    """The shapes of tests/test_gpu_png.py, every kind of content, zlib's files with and without a palette."""
    from tests.test_gpu_png import calls_of
    out = []
    for shape in SHAPES:
        for k, (kinds, maps) in enumerate(calls_of(shape)):
            for t, kind in enumerate(kinds):
                m = maps[t]
                out.append(case('shape%dx%d_%s' % (shape[1], shape[2], kind),
                                R.png_file(m.shape[1], m.shape[0], 8, 3 if k % 2 == 0 else 0, deflate(scanlines(m)),
                                           palette=PAL if k % 2 == 0 else None), m))
    return out


_good = {}


def good_cases():
    """Every good file but the Fibonacci one (which needs the encoder's host program), built once."""
    if not _good:
        _good['all'] = stream_cases() + depth_cases() + filter_cases() + container_cases() + shape_cases()
    return _good['all']


def calls_of_cases(cases):
    """[(channels, (Hs, Ws), [case])]: the cases of one size and channel count share a call whose slot they fill exactly; every
    one-channel case no wider than 900 also goes into one call with a 40 x 900 slot (files smaller than the slot, many sizes)."""
    groups = {}
    for c in cases:
        groups.setdefault((c['channels'],) + c['want'].shape[:2], []).append(c)
    calls = [(k[0], k[1:], v) for k, v in sorted(groups.items())]
    mixed = [c for c in cases if c['channels'] == 1 and c['want'].shape[0] <= 40 and c['want'].shape[1] <= 900]
    calls.append((1, (40, 900), mixed[::3]))
    mixed3 = [c for c in cases if c['channels'] == 3 and c['want'].shape[1] <= 80]
    calls.append((3, (24, 80), mixed3))
    return calls


def check_result(res, t, c, slot_hw):
    """File t of a call's result against case c: status 0, the size, the pixels in the top-left corner and zeros around them,
    the palette zero-padded."""
    assert int(res['status'][t]) == 0, (c['name'], int(res['status'][t]))
    h, w = c['want'].shape[:2]
    assert tuple(res['sizes'][t]) == (h, w), c['name']
    slot = res['pixels'][t]
    assert np.array_equal(slot[:h, :w], c['want']), c['name']
    assert not slot[h:].any() and not slot[:, w:].any(), c['name']
    pal = np.zeros(768, np.uint8)
    if c['palette'] is not None:
        pal[:c['palette'].size] = c['palette'].reshape(-1)
    assert np.array_equal(res['palettes'][t], pal), c['name']
    assert int(res['npal'][t]) == (0 if c['palette'] is None else len(c['palette'])), c['name']


# ---- the named malformed files: one per entry of the refusal list (include/swem_hip_io.h), decoded in a slot of BAD_SLOT
BAD_SLOT = (8, 12)


def _dyn_header(w, hlit, hdist, cl):
    """BFINAL 1, BTYPE 10, the counts, and the code-length code lengths {symbol: length} written up to the last one set."""
    order = R.CL_ORDER
    ncode = max(4, max(order.index(s) for s in cl) + 1)
    w.block(1, 2).bits(hlit, 5).bits(hdist, 5).bits(ncode - 4, 4)
    for k in range(ncode):
        w.bits(cl.get(order[k], 0), 3)
    return w


def base_files():
    m = make_map('blobs', 6, 9, seed=5)
    m[0, :3] = [7, 1, 4]
    g = gray(m)
    p = R.png_file(9, 6, 8, 3, deflate(scanlines(m % 3)), palette=PAL[:9])
    return m, g, p


def malformed_cases():
    """[(name, file, status name, channels)].  Every file has one defect; all CRCs are correct unless the CRC is the defect."""
    m, g, p = base_files()
    raw = scanlines(m)
    good = deflate(raw)
    cs = R.split_chunks(g)
    pcs = R.split_chunks(p)
    H, W = m.shape

    def hdr(**kw):
        a = dict(w=W, h=H, depth=8, colour=0, comp=0, filt=0, lace=0)
        a.update(kw)
        return R.join_chunks([(b'IHDR', struct.pack('>IIBBBBB', a['w'], a['h'], a['depth'], a['colour'], a['comp'], a['filt'], a['lace']))] + cs[1:])

    def zl(deflate_bytes, data=raw, **kw):
        return R.with_stream(g, R.zlib_wrap(deflate_bytes, data, **kw))
    idat_at = g.index(b'IDAT')
    out = [
        ('signature', b'\x88' + g[1:], 'SIGNATURE'),
        ('chunk_past_file', g[:idat_at - 4] + struct.pack('>I', 10 ** 6) + g[idat_at:], 'CHUNK'),
        ('crc', g[:idat_at + 8] + bytes([g[idat_at + 8] ^ 0x10]) + g[idat_at + 9:], 'CRC'),
        ('crc_field', g[:-1] + bytes([g[-1] ^ 1]), 'CRC'),
        ('ihdr_not_first', R.join_chunks([(b'gAMA', bytes(4))] + cs), 'IHDR'),
        ('ihdr_twice', R.join_chunks(cs[:1] + cs[:1] + cs[1:]), 'IHDR'),
        ('ihdr_14_bytes', R.join_chunks([(b'IHDR', cs[0][1] + b'\0')] + cs[1:]), 'IHDR'),
        ('width_zero', hdr(w=0), 'DIMENSIONS'),
        ('height_2_31', hdr(h=1 << 31), 'DIMENSIONS'),
        ('depth_16', hdr(depth=16), 'UNSUPPORTED'),
        ('depth_3', hdr(depth=3), 'UNSUPPORTED'),
        ('gray_alpha', hdr(colour=4), 'UNSUPPORTED'),
        ('rgba', hdr(colour=6), 'UNSUPPORTED'),
        ('rgb_depth_4', hdr(colour=2, depth=4), 'UNSUPPORTED'),
        ('interlaced', hdr(lace=1), 'UNSUPPORTED'),
        ('truecolour_in_one_channel', R.png_file(3, 2, 8, 2, deflate(scanlines(np.arange(18).reshape(2, 9)))), 'UNSUPPORTED'),
        ('compression_1', hdr(comp=1), 'METHOD'),
        ('filter_method_1', hdr(filt=1), 'METHOD'),
        ('plte_missing', R.join_chunks([c for c in pcs if c[0] != b'PLTE']), 'PLTE'),
        ('plte_late', R.join_chunks([pcs[0], pcs[2], pcs[1]] + pcs[3:]), 'PLTE'),
        ('plte_twice', R.join_chunks(pcs[:2] + pcs[1:]), 'PLTE'),
        ('plte_4_bytes', R.join_chunks([pcs[0], (b'PLTE', bytes(4))] + pcs[2:]), 'PLTE'),
        ('plte_771_bytes', R.join_chunks([pcs[0], (b'PLTE', bytes(771))] + pcs[2:]), 'PLTE'),
        ('plte_in_gray', R.join_chunks(cs[:1] + [(b'PLTE', bytes(9))] + cs[1:]), 'PLTE'),
        ('idat_absent', R.join_chunks([c for c in cs if c[0] != b'IDAT']), 'IDAT'),
        ('idat_apart', R.png_file(W, H, 8, 0, good[:5]) [:-12] + R.chunk(b'tEXt', b'k\0v') + R.chunk(b'IDAT', good[5:]) + R.chunk(b'IEND'), 'IDAT'),
        ('critical_unknown', R.join_chunks(cs[:1] + [(b'ABCD', b'xyz')] + cs[1:]), 'CRITICAL'),
        ('iend_missing', R.join_chunks(cs[:-1]), 'IEND'),
        ('iend_not_empty', R.join_chunks(cs[:-1] + [(b'IEND', b'\0')]), 'IEND'),
        ('after_iend', g + b'\0', 'TRAILING'),
        ('taller_than_slot', gray(np.zeros((BAD_SLOT[0] + 1, 5), np.uint8)), 'TOO_LARGE'),
        ('wider_than_slot', gray(np.zeros((2, BAD_SLOT[1] + 1), np.uint8)), 'TOO_LARGE'),
        ('zlib_cm_9', zl(good[2:-4], cmf=0x79), 'ZLIB_CM'),
        ('zlib_cinfo_8', zl(good[2:-4], cmf=0x88), 'ZLIB_CINFO'),
        ('zlib_fcheck', R.with_stream(g, good[:1] + bytes([good[1] ^ 1]) + good[2:]), 'ZLIB_FCHECK'),
        ('zlib_fdict', zl(good[2:-4], flg=0x20 + (31 - (0x78 * 256 + 0x20) % 31) % 31), 'ZLIB_FDICT'),
        ('block_type_3', zl(R.BitWriter().block(1, 3).bits(0, 13).getvalue()), 'BLOCK_TYPE'),
        ('stored_nlen', zl(b'\x01' + struct.pack('<HH', len(raw), len(raw)) + raw), 'STORED_LEN'),
        ('hlit_287', zl(R.BitWriter().block(1, 2).bits(30, 5).bits(0, 5).bits(0, 4).bits(0, 32).getvalue()), 'HLIT_HDIST'),
        ('hdist_31', zl(R.BitWriter().block(1, 2).bits(0, 5).bits(30, 5).bits(0, 4).bits(0, 32).getvalue()), 'HLIT_HDIST'),
        # the code-length code {1: 1 bit, 16: 1 bit}: symbol 1 is code 0, symbol 16 code 1; the first length is a repeat
        ('repeat_without_previous', zl(_dyn_header(R.BitWriter(), 0, 0, {1: 1, 16: 1}).code(1, 1).bits(0, 2).bits(0, 32).getvalue()), 'REPEAT'),
        # {1: 1 bit, 18: 1 bit}: 138 zeros twice are 276 lengths of 258
        ('repeat_past_the_end', zl(_dyn_header(R.BitWriter(), 0, 0, {1: 1, 18: 1}).code(1, 1).bits(127, 7).code(1, 1).bits(127, 7)
                                   .bits(0, 32).getvalue()), 'REPEAT'),
        ('oversubscribed', zl(_dyn_header(R.BitWriter(), 0, 0, {0: 1, 1: 1, 2: 1}).bits(0, 32).getvalue()), 'OVERSUBSCRIBED'),
        ('incomplete', zl(_dyn_header(R.BitWriter(), 0, 0, {1: 1}).bits(0, 32).getvalue()), 'INCOMPLETE'),
        # lengths: 1, 1, then 138 + 118 zeros: symbols 0 and 1 have codes, 256 has none
        ('no_end_of_block', zl(_dyn_header(R.BitWriter(), 0, 0, {1: 1, 18: 1}).code(0, 1).code(0, 1).code(1, 1).bits(127, 7).code(1, 1)
                               .bits(107, 7).bits(0, 32).getvalue()), 'NO_EOB'),
        ('symbol_286', zl(R.BitWriter().block(1, 1).fixed_symbol(286).bits(0, 32).getvalue()), 'BAD_SYMBOL'),
        ('distance_symbol_30', zl(R.BitWriter().block(1, 1).fixed_symbol(65).fixed_symbol(257).code(30, 5).bits(0, 32).getvalue()),
         'BAD_SYMBOL'),
        ('distance_before_start', zl(R.BitWriter().block(1, 1).fixed_symbol(0).fixed_match(3, 2).bits(0, 32).getvalue()), 'DISTANCE'),
        ('no_final_block', R.with_stream(g, b'\x78\x01' + R.BitWriter().stored(raw, 0).getvalue()), 'NO_FINAL'),
        ('cut_inside_a_block', R.with_stream(g, good[:len(good) // 2]), 'TRUNCATED'),
        ('cut_inside_the_adler', R.with_stream(g, good[:-2]), 'TRUNCATED'),
        ('idat_left', R.with_stream(g, good + b'\0'), 'IDAT_LEFT'),
        ('one_byte_short', R.with_stream(g, deflate(raw[:-1])), 'LENGTH'),
        ('one_byte_long', R.with_stream(g, deflate(raw + b'\0')), 'LENGTH'),
        ('adler', R.with_stream(g, good[:-1] + bytes([good[-1] ^ 1])), 'ADLER'),
        ('filter_5', R.with_stream(g, deflate(raw[:W + 1] + b'\5' + raw[W + 2:])), 'FILTER'),
        ('index_past_plte', R.png_file(9, 6, 8, 3, deflate(scanlines(m % 4)), palette=PAL[:9]), 'INDEX'),
    ]
    assert int((m % 4).max()) == 3
    return [(n, d, s, 1) for n, d, s in out] + [
        ('gray_in_three_channels', g, 'UNSUPPORTED', 3),
        ('rgb_filter_5', R.png_file(3, 2, 8, 2, deflate(b'\5' + bytes(9) + b'\0' + bytes(9))), 'FILTER', 3)]


def strict_accepts(data, channels=1):
    """The strict reader's verdict on any bytes: (pixels, palette) or None where it raises."""
    try:
        if len(data) > 25 and data[24] != 8:
            px, pal, _ = R.parse_png_depths(data)
        else:
            px, pal = png_ref_px.parse_png(data)[:2]
    except (png_ref.PngError, struct.error, IndexError, ValueError):
        return None
    return px, pal


# ---- the mutation sweep
def sweep_files(data):
    """Every single-byte change at three values, every truncation, and the same applied to the zlib stream and re-wrapped with
    correct CRCs."""
    out = []

    def mutations(b):
        for i in range(len(b)):
            for x in (0x01, 0x80, 0xff):
                yield b[:i] + bytes([b[i] ^ x]) + b[i + 1:]
        for n in range(len(b)):
            yield b[:n]
    out += list(mutations(data))
    stream = R.idat_stream(data)
    out += [R.with_stream(data, s) for s in mutations(stream)]
    return out


def sweep_bases():
    """One small grayscale file (a fixed block) and one small file with a dynamic block; the conditions asserted."""
    m, g, _p = base_files()
    assert R.inflate(R.idat_stream(g))[1]['blocks'] == ['fixed']
    rng = np.random.RandomState(9)
    d = np.where(rng.rand(12, 40) < 0.8, 0, rng.randint(0, 6, (12, 40))).astype(np.uint8)
    d[3:9, 10:30] = 200
    dyn = gray(d)
    st = R.inflate(R.idat_stream(dyn))[1]
    assert st['blocks'] == ['dynamic'] and st['matches'] > 0, st['blocks']
    return [('fixed', g, m), ('dynamic', dyn, d)]


def check_sweep(res, files, slot_hw):
    """Zero / non-zero against the strict reader; where it accepts, equal pixels.  Returns (accepted, refused)."""
    accepted = 0
    for t, data in enumerate(files):
        verdict = strict_accepts(data)
        if verdict is not None and (verdict[0].ndim != 2 or verdict[0].shape[0] > slot_hw[0] or verdict[0].shape[1] > slot_hw[1]):
            verdict = None                                # (a changed header the slot does not take)
        if verdict is None:
            assert int(res['status'][t]) != 0, (t, len(data))
            assert not res['pixels'][t].any() and tuple(res['sizes'][t]) == (0, 0), t
        else:
            assert int(res['status'][t]) == 0, (t, int(res['status'][t]))
            h, w = verdict[0].shape
            assert np.array_equal(res['pixels'][t][:h, :w], verdict[0]), t
            accepted += 1
    return accepted, len(files) - accepted
