"""A strict reader for 8-bit palette / grayscale PNG files: the yardstick of tests/test_gpu_png.py, written from the PNG
specification (ISO/IEC 15948, sections 5, 9, 11) and RFC 1950; inflating is zlib's.  Everything a lenient viewer would let
pass is an error here: a wrong length, a wrong CRC, chunks out of order, bytes after IEND, a deflate stream that does not end
exactly where the IDAT data ends (zlib checks the Adler-32 on the way)."""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


class PngError(ValueError):
    pass


def chunks(data):
    """[(type, payload)] of a whole file; every length and CRC checked, nothing may follow IEND."""
    if data[:8] != SIGNATURE:
        raise PngError('bad signature')
    pos, out = 8, []
    while True:
        if pos + 12 > len(data):
            raise PngError('truncated chunk at byte %d' % pos)
        n, = struct.unpack('>I', data[pos:pos + 4])
        ctype = bytes(data[pos + 4:pos + 8])
        if pos + 12 + n > len(data):
            raise PngError('chunk %r at byte %d runs past the end of the file' % (ctype, pos))
        body = bytes(data[pos + 8:pos + 8 + n])
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(ctype + body) & 0xffffffff):
            raise PngError('chunk %r at byte %d: CRC %08x, computed %08x' % (ctype, pos, crc, zlib.crc32(ctype + body) & 0xffffffff))
        out.append((ctype, body))
        pos += 12 + n
        if ctype == b'IEND':
            break
    if pos != len(data):
        raise PngError('%d bytes after IEND' % (len(data) - pos))
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(raw, H, W):
    """Filtered scanlines (a filter byte, then W bytes; one byte per pixel) -> (H, W) uint8; filter types 0-4."""
    if len(raw) != H * (W + 1):
        raise PngError('%d bytes of scanlines, %d x (%d + 1) expected' % (len(raw), H, W))
    out = np.zeros((H, W), np.uint8)
    prev = [0] * W
    for y in range(H):
        ft = raw[y * (W + 1)]
        line = list(raw[y * (W + 1) + 1:(y + 1) * (W + 1)])
        if ft == 0:
            cur = line
        elif ft == 1:
            cur = []
            for x in range(W):
                cur.append((line[x] + (cur[x - 1] if x else 0)) & 255)
        elif ft == 2:
            cur = [(line[x] + prev[x]) & 255 for x in range(W)]
        elif ft == 3:
            cur = []
            for x in range(W):
                cur.append((line[x] + (((cur[x - 1] if x else 0) + prev[x]) >> 1)) & 255)
        elif ft == 4:
            cur = []
            for x in range(W):
                cur.append((line[x] + _paeth(cur[x - 1] if x else 0, prev[x], prev[x - 1] if x else 0)) & 255)
        else:
            raise PngError('scanline %d: filter type %d' % (y, ft))
        out[y] = cur
        prev = cur
    return out


def parse_png(data):
    """-> (index_map (H,W) uint8, palette (n,3) uint8 or None, n_idat, sizes) with sizes = {'file', 'idat' (compressed bytes),
    'raw' (filtered bytes)}.  8-bit colour type 3 (PLTE required, before IDAT) or 0 (PLTE forbidden), no interlace."""
    data = bytes(data)
    cs = chunks(data)
    types = [c[0] for c in cs]
    if types[0] != b'IHDR' or types.count(b'IHDR') != 1 or len(cs[0][1]) != 13:
        raise PngError('IHDR must come first, once, with 13 bytes')
    W, H, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', cs[0][1])
    if W < 1 or H < 1 or W > 0x7fffffff or H > 0x7fffffff:
        raise PngError('IHDR: %d x %d' % (W, H))
    if depth != 8 or colour not in (0, 3) or comp != 0 or filt != 0 or lace != 0:
        raise PngError('IHDR: depth %d colour %d compression %d filter %d interlace %d' % (depth, colour, comp, filt, lace))
    if types[-1] != b'IEND' or types.count(b'IEND') != 1 or cs[-1][1]:
        raise PngError('IEND must come last, once, empty')
    idat = [i for i, t in enumerate(types) if t == b'IDAT']
    if not idat or idat != list(range(idat[0], idat[0] + len(idat))):
        raise PngError('IDAT chunks must be there and consecutive')
    for t in types:
        if t not in (b'IHDR', b'PLTE', b'IDAT', b'IEND') and not (t[0] & 0x20):
            raise PngError('unknown critical chunk %r' % t)
    palette = None
    if colour == 3:
        if types.count(b'PLTE') != 1 or types.index(b'PLTE') > idat[0]:
            raise PngError('colour type 3 needs one PLTE before the first IDAT')
        body = cs[types.index(b'PLTE')][1]
        if len(body) % 3 or not 3 <= len(body) <= 768:
            raise PngError('PLTE of %d bytes' % len(body))
        palette = np.frombuffer(body, np.uint8).reshape(-1, 3).copy()
    elif b'PLTE' in types:
        raise PngError('PLTE in a grayscale file')
    stream = b''.join(cs[i][1] for i in idat)
    d = zlib.decompressobj(15)
    try:
        raw = d.decompress(stream)
    except zlib.error as e:
        raise PngError('inflate: %s' % e)
    if not d.eof or d.unused_data or d.unconsumed_tail:
        raise PngError('the deflate stream does not end with the IDAT data (eof=%s, %d bytes unused)' % (d.eof, len(d.unused_data)))
    index_map = unfilter(raw, H, W)
    if palette is not None and int(index_map.max()) >= len(palette):
        raise PngError('index %d beyond a palette of %d' % (int(index_map.max()), len(palette)))
    return index_map, palette, len(idat), {'file': len(data), 'idat': len(stream), 'raw': len(raw)}
