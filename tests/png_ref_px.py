"""The strict reader of tests/png_ref.py with truecolour beside palette and grayscale: 8-bit colour types 0, 2 and 3, an unfilter
for `bpp` bytes per pixel (PNG specification section 9.2).  As strict as its neighbour: chunk lengths, CRCs and order are
png_ref.chunks'; the deflate stream must end exactly where the IDAT data ends (zlib checks the Adler-32); nothing may follow
IEND.  Inflating is zlib's."""
import struct
import zlib

import numpy as np

from tests.png_ref import PngError, _paeth, chunks


def unfilter(raw, H, row_bytes, bpp):
    """Filtered scanlines (a filter byte, then row_bytes bytes) -> (H, row_bytes) uint8; filter types 0-4."""
    if len(raw) != H * (row_bytes + 1):
        raise PngError('%d bytes of scanlines, %d x (%d + 1) expected' % (len(raw), H, row_bytes))
    out = np.zeros((H, row_bytes), np.uint8)
    prev = np.zeros(row_bytes, np.uint8)
    for y in range(H):
        ft = raw[y * (row_bytes + 1)]
        line = np.frombuffer(raw, np.uint8, row_bytes, y * (row_bytes + 1) + 1)
        if ft == 0:
            cur = line.copy()
        elif ft == 1:
            cur = np.empty(row_bytes, np.uint8)
            for k in range(min(bpp, row_bytes)):
                cur[k::bpp] = np.cumsum(line[k::bpp], dtype=np.uint64).astype(np.uint8)     # (mod 256)
        elif ft == 2:
            cur = line + prev                                                             # (uint8: mod 256)
        elif ft in (3, 4):
            ln, up, c = line.tolist(), prev.tolist(), [0] * row_bytes
            for x in range(row_bytes):
                a = c[x - bpp] if x >= bpp else 0
                if ft == 3:
                    c[x] = (ln[x] + ((a + up[x]) >> 1)) & 255
                else:
                    c[x] = (ln[x] + _paeth(a, up[x], up[x - bpp] if x >= bpp else 0)) & 255
            cur = np.asarray(c, np.uint8)
        else:
            raise PngError('scanline %d: filter type %d' % (y, ft))
        out[y] = cur
        prev = cur
    return out


def parse_png(data):
    """-> (pixels (H,W) or (H,W,3) uint8, palette (n,3) uint8 or None, n_idat, sizes, filter types per row) with sizes =
    {'file', 'idat' (compressed bytes), 'raw' (filtered bytes)}.  8-bit colour type 3 (PLTE required, before IDAT), 0 or 2
    (PLTE forbidden here: this encoder never writes a suggested palette), no interlace."""
    data = bytes(data)
    cs = chunks(data)
    types = [c[0] for c in cs]
    if types[0] != b'IHDR' or types.count(b'IHDR') != 1 or len(cs[0][1]) != 13:
        raise PngError('IHDR must come first, once, with 13 bytes')
    W, H, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', cs[0][1])
    if W < 1 or H < 1 or W > 0x7fffffff or H > 0x7fffffff:
        raise PngError('IHDR: %d x %d' % (W, H))
    if depth != 8 or colour not in (0, 2, 3) or comp != 0 or filt != 0 or lace != 0:
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
        raise PngError('PLTE in a file of colour type %d' % colour)
    stream = b''.join(cs[i][1] for i in idat)
    d = zlib.decompressobj(15)
    try:
        raw = d.decompress(stream)
    except zlib.error as e:
        raise PngError('inflate: %s' % e)
    if not d.eof or d.unused_data or d.unconsumed_tail:
        raise PngError('the deflate stream does not end with the IDAT data (eof=%s, %d bytes unused)' % (d.eof, len(d.unused_data)))
    bpp = 3 if colour == 2 else 1
    pixels = unfilter(raw, H, bpp * W, bpp)
    filters = [raw[y * (bpp * W + 1)] for y in range(H)]
    if colour == 2:
        pixels = pixels.reshape(H, W, 3)
    if palette is not None and int(pixels.max()) >= len(palette):
        raise PngError('index %d beyond a palette of %d' % (int(pixels.max()), len(palette)))
    return pixels, palette, len(idat), {'file': len(data), 'idat': len(stream), 'raw': len(raw)}, filters
