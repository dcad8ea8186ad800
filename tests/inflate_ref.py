"""A pure-Python inflate written from RFC 1951 (and the zlib wrapper of RFC 1950), the yardstick of the device PNG decoder's
tests beside zlib itself: it returns, with the bytes, the statistics the tests assert about their inputs -- block types, the
longest codes, the largest distance and length, the matches longer than their distance -- so that a case cannot silently stop
covering its ground.  Every stream it inflates is also compared with zlib.decompress.  Also: a deflate bit writer for hand-made
streams, a PNG chunk writer with correct CRCs, a scanline filter writer, and a strict reader for depths 1, 2 and 4
(tests/png_ref.py and tests/png_ref_px.py cover depth 8)."""
import struct
import zlib

import numpy as np

from tests import png_ref, png_ref_px
from tests.png_ref import PngError

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class InflateError(ValueError):
    pass


class _Bits:
    def __init__(self, data, pos=0):
        self.data, self.pos, self.bit = data, pos, 0

    def take(self, n):
        v = 0
        for k in range(n):
            if self.pos >= len(self.data):
                raise InflateError('the input ends inside the stream')
            v |= ((self.data[self.pos] >> self.bit) & 1) << k
            self.bit += 1
            if self.bit == 8:
                self.bit, self.pos = 0, self.pos + 1
        return v

    def to_byte(self):
        if self.bit:
            self.bit, self.pos = 0, self.pos + 1


def _codes(lengths, what, complete):
    """{(length, code): symbol} of the canonical code (section 3.2.2); over-subscribed sets raise, incomplete ones too unless
    empty or a single code of one bit (zlib's rule), or always when `complete`."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    left = 1
    for b in range(1, 16):
        left = 2 * left - count[b]
        if left < 0:
            raise InflateError('over-subscribed %s code' % what)
    longest = max([l for l in lengths if l] or [0])
    if left > 0 and longest and (complete or longest != 1):
        raise InflateError('incomplete %s code' % what)
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table, longest


def _symbol(bits, table, what):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (l, code) in table:
            return table[(l, code)]
    raise InflateError('a %s code that no symbol has' % what)


def inflate_raw(data, pos=0):
    """The deflate stream at data[pos:] -> (bytes, statistics, position of the first byte after it)."""
    bits = _Bits(data, pos)
    out = bytearray()
    st = {'blocks': [], 'longest_ll': 0, 'longest_dist': 0, 'max_distance': 0, 'max_length': 0, 'overlaps': 0, 'matches': 0,
          'dist_codes': [], 'empty_stored': 0}
    while True:
        final, btype = bits.take(1), bits.take(2)
        st['blocks'].append(('stored', 'fixed', 'dynamic', 'reserved')[btype])
        if btype == 3:
            raise InflateError('block type 3')
        if btype == 0:
            bits.to_byte()
            n, c = bits.take(16), bits.take(16)
            if n != (~c & 0xffff):
                raise InflateError('stored block: LEN %d, NLEN %d' % (n, c))
            if bits.pos + n > len(data):
                raise InflateError('the input ends inside a stored block')
            out += data[bits.pos:bits.pos + n]
            bits.pos += n
            st['empty_stored'] += n == 0
        else:
            if btype == 1:
                ll, dist = FIXED_LL, FIXED_DIST
            else:
                nlen, ndist, ncode = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                if nlen > 286 or ndist > 30:
                    raise InflateError('HLIT %d, HDIST %d' % (nlen, ndist))
                cl = [0] * 19
                for k in range(ncode):
                    cl[CL_ORDER[k]] = bits.take(3)
                cltab, _ = _codes(cl, 'code-length', True)
                lens = []
                while len(lens) < nlen + ndist:
                    s = _symbol(bits, cltab, 'code-length')
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise InflateError('a repeat with no length before it')
                        rep, v = 3 + bits.take(2), lens[-1]
                    elif s == 17:
                        rep, v = 3 + bits.take(3), 0
                    else:
                        rep, v = 11 + bits.take(7), 0
                    if len(lens) + rep > nlen + ndist:
                        raise InflateError('a repeat past the last length')
                    lens += [v] * rep
                if not lens[256]:
                    raise InflateError('no code for the end of block')
                ll, dist = lens[:nlen], lens[nlen:]
                st['dist_codes'].append(sum(1 for l in dist if l))
            lltab, a = _codes(ll, 'literal/length', False)
            dtab, b = _codes(dist, 'distance', False)
            if btype == 2:
                st['longest_ll'], st['longest_dist'] = max(st['longest_ll'], a), max(st['longest_dist'], b)
            while True:
                s = _symbol(bits, lltab, 'literal/length')
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise InflateError('length symbol %d' % s)
                    n = LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])
                    d = _symbol(bits, dtab, 'distance')
                    if d > 29:
                        raise InflateError('distance symbol %d' % d)
                    d = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                    if d > len(out):
                        raise InflateError('distance %d with %d bytes of output' % (d, len(out)))
                    for k in range(n):
                        out.append(out[-d])
                    st['matches'] += 1
                    st['max_distance'], st['max_length'] = max(st['max_distance'], d), max(st['max_length'], n)
                    st['overlaps'] += n > d
        if final:
            break
    bits.to_byte()
    return bytes(out), st, bits.pos


def inflate(stream):
    """A zlib stream (RFC 1950) -> (bytes, statistics); the stream must end with its Adler-32.  Compared with zlib.decompress."""
    stream = bytes(stream)
    if len(stream) < 2:
        raise InflateError('no zlib header')
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8:
        raise InflateError('CM %d' % (cmf & 15))
    if cmf >> 4 > 7:
        raise InflateError('CINFO %d' % (cmf >> 4))
    if (cmf * 256 + flg) % 31:
        raise InflateError('FCHECK')
    if flg & 0x20:
        raise InflateError('FDICT')
    out, st, pos = inflate_raw(stream, 2)
    if len(stream) - pos < 4:
        raise InflateError('the input ends before the Adler-32')
    if struct.unpack('>I', stream[pos:pos + 4])[0] != (zlib.adler32(out) & 0xffffffff):
        raise InflateError('Adler-32')
    if len(stream) - pos > 4:
        raise InflateError('%d bytes after the Adler-32' % (len(stream) - pos - 4))
    assert out == zlib.decompress(stream), 'inflate_ref and zlib disagree'
    return out, st


# ---- a deflate bit writer for hand-made streams
def _rev(v, n):
    return int(format(v, '0%db' % n)[::-1], 2) if n else 0


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        """n bits of v, least significant first (headers, extra bits)."""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code, n):
        """A Huffman code of n bits, most significant first."""
        return self.bits(_rev(code, n), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def block(self, final, btype):
        return self.bits(final, 1).bits(btype, 2)

    def stored(self, data, final=0):
        self.block(final, 0).align()
        self.out += struct.pack('<HH', len(data), ~len(data) & 0xffff) + bytes(data)
        return self

    def fixed_symbol(self, s):
        if s < 144:
            return self.code(0x30 + s, 8)
        if s < 256:
            return self.code(0x190 + s - 144, 9)
        if s < 280:
            return self.code(s - 256, 7)
        return self.code(0xC0 + s - 280, 8)

    def fixed_match(self, length, dist):
        ls = max(k for k in range(29) if LENGTH_BASE[k] <= length and (k == 28) == (length == 258))
        self.fixed_symbol(257 + ls).bits(length - LENGTH_BASE[ls], LENGTH_EXTRA[ls])
        ds = max(k for k in range(30) if DIST_BASE[k] <= dist)
        return self.code(ds, 5).bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b'')


def zlib_wrap(deflate, data, cmf=0x78, flg=None):
    """RFC 1950 around a raw deflate stream that inflates to `data`."""
    if flg is None:
        flg = 31 - (cmf * 256) % 31 if (cmf * 256) % 31 else 0
    return bytes([cmf, flg]) + bytes(deflate) + struct.pack('>I', zlib.adler32(bytes(data)) & 0xffffffff)


# ---- a PNG chunk writer
def chunk(ctype, body=b''):
    body = bytes(body)
    return struct.pack('>I', len(body)) + ctype + body + struct.pack('>I', zlib.crc32(ctype + body) & 0xffffffff)


def ihdr(w, h, depth, colour, comp=0, filt=0, lace=0):
    return chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, colour, comp, filt, lace))


def png_file(w, h, depth, colour, stream, palette=None, cuts=None, before=(), between=(), after=()):
    """A file around the zlib stream `stream`: IHDR, the chunks `before`, PLTE (palette: bytes), IDAT chunks -- one, or cut at
    the byte positions `cuts` (equal neighbours give zero-length chunks) --, the chunks `after`, IEND.  `between`: chunks put
    between PLTE and the first IDAT."""
    stream = bytes(stream)
    edges = [0] + list(cuts or []) + [len(stream)]
    out = png_ref.SIGNATURE + ihdr(w, h, depth, colour) + b''.join(before)
    if palette is not None:
        out += chunk(b'PLTE', palette)
    out += b''.join(between)
    out += b''.join(chunk(b'IDAT', stream[a:b]) for a, b in zip(edges, edges[1:]))
    return out + b''.join(after) + chunk(b'IEND')


def split_chunks(data):
    """[(type, body)] without any check: for taking a good file apart."""
    pos, out = 8, []
    while pos + 12 <= len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        out.append((bytes(data[pos + 4:pos + 8]), bytes(data[pos + 8:pos + 8 + n])))
        pos += 12 + n
    return out


def join_chunks(cs):
    return png_ref.SIGNATURE + b''.join(chunk(t, b) for t, b in cs)


def idat_stream(data):
    return b''.join(b for t, b in split_chunks(data) if t == b'IDAT')


def with_stream(data, stream):
    """The file `data` with its IDAT chunks replaced by one that carries `stream`; every CRC correct."""
    cs, out, done = split_chunks(data), [], False
    for t, b in cs:
        if t == b'IDAT':
            if not done:
                out.append((t, bytes(stream)))
            done = True
        else:
            out.append((t, b))
    return join_chunks(out)


# ---- scanline filters, test side (PNG specification section 9.2)
def filter_rows(rows, types, bpp):
    """rows (H, row_bytes) uint8 and a filter type per row -> the filtered scanlines, filter bytes included."""
    rows = np.asarray(rows, np.uint8)
    H, rb = rows.shape
    out = bytearray()
    prev = [0] * rb
    for y in range(H):
        cur, ft, line = rows[y].tolist(), int(types[y]), []
        for x in range(rb):
            a = cur[x - bpp] if x >= bpp else 0
            b, c = prev[x], (prev[x - bpp] if x >= bpp else 0)
            pred = [0, a, b, (a + b) >> 1, png_ref._paeth(a, b, c)][ft]
            line.append((cur[x] - pred) & 255)
        out += bytes([ft]) + bytes(line)
        prev = cur
    return bytes(out)


def pack_rows(samples, depth):
    """(H, W) samples < 2^depth -> (H, ceil(W * depth / 8)) bytes, most significant bits first, the padding bits zero."""
    samples = np.asarray(samples, np.uint8)
    if depth == 8:
        return samples.copy()
    H, W = samples.shape
    per = 8 // depth
    padded = np.zeros((H, -(-W // per) * per), np.uint8)
    padded[:, :W] = samples
    out = np.zeros((H, padded.shape[1] // per), np.uint8)
    for k in range(per):
        out |= padded[:, k::per] << (8 - depth * (k + 1))
    return out


# ---- a strict reader for depths 1, 2, 4 and 8, colour types 0 and 3: the chunk rules of tests/png_ref.py, zlib's inflate
def parse_png_depths(data):
    """-> (samples (H,W) uint8 as stored, palette (n,3) uint8 or None, depth)."""
    data = bytes(data)
    cs = png_ref.chunks(data)
    types = [c[0] for c in cs]
    if types[0] != b'IHDR' or types.count(b'IHDR') != 1 or len(cs[0][1]) != 13:
        raise PngError('IHDR must come first, once, with 13 bytes')
    W, H, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', cs[0][1])
    if W < 1 or H < 1 or W > 0x7fffffff or H > 0x7fffffff:
        raise PngError('IHDR: %d x %d' % (W, H))
    if depth not in (1, 2, 4, 8) or colour not in (0, 3) or comp != 0 or filt != 0 or lace != 0:
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
        raise PngError('the deflate stream does not end with the IDAT data')
    rb = (W * depth + 7) // 8
    rows = png_ref_px.unfilter(raw, H, rb, 1)
    per = 8 // depth
    samples = np.zeros((H, rb * per), np.uint8)
    for k in range(per):
        samples[:, k::per] = (rows >> (8 - depth * (k + 1))) & ((1 << depth) - 1)
    samples = samples[:, :W].copy()
    if palette is not None and int(samples.max()) >= len(palette):
        raise PngError('index %d beyond a palette of %d' % (int(samples.max()), len(palette)))
    return samples, palette, depth
