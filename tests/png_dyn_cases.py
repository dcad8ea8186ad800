"""What tests/test_png_dyn_host.py and tests/test_gpu_png_dyn.py share: the truecolour contents, the host program
(tests/png_dyn_host.cpp) compiled and run, the strict check of one file, a plain heap Huffman, and the Fibonacci map."""
import heapq
import io as pyio
import os
import subprocess

import numpy as np
from PIL import Image

from tests import png_ref_px
from tests.test_gpu_png import make_map

HERE = os.path.dirname(os.path.abspath(__file__))
COLOUR_KINDS = ['constant', 'noise256', 'gradient', 'blend']
CODES = ['fixed', 'dynamic']
# IDAT bytes of the dynamic file of make_map('blobs', 480, 854, seed=0) over zlib.compress(scanlines, 6), measured with the
# host program (tests/test_png_dyn_host.py::test_blobs_map_against_zlib prints it; profiles/png_dynamic.json): 11660 / 10997.
# The encoder is integer code, so the device gives the same bytes; the test's bar is this plus 5 % for another zlib build.
BLOBS_IDAT_OVER_ZLIB6 = 1.0603


def make_picture(kind, H, W, seed=0):
    """(H,W,3) uint8: one colour; 256-value noise; a smooth gradient with +-2 noise; a gradient blended with the `blobs` mask."""
    rng = np.random.RandomState(seed)
    if kind == 'constant':
        return np.broadcast_to(np.array([10, 200, 77], np.uint8), (H, W, 3)).copy()
    if kind == 'noise256':
        return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    g = np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y) * 255 // max(W + H - 2, 1)], -1).astype(np.int64)
    if kind == 'gradient':
        return np.clip(g + rng.randint(-2, 3, g.shape), 0, 255).astype(np.uint8)
    if kind == 'blend':
        m = make_map('blobs', H, W, seed)
        colours = np.array([[0, 0, 0], [255, 0, 0], [0, 255, 0]], np.int64)
        return np.where(m[..., None] > 0, (6 * g + 4 * colours[m]) // 10, g).astype(np.uint8)
    raise KeyError(kind)


def picture_calls_of(shape):
    """As test_gpu_png.calls_of: every colour kind through a shape, a different one in each frame: [(kinds, pictures)]."""
    T, H, W = shape
    out = []
    for k0 in range(0, len(COLOUR_KINDS), T):
        kinds = [COLOUR_KINDS[(k0 + f) % len(COLOUR_KINDS)] for f in range(T)]
        out.append((kinds, np.stack([make_picture(k, H, W, seed=13 * k0 + f) for f, k in enumerate(kinds)])))
    return out


def fibonacci_map():
    """(1, 46365) uint8: byte value k in F(k + 2) places, k = 1..20 (F = 1, 1, 2, 3, ..), no two equal neighbours: the values go
    by falling count to the even places, then to the odd ones.  One scanline, one segment, no matches: the symbol histogram is
    the byte histogram plus ONE filter byte and ONE end-of-block symbol -- F(1) and F(2) -- so the 22 symbols together are the
    Fibonacci numbers F(1..22), every partial sum is below the next but one, and any Huffman tree over them is the chain of
    depth 21.  (Value k in F(k) places, k = 1..21, over 16 rows does not do it: with the 16 filter bytes and the end-of-block
    symbol counted the chain breaks at its foot and a heap Huffman stays at 14 bits.)"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    counts = fib[2:]                                  # of the values 1..20
    total = sum(counts)
    assert total == 46365 and max(counts) <= (total + 1) // 2
    values = np.concatenate([np.full(counts[k - 1], k, np.uint8) for k in range(20, 0, -1)])
    flat = np.empty(total, np.uint8)
    n_even = (total + 1) // 2
    flat[0::2] = values[:n_even]
    flat[1::2] = values[n_even:]
    m = flat.reshape(1, total)
    assert (m[:, 1:] != m[:, :-1]).all()
    return m


def huffman_depths(freq):
    """Plain heap Huffman: the code length of every symbol with freq > 0 (a single one gets 1); {symbol: length}."""
    heap = [(f, i, (i,)) for i, f in enumerate(freq) if f > 0]
    depth = {i: 0 for _f, i, _s in heap}
    if len(heap) == 1:
        return {heap[0][1]: 1}
    heapq.heapify(heap)
    while len(heap) > 1:
        fa, ia, sa = heapq.heappop(heap)
        fb, ib, sb = heapq.heappop(heap)
        for s in sa + sb:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, min(ia, ib), sa + sb))
    return depth


def compile_host(out_dir, name='png_dyn_host', extra=()):
    """tests/<name>.cpp as ordinary C++, the way tests/test_png_host.py compiles its program."""
    from swem_amd import build
    exe = os.path.join(str(out_dir), name + ('_san' if extra else ''))
    subprocess.run([build.HIPCC, '-x', 'c++', '-std=c++17', '-O1', *extra, '-I', build.CSRC, os.path.join(HERE, name + '.cpp'),
                    '-o', exe], check=True, capture_output=True, timeout=300)
    return exe


def run_host(exe, work_dir, pixels, codes, palette=None):
    """pixels (T,H,W) or (T,H,W,3) uint8 through the host program -> the T files as bytes."""
    T, H, W = pixels.shape[:3]
    channels = 3 if pixels.ndim == 4 else 1
    raw, pal, out = (os.path.join(str(work_dir), n) for n in ('px.raw', 'pal.raw', 'out'))
    np.ascontiguousarray(pixels).tofile(raw)
    if palette is not None:
        np.asarray(palette, np.uint8).tofile(pal)
    subprocess.run([exe, 'encode', raw, str(T), str(H), str(W), str(channels), pal if palette is not None else '-', codes, out],
                   check=True, timeout=300)
    files = []
    for t in range(T):
        with open('%s.%d.png' % (out, t), 'rb') as f:
            files.append(f.read())
    return files


def run_lengths(exe, freq, maxbits):
    r = subprocess.run([exe, 'lengths', str(maxbits)] + [str(int(f)) for f in freq], check=True, capture_output=True, timeout=60)
    return [int(v) for v in r.stdout.split()]


def check_file(data, want, palette=None):
    """One file through the strict reader and through PIL: the pixels (and the palette) that went in, byte for byte.  Returns
    the strict reader's sizes."""
    got, got_pal, n_idat, sizes, _filters = png_ref_px.parse_png(data)
    assert got.shape == want.shape and np.array_equal(got, want)
    rw = (3 * want.shape[1] if want.ndim == 3 else want.shape[1]) + 1
    assert sizes['raw'] == want.shape[0] * rw and n_idat >= 2
    img = Image.open(pyio.BytesIO(data))
    img.load()
    if want.ndim == 3:
        assert got_pal is None and img.mode == 'RGB'
    elif palette is None:
        assert got_pal is None and img.mode == 'L'
    else:
        pal = np.asarray(palette, np.uint8).reshape(256, 3)
        assert np.array_equal(got_pal, pal)
        assert img.mode == 'P' and np.array_equal(np.asarray(img.getpalette(), np.uint8).reshape(-1, 3), pal)
    assert np.array_equal(np.asarray(img), want)
    return sizes
