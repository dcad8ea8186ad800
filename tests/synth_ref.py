"""Not a test file: the numpy restatement of the stage-0 path (swem_amd/csrc/synth.hip and the static form of
swem_amd/csrc/augment.hip) that the synthesis tests measure against -- foreground statistics, placement, compositing, the static
geometric chain, the hue op -- in float64, or with `dtype=np.float32` the same formulas in fp32 on the CPU (that run measures the
tolerance of the device tests).

Like tests/augment_ref.py, from which it takes the cubic, the sampler, the three jitter ops and the object choice, it follows the
definition step by step on uncentred coordinates and never touches the packed matrices: `augment.static_frame_matrices` and
`augment.pack_static_params` are checked through it.  Compositing pastes whole resized objects in paste order, as the reference
does; the kernel walks the objects backwards per pixel.  Also here: the seeded inputs and cases the tests and tools share.
"""
import numpy as np

from swem_amd import augment as A
from tests import augment_ref as R

EDGE = R.EDGE            # px / colour steps: closer than this to a threshold is excluded from the comparison
HALF_MARGIN = 1e-6       # no float64 object size may lie this close to a half-integer
SLOT_HW = (48, 56)
MASK_VALUES = (0, 0, 1, 200)     # foreground is != 0


# ------------------------------------------------------------------------------------------------------------ statistics
def foreground_stats(img, mask):
    """dict(count, box=(hmin, wmin, hmax + 1, wmax + 1) or None, sums (3,) int64) of the pixels with mask != 0."""
    fg = mask != 0
    if not fg.any():
        return {'count': 0, 'box': None, 'sums': np.zeros(3, np.int64)}
    ys, xs = np.nonzero(fg)
    return {'count': int(fg.sum()), 'box': (int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1),
            'sums': img[fg].astype(np.int64).sum(axis=0)}


# -------------------------------------------------------------------------------------------------------------- placement
def place(clip, fr, stats):
    """random_resize and place_object (static_dataset.py:43-79) for every object of one frame, float64 on the drawn fp32 numbers:
    (rows of (rh, rw, tx, ty, id, present), the unrounded sizes)."""
    h0, w0 = clip['sizes'][0]
    ids = clip.get('ids', list(range(1, len(clip['sizes']) + 1)))
    rows, raw = [], []
    for k, st in enumerate(stats):
        if st['count'] == 0:
            rows.append((0, 0, 0, 0, int(ids[k]) & 255, 0))
            continue
        area, aspect, ux, uy = [np.float64(np.float32(v)) for v in np.asarray(fr['objects'])[k]]
        hc, wc = st['box'][2] - st['box'][0], st['box'][3] - st['box'][1]
        fh, fw = np.sqrt(area * hc * wc / aspect), np.sqrt(area * hc * wc * aspect)
        raw += [fh, fw]
        rh, rw = max(1, int(np.rint(fh))), max(1, int(np.rint(fw)))

        def centre(u, size, full):
            lo, hi = size // 2, max(full - size // 2, size // 2)
            return lo + min(hi - lo, int(np.floor(u * (hi - lo + 1))))
        tx, ty = centre(ux, rw, w0) - rw // 2, centre(uy, rh, h0) - rh // 2
        rows.append((rh, rw, tx, ty, int(ids[k]) & 255, 1))
    return rows, raw


def resize_object(img, mask, rh, rw, dtype=np.float64):
    """The boxed object (hc, wc, 3) uint8 / (hc, wc) uint8 at (rh, rw): colour (rh, rw, 3) in `dtype` on the 0..255 scale by the
    project's cubic at ((d + 0.5) size / r - 0.5), taps clamped to the box; mask (rh, rw) by nearest at min(floor(d size / r),
    size - 1)."""
    f = dtype
    hc, wc = mask.shape

    def axis(n, r):
        d = np.arange(r, dtype=np.float64)
        near = np.minimum(np.floor(d * n / r), n - 1).astype(np.int64)
        b = ((d + 0.5) * n / r - 0.5).astype(f)
        fl = np.floor(b)
        taps = [np.clip(fl.astype(np.int64) - 1 + q, 0, n - 1) for q in range(4)]
        return near, taps, R._cubic_weights(b - fl, f)
    ny, ty, wy = axis(hc, rh)
    nx, tx, wx = axis(wc, rw)
    S = img.astype(f)
    col = np.zeros((rh, rw, 3), f)
    for a in range(4):
        row = np.zeros((rh, rw, 3), f)
        for q in range(4):
            row = row + wx[q][None, :, None] * S[ty[a]][:, tx[q]]
        col = col + wy[a][:, None, None] * row
    return col.astype(f), mask[ny][:, nx]


# ------------------------------------------------------------------------------------------------------------ compositing
def composite(imgs, masks, clip, dtype=np.float64):
    """synthesis_frames: imgs / masks lists of the n_img real-size arrays.  dict of frames (T,h0,w0,3) uint8, labels (T,h0,w0)
    uint8, exclude (T,h0,w0) bool (a colour within EDGE of k + 0.5), stats, plan (T,n_img,6), raw_sizes, value (the unrounded
    colours)."""
    f = dtype
    n_img, T = len(imgs), len(clip['frames'])
    h0, w0 = masks[0].shape
    stats = [foreground_stats(i, m) for i, m in zip(imgs, masks)]
    if n_img == 1:
        return {'frames': np.stack([imgs[0]] * T), 'labels': np.stack([masks[0]] * T), 'exclude': np.zeros((T, h0, w0), bool),
                'stats': stats, 'plan': None, 'raw_sizes': [], 'value': np.stack([imgs[0].astype(f)] * T)}
    mean_fg = stats[0]['sums'].astype(np.float64) / (stats[0]['count'] + 1e-8)
    out = {k: [] for k in ('frames', 'labels', 'exclude', 'plan', 'value')}
    raw_sizes = []
    for fr in clip['frames']:
        rows, raw = place(clip, fr, stats)
        raw_sizes += raw
        canvas = imgs[0].astype(f)
        canvas[masks[0] != 0] = mean_fg.astype(f)
        label = np.zeros((h0, w0), np.uint8)
        for k in fr.get('paste', range(n_img)):
            rh, rw, tx, ty, ident, present = rows[k]
            if not present:
                continue
            y0, x0, y1, x1 = stats[k]['box']
            col, m = resize_object(imgs[k][y0:y1, x0:x1], masks[k][y0:y1, x0:x1], rh, rw, f)
            hv, wv = min(rh, h0 - ty), min(rw, w0 - tx)
            if hv <= 0 or wv <= 0:
                continue
            hit = m[:hv, :wv] != 0
            canvas[ty:ty + hv, tx:tx + wv][hit] = col[:hv, :wv][hit]
            label[ty:ty + hv, tx:tx + wv][hit] = ident
        v64 = canvas.astype(np.float64)
        out['value'].append(canvas)
        out['frames'].append(np.floor(np.clip(v64, 0, 255) + 0.5).astype(np.uint8))
        out['labels'].append(label)
        out['exclude'].append((np.abs(v64 - np.floor(v64) - 0.5) < EDGE).any(axis=-1))
        out['plan'].append(np.array(rows, np.int64))
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(stats=stats, raw_sizes=raw_sizes)
    return res


def stats_table(stats, N):
    """(N, 8) int64 as StaticClipSynthesizer.stats gives it; the box of an empty mask is left 0 (compare it where count > 0)."""
    tab = np.zeros((N, 8), np.int64)
    for k, st in enumerate(stats):
        tab[k, 4] = st['count']
        tab[k, 5:] = st['sums']
        if st['box'] is not None:
            tab[k, :4] = st['box']
    return tab


# ------------------------------------------------------------------------------------------------------------- the hue op
def hue(x, shift, dtype=np.float64):
    """torchvision's adjust_hue on floats in [0,1], x (3, ...): the vector form of colorsys."""
    f = dtype
    r, g, b = [c.astype(f) for c in x]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    eqc = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eqc, f(1), maxc)
    crd = np.where(eqc, f(1), cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, f(2) + rc - bc, f(4) + gc - rc))
    h = np.fmod(h / f(6) + f(1), f(1))
    h = np.fmod(h + f(shift) + f(1), f(1))
    h6 = h * f(6)
    fi = np.floor(h6)
    fr = h6 - fi
    i = fi.astype(np.int64) % 6
    v = maxc
    p = np.clip(v * (f(1) - s), 0, 1)
    q = np.clip(v * (f(1) - s * fr), 0, 1)
    t = np.clip(v * (f(1) - s * (f(1) - fr)), 0, 1)
    out = np.stack([np.choose(i, [v, q, p, p, t, v]), np.choose(i, [t, v, v, q, p, p]), np.choose(i, [p, p, t, v, v, q])])
    return out.astype(f)


# ------------------------------------------------------------------------------------------------------- the static chain
def static_geometry(clip, fr, dtype=np.float64):
    """Steps 1-5 of DESIGN.md section 9 for every output pixel: u, v, px, py (before the flip), sx, sy in `dtype`; bools
    outside, fill1 (outside image 0 after the frame-level affine), fill2 (outside the source after the clip-level scale)."""
    f = dtype
    Ho, Wo = clip['out_hw']
    h0, w0 = clip['sizes'][0]
    g = R.geometry({'out_hw': (Ho, Wo), 'crop': (0, 0, Ho, Wo), 'flip': False},
                   {k: fr[k] for k in ('tps_on', 'tps_Y') if k in fr}, f)
    u, v = g['u'], g['v']
    r = f(A.static_scale(clip['sizes'][0], clip['out_hw']))
    cx = (u + f(0.5) + f(fr.get('left', 0))) / r
    cy = (v + f(0.5) + f(fr.get('top', 0))) / r
    inv = A.inverse_affine(fr.get('angle', 0.0), fr.get('shear', 0.0), (h0, w0)).astype(f)
    qx = inv[0, 0] * cx + inv[0, 1] * cy + inv[0, 2]
    qy = inv[1, 0] * cx + inv[1, 1] * cy + inv[1, 2]
    ctr_x, ctr_y, s2, s1 = f(w0 / 2.0), f(h0 / 2.0), f(fr.get('s2', 1.0)), f(clip.get('s1', 1.0))
    px = ctr_x + (qx - ctr_x) / s2
    py = ctr_y + (qy - ctr_y) / s2
    fill1 = (px < 0) | (px >= w0) | (py < 0) | (py >= h0)
    fx = (f(w0) - px) if clip.get('flip', False) else px
    sx = ctr_x + (fx - ctr_x) / s1
    sy = ctr_y + (py - ctr_y) / s1
    fill2 = (sx < 0) | (sx >= w0) | (sy < 0) | (sy >= h0)
    if not clip.get('src_fill', True):
        fill2 = np.zeros_like(fill2)
    return dict(u=u, v=v, px=px, py=py, sx=sx, sy=sy, outside=g['outside'], fill1=fill1, fill2=fill2, fill=fill1 | fill2)


def near_threshold(g, clip, edge=EDGE):
    """Section 8's exclusion set for the static chain: u, v within `edge` of -1 / Wo / Ho, (px, py) of image 0's borders,
    sx, sy of an integer (the source's borders are integers)."""
    Ho, Wo = clip['out_hw']
    h0, w0 = clip['sizes'][0]
    near = np.zeros(g['u'].shape, bool)
    for a, lims in ((g['u'], (-1, Wo)), (g['v'], (-1, Ho)), (g['px'], (0, w0)), (g['py'], (0, h0))):
        for lim in lims:
            near |= np.abs(a - lim) < edge
    for a in (g['sx'], g['sy']):
        near |= np.abs(a - np.round(a)) < edge
    return near


def colour(img, region, clip, fr, dtype=np.float64):
    """Section 9's colour chain: the clip-level jitter's four ops (`hue_before` of the three, the hue op, the rest), the
    grayscale, the frame-level ops; fill pixels take the frame-level ops only, outside-TPS pixels none; one gray mean."""
    f = dtype
    m = f(R.gray(img, f).mean(dtype=f))
    none, one = (A.NO_OP,) * 3, (1.0, 1.0, 1.0)
    order, fac = tuple(clip.get('order', none)), clip.get('factors', one)
    shift = float(np.float32(clip.get('hue', 0.0)))
    if shift != 0.0:
        nb = int(clip.get('hue_before', 0))
        x = R.jitter(img, fac, order[:nb], m, f)
        x = hue(x, shift, f)
        x = R.jitter(x, fac, order[nb:], m, f)
    else:
        x = R.jitter(img, fac, order, m, f)
    if clip.get('gray', False):
        x = np.repeat(R.gray(x, f)[None], 3, axis=0)
    x = R.jitter(x, fr.get('factors', one), fr.get('order', none), m, f)
    y = R.jitter(img, fr.get('factors', one), fr.get('order', none), m, f)
    return np.where(region[None] == A.REGION_IMAGE, x, np.where(region[None] == A.REGION_FILL, y, f(0))).astype(f), m


def static_chain(comp, comp_lab, clip, max_nobj, dtype=np.float64):
    """The static chain on one clip's composites (T,h0,w0,3) / (T,h0,w0) uint8: augment_ref.augment_clip's dict, plus fill1, fill2."""
    keys = ('frames', 'wlabel', 'region', 'pre', 'mean', 'exclude', 'fill1', 'fill2')
    out = {k: [] for k in keys}
    for t, fr in enumerate(clip['frames']):
        g = static_geometry(clip, fr, dtype)
        img, wl, reg = R.sample(comp[t], comp_lab[t], g, dtype)
        col, m = colour(img, reg, clip, fr, dtype)
        for k, v in zip(keys, (col, wl, reg, img, m, near_threshold(g, clip), g['fill1'], g['fill2'])):
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    chosen, found, present = R.choose(out['wlabel'][0], clip.get('prio', np.arange(256)), max_nobj)
    fg = np.stack([(out['wlabel'] == chosen[o]) if o < len(chosen) else np.zeros(out['wlabel'].shape, bool)
                   for o in range(max_nobj)], axis=1)
    masks = np.concatenate([(1 - fg.sum(1, keepdims=True)), fg], axis=1).astype(np.float32)
    n = max(len(chosen), 1)
    out.update(masks=masks, label=masks.argmax(1).astype(np.int64), found=found, presence=present,
               valid=np.array([1.0] * (n + 1) + [0.0] * (max_nobj - n), np.float32))
    return out


def static_batch(comps, comp_labs, clips, max_nobj, dtype=np.float64):
    """A batch of `static_chain`: comps / comp_labs are slot arrays (B,T,Hmax,Wmax[,3]) or lists of real-size arrays."""
    outs = []
    for b, clip in enumerate(clips):
        h0, w0 = clip['sizes'][0]
        outs.append(static_chain(np.asarray(comps[b])[:, :h0, :w0], np.asarray(comp_labs[b])[:, :h0, :w0], clip, max_nobj, dtype))
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}


# ---------------------------------------------------------------------------------------- shared inputs of tests and tools
def make_slots(seed, sizes_per_clip, N, slot_hw=SLOT_HW, cell=6, values=MASK_VALUES):
    """White-noise images (B,N,Hmax,Wmax,3) and block masks (B,N,Hmax,Wmax) uint8, each at the top left of its slot; every byte
    outside a real size (unused slots included) is 0xFF, so that a read past it shows."""
    rng = np.random.default_rng(seed)
    B = len(sizes_per_clip)
    imgs = np.full((B, N) + tuple(slot_hw) + (3,), 0xFF, np.uint8)
    masks = np.full((B, N) + tuple(slot_hw), 0xFF, np.uint8)
    for b, sizes in enumerate(sizes_per_clip):
        for k, (h, w) in enumerate(sizes):
            imgs[b, k, :h, :w] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
            masks[b, k, :h, :w] = R.block_labels(rng, (h, w), cell, values)
    return imgs, masks


def unslot(imgs, masks, b, sizes):
    return ([imgs[b, k, :h, :w] for k, (h, w) in enumerate(sizes)], [masks[b, k, :h, :w] for k, (h, w) in enumerate(sizes)])


# name -> (seed, N, output size, the image sizes of each clip).  The seeds are chosen on the float64 restatement alone: no object
# size within 1e-6 of a half-integer, the exclusion sets under 3 % of a frame (tests/test_synth_host.py asserts both).
CASES = {
    'n2_24x40': (1, 2, (24, 40), [[(37, 53), (29, 41)], [(45, 33), (37, 53)]]),
    'n3_17x23': (2, 3, (17, 23), [[(29, 41), (45, 33), (37, 53)], [(37, 53), (29, 41)]]),
}
T = 3
EXCLUSION_CAP = R.EXCLUSION_CAP


def drawn_case(name):
    """(imgs, masks, clips) of a parity case: slots and one drawn parameter set per clip."""
    seed, N, out_hw, sizes = CASES[name]
    imgs, masks = make_slots(seed, sizes, N)
    rng = np.random.default_rng(2000 + seed)
    return imgs, masks, [A.draw_static_params(rng, T, s, out_hw) for s in sizes]


def composite_case(imgs, masks, clips, dtype=np.float64):
    """`composite` of every clip of a batch in slots."""
    return [composite(*unslot(imgs, masks, b, clip['sizes']), clip, dtype) for b, clip in enumerate(clips)]


def measure_bar(name):
    """The fp32-against-float64 maximum of the static chain's restatement on a case's own inputs (the float64 composites),
    outside the exclusion set, and the bar: 4x (tests/augment_ref.py: measure_bar)."""
    imgs, masks, clips = drawn_case(name)
    N = CASES[name][1]
    comp = composite_case(imgs, masks, clips)
    fr, lb = [c['frames'] for c in comp], [c['labels'] for c in comp]
    r64, r32 = static_batch(fr, lb, clips, N, np.float64), static_batch(fr, lb, clips, N, np.float32)
    keep = ~r64['exclude']
    err = np.abs(r32['frames'].astype(np.float64) - r64['frames']).max(axis=2)
    m = float(err[keep].max())
    raw = np.array([v for c in comp for v in c['raw_sizes']])
    return {'fp32_vs_fp64_max': m, 'bar': 4.0 * m,
            'excluded_fraction_max_per_frame': float(r64['exclude'].mean(axis=(2, 3)).max()),
            'composite_excluded_fraction_max_per_frame': float(max(c['exclude'].mean(axis=(1, 2)).max() for c in comp)),
            'label_or_region_differences_outside': int(((r32['wlabel'] != r64['wlabel']) | (r32['region'] != r64['region']))[keep].sum()),
            'half_integer_margin': float(np.abs(raw - np.floor(raw) - 0.5).min())}
