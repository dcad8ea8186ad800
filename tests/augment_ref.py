"""Not a test file: the numpy restatement of the device augmentation (swem_amd/csrc/augment.hip) that the
augmentation tests measure against -- geometry, cubic, regions, colour chain, mean, object choice -- in float64, or with
`dtype=np.float32` the same formulas in fp32 on the CPU (that run measures the tolerance of the device tests).

It follows the definition step by step (TPS -> affine -> crop / flip as a CHAIN on uncentred coordinates), not the composed and
centred matrices the host packs for the kernels: `augment.compose` / `augment.centred` are checked through it.  From
swem_amd.augment it takes only the parameter maths that tests/test_augment_host.py checks on its own: `inverse_affine` (M_aff)
and `tps_coefficients`, plus the anchor table.  Also here: the seeded inputs and parameter blocks the tests, the tolerance
measurement (tools/augment_parity.py) and the benchmark share.
"""
import numpy as np

from swem_amd import augment as A
from tests.io_ref import cubic_weights as _cubic_weights

EDGE = 1e-3        # px: a pixel whose float64 coordinate is this close to a threshold is excluded from the comparison
LABEL_VALUES = (0, 3, 7, 12, 255)


# ---------------------------------------------------------------------------------------------------------------- geometry
def geometry(clip, fr, dtype=np.float64):
    """Steps 1-3 for every output pixel: dict of (Ho, Wo) arrays u, v, xa, ya, sx, sy in `dtype`, bools outside, fill."""
    f = dtype
    Ho, Wo = clip['out_hw']
    i = np.arange(Wo, dtype=f)[None, :] + np.zeros((Ho, 1), f)
    j = np.arange(Ho, dtype=f)[:, None] + np.zeros((1, Wo), f)
    if fr.get('tps_on', False):
        Aff, W = A.tps_coefficients(fr['tps_Y'])
        Aff, W, X = Aff.astype(f), W.astype(f), A.TPS_ANCHORS.astype(f)
        xn = f(-1) + f(2) * i / f(Wo - 1)
        yn = f(-1) + f(2) * j / f(Ho - 1)
        qx = Aff[0, 0] + Aff[1, 0] * xn + Aff[2, 0] * yn
        qy = Aff[0, 1] + Aff[1, 1] * xn + Aff[2, 1] * yn
        for k in range(16):
            d = (xn - X[k, 0]) ** 2 + (yn - X[k, 1]) ** 2
            U = d * np.log(d + f(1e-9))
            qx = qx + W[k, 0] * U
            qy = qy + W[k, 1] * U
        u = ((qx + f(1)) * f(Wo) - f(1)) / f(2)
        v = ((qy + f(1)) * f(Ho) - f(1)) / f(2)
    else:
        u, v = i, j
    outside = (u <= -1) | (u >= Wo) | (v <= -1) | (v >= Ho)
    M = (np.asarray(fr['M_aff'], np.float64) if 'M_aff' in fr else
         A.inverse_affine(fr.get('angle', 0.0), fr.get('shear', 0.0), clip['out_hw'])).astype(f)
    x, y = u + f(0.5), v + f(0.5)
    xa = M[0, 0] * x + M[0, 1] * y + M[0, 2]
    ya = M[1, 0] * x + M[1, 1] * y + M[1, 2]
    fill = (xa < 0) | (xa >= Wo) | (ya < 0) | (ya >= Ho)
    top, left, ch, cw = [f(t) for t in clip['crop']]
    sx = left + ((f(Wo) - xa) if clip['flip'] else xa) * cw / f(Wo)
    sy = top + ya * ch / f(Ho)
    return dict(u=u, v=v, xa=xa, ya=ya, sx=sx, sy=sy, outside=outside, fill=fill)


def near_threshold(g, out_hw, edge=EDGE):
    """The exclusion set of a float64 geometry: u, v within `edge` of -1 / Wo / Ho, x', y' of 0 / Wo / Ho, sx, sy of an integer."""
    Ho, Wo = out_hw
    near = np.zeros(g['u'].shape, bool)
    for a, lims in ((g['u'], (-1, Wo)), (g['v'], (-1, Ho)), (g['xa'], (0, Wo)), (g['ya'], (0, Ho))):
        for lim in lims:
            near |= np.abs(a - lim) < edge
    for a in (g['sx'], g['sy']):
        near |= np.abs(a - np.round(a)) < edge
    return near


# ---------------------------------------------------------------------------------------------------------------- sampling
def sample(src, lab, g, dtype=np.float64):
    """Step 4: (img (3,Ho,Wo) before any colour op, label (Ho,Wo) uint8, region (Ho,Wo) uint8)."""
    f = dtype
    Hs, Ws = lab.shape
    region = np.where(g['outside'], A.REGION_OUTSIDE_TPS, np.where(g['fill'], A.REGION_FILL, A.REGION_IMAGE)).astype(np.uint8)
    ly = np.clip(np.floor(g['sy']), 0, Hs - 1).astype(np.int64)
    lx = np.clip(np.floor(g['sx']), 0, Ws - 1).astype(np.int64)
    label = np.where(region == A.REGION_IMAGE, lab[ly, lx], 0).astype(np.uint8)
    S = src.astype(f) / f(255)
    bx, by = g['sx'] - f(0.5), g['sy'] - f(0.5)
    fx, fy = np.floor(bx), np.floor(by)
    wx, wy = _cubic_weights(bx - fx, f), _cubic_weights(by - fy, f)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    img = np.zeros(g['u'].shape + (3,), f)
    for a in range(4):
        yy = np.clip(iy - 1 + a, 0, Hs - 1)
        row = np.zeros_like(img)
        for q in range(4):
            xx = np.clip(ix - 1 + q, 0, Ws - 1)
            row = row + wx[q][..., None] * S[yy, xx]
        img = img + wy[a][..., None] * row
    fillc = np.array(A.IM_MEAN, f) / f(255)
    img = np.where((region == A.REGION_IMAGE)[..., None], img, np.where((region == A.REGION_FILL)[..., None], fillc, f(0)))
    return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(f), label, region


# ------------------------------------------------------------------------------------------------------------------ colour
def gray(x, f):
    return f(0.299) * x[0] + f(0.587) * x[1] + f(0.114) * x[2]


def jitter(x, factors, order, m, f):
    """x (3, ...) through the ops of `order` (torchvision's tensor semantics on floats in [0,1]); m: the contrast mean."""
    for op in order:
        if op == A.NO_OP:
            continue
        fac = f(factors[op])
        if op == A.BRIGHTNESS:
            x = np.clip(fac * x, 0, 1)
        elif op == A.CONTRAST:
            x = np.clip(fac * x + (f(1) - fac) * m, 0, 1)
        else:
            x = np.clip(fac * x + (f(1) - fac) * gray(x, f)[None], 0, 1)
    return x.astype(f)


def colour(img, region, clip, fr, dtype=np.float64):
    """The colour chain on a warped frame (3,Ho,Wo): the clip-level ops and grayscale on image pixels, the frame-level ops on
    image and fill pixels, nothing on outside-TPS pixels; one gray mean, taken before any op, for both contrast ops."""
    f = dtype
    m = f(gray(img, f).mean(dtype=f))
    none, one = (A.NO_OP,) * 3, (1.0, 1.0, 1.0)
    x = jitter(img, clip.get('factors', one), clip.get('order', none), m, f)
    if clip.get('gray', False):
        x = np.repeat(gray(x, f)[None], 3, axis=0)
    x = jitter(x, fr.get('factors', one), fr.get('order', none), m, f)
    y = jitter(img, fr.get('factors', one), fr.get('order', none), m, f)        # fill pixels: frame-level ops only
    return np.where(region[None] == A.REGION_IMAGE, x, np.where(region[None] == A.REGION_FILL, y, f(0))).astype(f), m


# ----------------------------------------------------------------------------------------------------------------- objects
def choose(label0, prio, max_nobj):
    """(chosen labels in priority order, number found, presence (256,) bool) from the warped label of frame 0."""
    present = np.zeros(256, bool)
    present[np.unique(label0)] = True
    present[0] = present[255] = False
    cand = sorted(np.nonzero(present)[0].tolist(), key=lambda l: int(prio[l]))
    return cand[:max_nobj], len(cand), present


def augment_clip(src, lab, clip, max_nobj, dtype=np.float64):
    """One clip: src (T,Hs,Ws,3) uint8, lab (T,Hs,Ws) uint8 -> dict of frames (T,3,Ho,Wo), masks (T,N+1,Ho,Wo), valid (N+1,),
    label (T,Ho,Wo) int64, found, wlabel, region (T,Ho,Wo) uint8, presence (256,), pre (the frames before colour), mean (T,),
    exclude (T,Ho,Wo) bool (the exclusion set of THIS dtype's geometry: meaningful for float64)."""
    T = lab.shape[0]
    out = {k: [] for k in ('frames', 'wlabel', 'region', 'pre', 'mean', 'exclude')}
    for t in range(T):
        fr = clip['frames'][t]
        g = geometry(clip, fr, dtype)
        img, wl, reg = sample(src[t], lab[t], g, dtype)
        col, m = colour(img, reg, clip, fr, dtype)
        for k, v in zip(('frames', 'wlabel', 'region', 'pre', 'mean', 'exclude'),
                        (col, wl, reg, img, m, near_threshold(g, clip['out_hw']))):
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    chosen, found, present = choose(out['wlabel'][0], clip.get('prio', np.arange(256)), max_nobj)
    fg = np.stack([(out['wlabel'] == chosen[o]) if o < len(chosen) else np.zeros(out['wlabel'].shape, bool)
                   for o in range(max_nobj)], axis=1)
    masks = np.concatenate([(1 - fg.sum(1, keepdims=True)), fg], axis=1).astype(np.float32)
    n = max(len(chosen), 1)
    out.update(masks=masks, label=masks.argmax(1).astype(np.int64), found=found, presence=present, chosen=chosen,
               valid=np.array([1.0] * (n + 1) + [0.0] * (max_nobj - n), np.float32))
    return out


def augment(src, lab, clips, max_nobj, dtype=np.float64):
    """A batch: the per-clip dicts of `augment_clip` stacked on a leading B axis."""
    outs = [augment_clip(src[b], lab[b], clips[b], max_nobj, dtype) for b in range(len(clips))]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0] if k != 'chosen'}


# ---------------------------------------------------------------------------------------- shared inputs of tests and tools
def block_labels(rng, shape, cell, values=LABEL_VALUES):
    """uint8 label maps (..., H, W) of constant blocks, each at least `cell` >= 6 pixels on a side (the last block of a row or
    column takes the remainder), values drawn from `values`."""
    *lead, H, W = shape

    def sizes(n):
        k = max(n // cell, 1)
        return [cell] * (k - 1) + [n - cell * (k - 1)]
    hs, ws = sizes(H), sizes(W)
    coarse = rng.choice(np.array(values, np.uint8), size=tuple(lead) + (len(hs), len(ws)))
    return np.repeat(np.repeat(coarse, hs, axis=-2), ws, axis=-1)


def make_inputs(seed, B, T, src_hw, cell=6, values=LABEL_VALUES):
    """White-noise uint8 frames (B,T,Hs,Ws,3) -- the worst gradient -- and block label maps (B,T,Hs,Ws)."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, size=(B, T) + tuple(src_hw) + (3,), dtype=np.uint8)
    return src, block_labels(rng, (B, T) + tuple(src_hw), cell, values)


# name -> (seed, B, T, source size, output size, label block size).  The seeds are chosen on the float64 restatement alone: the
# exclusion set stays under 3 % of the pixels (asserted by the tests).
CASES = {
    'small_24x40': (1, 2, 3, (37, 53), (24, 40), 6),
    'small_17x23': (2, 2, 3, (37, 53), (17, 23), 6),
    'full_384': (3, 1, 3, (480, 854), (384, 384), 24),
}
MAX_NOBJ = 2
EXCLUSION_CAP = 0.03


def drawn_case(name):
    """(src, lab, clips) of a parity case: inputs and a different drawn parameter block per clip and frame."""
    seed, B, T, src_hw, out_hw, cell = CASES[name]
    src, lab = make_inputs(seed, B, T, src_hw, cell)
    rng = np.random.default_rng(1000 + seed)
    return src, lab, [A.draw_params(rng, T, src_hw, out_hw) for _ in range(B)]


def measure_bar(name):
    """The fp32-against-float64 maximum of the restatement on a case's own inputs, outside the exclusion set, and the bar (4x: FMA
    contraction and another summation order of the 16 taps and 16 TPS terms change roundings, not magnitudes)."""
    src, lab, clips = drawn_case(name)
    r64 = augment(src, lab, clips, MAX_NOBJ, np.float64)
    r32 = augment(src, lab, clips, MAX_NOBJ, np.float32)
    keep = ~r64['exclude']
    err = np.abs(r32['frames'].astype(np.float64) - r64['frames']).max(axis=2)
    lab_diff = int(((r32['wlabel'] != r64['wlabel']) | (r32['region'] != r64['region']))[keep].sum())
    m = float(err[keep].max())
    return {'fp32_vs_fp64_max': m, 'bar': 4.0 * m, 'excluded_fraction': float(r64['exclude'].mean()),
            'excluded_fraction_max_per_frame': float(r64['exclude'].mean(axis=(2, 3)).max()),
            'label_or_region_differences_outside': lab_diff}
