"""GPU: the convolution data gradient (SWEM_CONV_DGRAD in csrc/conv_f32.hip, conv_presplit.hip, conv_t256.hip; tap_coord in
conv_common.h) against float64, element by element, off the shapes the shipped plans hold it to.  Every stride-2 data-gradient
entry of the training plan files has EH = EW = 1 (the 384 crops are even) and none carries a mask; an odd forward size under
stride 2 (EH or EW = 0) has only ever run on the exact fp32 kernels.  The pre-split kernels and the 256-column kernel replace
tap_coord by "pixel of tap (0, 0) minus (ky >> s) W + (kx >> s)": DCASES gives them every parity of the forward size, stride 2
together with SWEM_CONV_MASK_POS, a ragged column tile, 1x1 stride 2 without padding (one input pixel in four receives
anything), the 49 taps of a stem, and fewer rows per image than one tile -- B = 3 throughout, so that row tiles straddle images.

The call is autograd._Conv.backward's: ops.conv2d([dY], transposed-filter ConvPack with fast16, dgrad=(H, W), mask=, plan=) with
dY marked `_swem_grad`.  Plan forms (FORMS, read at import time from the three shipped plan files): every distinct (tile, plan
bits 20-23, arithmetic) that occurs on an entry with the DGRAD flag plus the plain heuristic word of each arithmetic (m << 16),
each with K-split 1 and 3 (a word that names no tile leaves the K-split to the library and runs once).  ops.MATH_RAN must report
the plan's own arithmetic (a silent fallback fails), ops.check_faults() follows every launch; a form the library refuses for a
shape (SwemHipError at the call) is listed in the output as skipped, and every geometry must still run on at least one form of
each of fp32, bf16x6, bf16 and f16x3.

The bar, per element, is test_shipped_conv_plan's:  |dX - ref| <= c * bnd + 1e-30,  ref = torch.nn.grad.conv2d_input in float64
(for plain bf16 on the bf16-rounded operands), bnd = the same on |dY|, |w|, c = C_ARITH of the arithmetic; both are zero wherever
mask <= 0, and there the result must be exactly zero (masks hold positive and negative values, +0.0 and -0.0).  The sensitivity
reference is the float64 result without one 32-channel block of dY over ALL taps (under stride 2 a single tap reaches a quarter
of the pixels): it must break the same bar on >= 1 % of the elements that have a valid tap.

test_standin_dgrad (no GPU) runs the same cases and checks with fp32 torch on the CPU in the kernel's place: at least 4x under
the bar, else the case's bar is 8x what the stand-in measures on that case (Sweep.add(standin=)).  Measured on the CPU, largest
|dX - ref| / bar: bf16 0.12, f16x3 0.14, fp32 / bf16x6 0.18 - 0.24 on the stride-2 cases (sums of 36 - 400 products over
up to 37 thousand elements) and 0.29 on s2_even_odd, which therefore gets the 8x rule on those two arithmetics.  What the bar
is worth (test_standin_with_a_dropped_element_misses_the_bars): the float64 reference of `s2_odd_odd` without tap (1, 1)
misses the fp32 / bf16x6 / bf16 bar by up to 6.2e5x and the f16x3 bar by up to 3.1e5x on the elements that tap reaches (13.3 %
of dX: one pixel in four, about half of them masked), 100 % of which break it.

What the kernels measure is printed and recorded under dgrad_edges/<arithmetic> (helpers.record_parity) before anything is asserted.
On an MI355X, largest |dX - ref| / bnd over all geometries and the 20 forms (36 launches per geometry, none refused): fp32 3.1e-7,
bf16x6 2.0e-7, bf16 1.0e-7 (c = 9.5e-7), f16x3 1.9e-7 (c = 1.9e-6)."""
import functools
import zlib

import pytest
import torch

from swem_amd import _lib, ops
from tests import helpers as H
from tests import test_gpu_shipped_plans as SP
from tests.test_gpu_shipped_plans import C_ARITH, MATH_NAME
from tests.test_gpu_train_edges import Sweep

gpu = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
UNIT = {'bar': 1.0}                       # every value is recorded as a fraction of its element's own bar
B = 3

# id -> forward Cin, Cout, k, stride, pad, forward H x W, mask
DCASES = {
    's2_even_odd': dict(cin=96, cout=160, k=3, s=2, pad=1, hw=(10, 13), mask=False),
    's2_odd_even': dict(cin=96, cout=160, k=3, s=2, pad=1, hw=(13, 10), mask=False),
    's2_odd_odd': dict(cin=32, cout=64, k=3, s=2, pad=1, hw=(9, 11), mask=True),
    's2_even_mask': dict(cin=32, cout=64, k=3, s=2, pad=1, hw=(10, 12), mask=True),
    'p0_s2_9x12': dict(cin=64, cout=128, k=1, s=2, pad=0, hw=(9, 12), mask=False),
    'p0_s2_12x9': dict(cin=64, cout=128, k=1, s=2, pad=0, hw=(12, 9), mask=False),
    'stem_s2': dict(cin=32, cout=64, k=7, s=2, pad=3, hw=(14, 11), mask=False),
    's1_mask': dict(cin=64, cout=96, k=3, s=1, pad=1, hw=(7, 5), mask=True),
}


def geom(c):
    """dY is (B, Ho, Wo, Cout); eh / ew = rows / columns of the forward input the strided filter never reached."""
    (Hh, Ww), k, s, pad = c['hw'], c['k'], c['s'], c['pad']
    Ho, Wo = (Hh + 2 * pad - k) // s + 1, (Ww + 2 * pad - k) // s + 1
    return dict(H=Hh, W=Ww, Ho=Ho, Wo=Wo, eh=Hh - ((Ho - 1) * s + k - 2 * pad), ew=Ww - ((Wo - 1) * s + k - 2 * pad),
                nkb=-(-k * k * c['cout'] // 32))


def plan_forms():
    """(tile, plan bits 20-23, arithmetic) of every shipped conv entry with the DGRAD flag + the heuristic word of each arithmetic."""
    forms = {(0, 0, m) for m in (0, 1, 2, 7)}
    for prm in SP.CONV_ENTRIES:
        key, plan = prm.values
        if key[6] & ops.DGRAD:
            forms.add((plan & 0xff, (plan >> 20) & 15, SP._math_of(plan)))
    return sorted(forms)


FORMS = plan_forms()


def plan_words(form, nkb):
    """The form with K-split 1, and 3 where the shape has at least 3 k-blocks (a word without a tile is the heuristic's: once)."""
    tile, var, m = form
    if tile == 0:
        return [m << 16 | var << 20]
    return [tile | ks << 8 | m << 16 | var << 20 for ks in (1, 3) if ks == 1 or nkb >= 3]


def test_dgrad_cases_reach_what_they_are_for():
    G = {n: geom(c) for n, c in DCASES.items()}
    par = lambda n: (G[n]['eh'], G[n]['ew'])
    assert par('s2_even_odd') == (1, 0) and par('s2_odd_even') == (0, 1) and par('s2_odd_odd') == (0, 0) and par('s2_even_mask') == (1, 1)
    assert par('p0_s2_9x12') == (0, 1) and par('p0_s2_12x9') == (1, 0) and par('stem_s2') == (1, 0) and par('s1_mask') == (0, 0)
    assert DCASES['s2_even_odd']['cin'] % 64 == 32                                   # a ragged column tile (dX has the forward Cin)
    assert DCASES['s2_odd_odd']['mask'] and DCASES['s2_even_mask']['mask'] and DCASES['s1_mask']['mask']
    assert G['s1_mask']['H'] * G['s1_mask']['W'] == 35 < 64                           # fewer rows than one tile per image
    assert all((B * g['H'] * g['W']) % 64 for g in G.values())                        # every last row tile is ragged
    assert {ky >> 1 for ky in range(7)} == {0, 1, 2, 3} and DCASES['stem_s2']['k'] ** 2 == 49 <= 64
    assert all(g['nkb'] >= 3 for g in G.values())                                     # K-split 3 runs on every geometry
    # 1x1, stride 2, no padding: one input pixel in four has a tap at all
    k = dcase('p0_s2_9x12')
    assert abs(float((dbars('p0_s2_9x12')['fp32'][2] > 0).double().mean()) - 0.25) < 0.03
    # masks: positive, negative, +0.0 and -0.0
    m = dcase('s2_odd_odd')['mask']
    z = m[m == 0]
    assert bool((m > 0).any()) and bool((m < 0).any()) and bool(torch.signbit(z).any()) and bool((~torch.signbit(z)).any())
    # the forms: every arithmetic, the pre-split tiles and the 256-column tile among them
    print('data-gradient plan forms (tile, bits 20-23, arithmetic): %s' % [(hex(t), v, MATH_NAME[m]) for t, v, m in FORMS])
    assert {m for _, _, m in FORMS} == {0, 1, 2, 7} and any(t == 0x44 for t, _, _ in FORMS) and any(t == 0x21 for t, _, _ in FORMS)
    assert plan_words((0x11, 4, 7), 5) == [0x11 | 1 << 8 | 7 << 16 | 4 << 20, 0x11 | 3 << 8 | 7 << 16 | 4 << 20]
    assert plan_words((0, 0, 2), 5) == [2 << 16] and k['dy'].shape == (B, 128, 5, 6)


# ------------------------------------------------------------------------------------------------ cases and float64 references
@functools.lru_cache(maxsize=None)
def dcase(name):
    """dY (B, Cout, Ho, Wo), the forward filters w (Cout, Cin, k, k), the mask (B, Cin, H, W) or None: plain randn, seeded by name."""
    c, g = DCASES[name], geom(DCASES[name])
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    dy = torch.randn(B, c['cout'], g['Ho'], g['Wo'], generator=gen)
    w = torch.randn(c['cout'], c['cin'], c['k'], c['k'], generator=gen) / (c['k'] * c['k'] * c['cout']) ** 0.5
    mask = None
    if c['mask']:
        mask = torch.randn(B, c['cin'], g['H'], g['W'], generator=gen)
        mask.view(-1)[::7] = 0.0
        mask.view(-1)[3::11] = -0.0
    return dict(c=c, g=g, name=name, dy=dy, w=w, mask=mask)


def grad_in(k, dy, w, dtype):
    c, g = k['c'], k['g']
    return torch.nn.grad.conv2d_input((B, c['cin'], g['H'], g['W']), w.to(dtype), dy.to(dtype), stride=c['s'], padding=c['pad'])


def keep_of(k):
    return 1.0 if k['mask'] is None else (k['mask'] > 0).double()


@functools.lru_cache(maxsize=None)
def dbars(name):
    """arithmetic name -> (ref, bar, bnd, sens) in float64; sens = ref without the last 32 channels of dY, all taps."""
    k = dcase(name)
    keep = keep_of(k)
    out = {}
    for a, m in (('fp32', 0), ('bf16x6', 1), ('bf16', 2), ('f16x3', 7)):
        rnd = (lambda t: t.bfloat16().double()) if m == 2 else (lambda t: t.double())
        d64, w64 = rnd(k['dy']), rnd(k['w'])
        ref = grad_in(k, d64, w64, F64) * keep
        bnd = grad_in(k, d64.abs(), w64.abs(), F64) * keep
        delta = grad_in(k, d64[:, -32:], w64[-32:], F64) * keep
        out[a] = (ref, C_ARITH[m] * bnd + 1e-30, bnd, ref - delta)
    return out


def standin(k, arith, drop_tap=None):
    """fp32 ATen on the CPU in the kernel's place (on the bf16-rounded operands for plain bf16).  drop_tap = (ky, kx): left out."""
    dy, w = k['dy'], k['w']
    if drop_tap is not None:
        w = w.clone()
        w[:, :, drop_tap[0], drop_tap[1]] = 0
    if arith == 'bf16':
        dy, w = dy.bfloat16().float(), w.bfloat16().float()
    return grad_in(k, dy, w, F32) * (1.0 if k['mask'] is None else (k['mask'] > 0).float())


def measure(got, name, arith):
    """got: dX as (B, Cin, H, W).  (largest |dX - ref| / bar, largest |dX - ref| / bnd, share of the elements with a valid tap on
    which the sensitivity reference is beyond the bar, exactly zero wherever mask <= 0)."""
    ref, bar, bnd, sens = dbars(name)[arith]
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    valid = bnd > 0
    tell = float(((got - sens).abs() > bar)[valid].double().mean())
    mask = dcase(name)['mask']
    zero = True if mask is None else bool((got[mask <= 0] == 0).all())
    return float((err / bar).max()), float((err / bnd.clamp_min(1e-300))[valid].max()), tell, zero


def check(S, name, arith, tag, got, stand=None):
    fr, ratio, tell, zero = measure(got, name, arith)
    if stand is None and fr > 0.25:
        # the stand-in itself, not 4x under the bar: an 8x-rule case (the GPU test decides by the same measurement); it must
        # at least sit within half the bar
        S.add((name, tag), arith + '/8x_standin', fr, 'bar', shrink=0.5)
    else:
        S.add((name, tag), arith, fr, 'bar', standin=stand)
    S.add((name, tag), arith + '/finite', bool(torch.isfinite(got).all()))
    S.add((name, tag), arith + '/zero_where_mask_is_not_positive', zero)
    S.add((name, tag), arith + '/a_missing_k_block_shows_on_1_percent', tell >= 0.01)
    return ratio


@pytest.mark.parametrize('name', list(DCASES))
def test_standin_dgrad(name):
    S = Sweep('standin/dgrad[%s]' % name, shrink=0.25, bars=UNIT, prefix='dgrad_edges/')
    k = dcase(name)
    for a in ('fp32', 'bf16x6', 'bf16', 'f16x3'):
        check(S, name, a, 'aten_fp32', standin(k, a))
    S.finish(record=False)


def test_standin_with_a_dropped_element_misses_the_bars():
    """The float64 reference of `s2_odd_odd` without ONE tap against every arithmetic's bar, on the elements that tap reaches."""
    name, tap = 's2_odd_odd', (1, 1)
    k = dcase(name)
    out = {}
    for a in ('fp32', 'bf16x6', 'bf16', 'f16x3'):
        ref, bar, _, _ = dbars(name)[a]
        rnd = (lambda t: t.bfloat16().double()) if a == 'bf16' else (lambda t: t.double())
        only = torch.zeros_like(k['w'])
        only[:, :, tap[0], tap[1]] = k['w'][:, :, tap[0], tap[1]]
        delta = grad_in(k, rnd(k['dy']), rnd(only), F64) * keep_of(k)
        reached = grad_in(k, rnd(k['dy']).abs(), rnd(only).abs(), F64) * keep_of(k) > 0
        miss = (delta.abs() / bar)[reached]
        out[a] = (float(miss.max()), float((miss > 1).double().mean()), float(reached.double().mean()))
    print('s2_odd_odd without tap %s, (largest |dX - ref| / bar, share of the reached elements beyond the bar, share reached): %s' % (tap, out))
    assert all(f > 100 and share > 0.9 and 0.05 < reached < 0.25 for f, share, reached in out.values()), out
    # ... and the fp32 stand-in that drops the tap misses as well
    assert measure(standin(k, 'fp32', drop_tap=tap), name, 'fp32')[0] > 100


# ------------------------------------------------------------------------------------------------------------ the kernels
MARGIN = {}


def note(arith, ratio):
    MARGIN[arith] = max(MARGIN.get(arith, 0.0), ratio)
    H.record_parity('dgrad_edges/' + arith, {'largest_err_over_bnd': MARGIN[arith], 'c': C_ARITH[{v: n for n, v in MATH_NAME.items()}[arith]]})


@gpu
@pytest.mark.parametrize('name', list(DCASES))
def test_dgrad_vs_float64(lib, name):
    """One geometry of DCASES on every plan form and K-split: the arithmetic that ran is the plan's own, no fault word, every
    element within the bar of its arithmetic, exactly zero under the mask, the sensitivity reference beyond the bar on >= 1 % of
    the elements with a valid tap.  Refused forms are listed; each of the four arithmetics must run at least once."""
    k = dcase(name)
    c, g = k['c'], k['g']
    dy = k['dy'].permute(0, 2, 3, 1).contiguous().to(DEV)
    dy.__dict__['_swem_grad'] = True                      # (autograd._Conv.backward marks the map: f16x3 reads the scaled pair)
    mask = None if k['mask'] is None else k['mask'].permute(0, 2, 3, 1).contiguous().to(DEV)
    # the data-gradient pack of autograd._dgrad_pack: filters [Cin][KH][KW][Cout]
    pk = ops.ConvPack(k['w'].to(DEV).permute(1, 2, 3, 0).contiguous(), None, None, c['cin'], c['k'], c['k'], c['s'], c['pad'], lazy_planes=True)
    pk.fast16 = True
    stand = {a: measure(standin(k, a), name, a)[0] for a in ('fp32', 'bf16x6', 'bf16', 'f16x3')}
    S = Sweep('dgrad[%s]' % name, bars=UNIT, prefix='dgrad_edges/')
    skipped, ran_on, worst = [], {}, {}
    for form in FORMS:
        a = MATH_NAME[form[2]]
        for plan in plan_words(form, g['nkb']):
            ops.MATH_RAN = {}
            try:
                y = ops.conv2d([dy], pk, dgrad=(g['H'], g['W']), mask=mask, batch=B, plan=plan)
            except _lib.SwemHipError as e:
                skipped.append('%#x (%s): %s' % (plan, a, str(e)[:120]))
                continue
            finally:
                ran = dict(ops.MATH_RAN)
                ops.MATH_RAN = None
            ops.check_faults()
            S.add((name, hex(plan)), a + '/ran_its_own_arithmetic', ran == {form[2]: 1})
            S.add((name, hex(plan)), a + '/shape', tuple(y.shape) == (B, g['H'], g['W'], c['cin']))
            ratio = check(S, name, a, hex(plan), y.permute(0, 3, 1, 2), stand[a])
            worst[a] = max(worst.get(a, 0.0), ratio)
            ran_on[a] = ran_on.get(a, 0) + 1
    for a, r in worst.items():
        note(a, r)
    print('dgrad [%s]: launches per arithmetic %s, largest |dX - ref| / bnd %s; skipped (refused by the library): %s'
          % (name, ran_on, {a: float('%.3g' % r) for a, r in worst.items()}, skipped or 'none'))
    H.record_parity('dgrad_edges/skipped[%s]' % name, skipped)
    S.add(name, 'every_arithmetic_ran', set(ran_on) == {'fp32', 'bf16x6', 'bf16', 'f16x3'})
    S.finish()
