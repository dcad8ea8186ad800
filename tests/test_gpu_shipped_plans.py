"""GPU: every entry of every shipped plan file (swem_amd/plans/), run exactly as it ships -- its own plan, at its own layer shape
-- against the same operation in float64 on the device, element by element.

The product runs these plans, not the hand-picked ones of tests/test_gpu_ops.py, and the kernels' behaviour depends on the
real shape: resolve_plan clamps the K-split against the layer's k-block count, the tail split only turns on when the tile
grid overfills the chip, the 256-column tile heights were picked for one M.  The whole-frame parity tests see these plans
only through the logits after the whole network; here each layer has to stand on its own.

Per element the bar is  |y - ref| <= c * bnd + 1e-30,  bnd = the same operation on |operands| (conv(|x|, |w|) + |b| + |res|;
for the GLU gate bnd_f * sigma(a) + |f| * sigma'(a) * bnd_a; for the readout sum_l p_l |nu_l|), with c fixed per arithmetic
(C_ARITH below).  Every entry also proves its bar can fail at its shape: the reference with ONE k-block's contribution removed
must break the same bar on at least 1 % of the elements, so a missing or doubled K-split / tail-split slice cannot pass."""
import contextlib
import json
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import swem_oracle as O
from swem_amd import ops
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24          # the fp32 unit roundoff

# c per arithmetic (plan math field; 7 = f16x3), a-priori:
#  0 fp32 MFMA / 1 bf16x6: fp32 products of the operands (bf16x6: the six products of the exact three-plane split cover all 24
#    bits), fp32 accumulation.  Its error relative to sum |x w| grows like a random walk, not like K: a few U over millions of
#    elements, plus the K-split / tail-split reduction, the epilogue's scale / shift / residual adds and the output rounding.
#  2 plain bf16: the same, against the float64 operation on the bf16 round-to-nearest-even operands (the arithmetic it promises,
#    tests/test_gpu_ops.py::test_conv2d_plain_bf16_mode).
#  7 f16x3: each operand is the fp16 pair hi + mid, exact to half an ulp at 22-23 bits (filters scaled per column into
#    [2^13, 2^14) first; activations below 2^-2 to 2^-25 absolute), the dropped mid * mid product is 2^-22 relative, then fp32
#    accumulation as above.
#  3 bf16x3 (none shipped): two bf16 planes = 16 significant bits per operand.
C_ARITH = {0: 16 * U, 1: 16 * U, 2: 16 * U, 7: 2.0 ** -19, 3: 2.0 ** -14}
MATH_NAME = {0: 'fp32', 1: 'bf16x6', 2: 'bf16', 3: 'bf16x3', 7: 'f16x3'}
# matching's readout (mem_out = sum_l p_l nu_l over both banks): the probabilities come from fp32 affinities of unit vectors,
# |d aff| <= C * U (C = 128 key channels; + a few U for the normalisations); exp((aff - max) / tau) / sum then moves each p_l by
# at most 2 |d aff| / tau relative.  The readout GEMM itself adds at most the f16x3 term (the pre-split readout) or 16 U.
TAU, TOPL = 0.05, 64
C_READOUT = 2 * (128 + 8) * U / TAU + 2.0 ** -19

PLAN_FILES = (('inf', 'mi355x_480p_k256'), ('amp', 'mi355x_train_384_k256_amp'), ('f32lvl', 'mi355x_train_384_k256_fp32_level'))
MARGIN = {}             # arithmetic name -> (largest |y - ref| / bnd seen in this module, its bar c)


def _entries(section):
    out = []
    for short, name in PLAN_FILES:
        with open(ops.shipped_plans(name)) as f:
            d = json.load(f)
        for key, plan in d.get(section, []):
            key = tuple(key)
            if section == 'conv':
                cin, cout, kh, kw, stride, pad, flags, B, Hh, Ww = key[:10]
                tag = key[10:]
                pre = short + ('-math' + ''.join(str(m) for m in tag[1:]) if tag and short == 'inf' else '')
                tid = '%s:%dx%d_k%ds%dp%d_f%d_B%d_%dx%d:%#x' % (pre, cin, cout, kh, stride, pad, flags, B, Hh, Ww, plan)
            else:
                N, Cc, V, P, L, nb = key[:6]
                tag = key[6:]
                pre = short + ('-math' + ''.join(str(m) for m in tag[1:]) if tag else '')
                tid = '%s:N%d_C%d_V%d_P%d_L%d_banks%d:%#x' % (pre, N, Cc, V, P, L, nb, plan)
            out.append(pytest.param(key, plan, id=tid))
    return out


CONV_ENTRIES = _entries('conv')
MATCH_ENTRIES = _entries('match')


@pytest.fixture(scope='module', autouse=True)
def _margins():
    yield
    for name, (r, c) in sorted(MARGIN.items()):
        print('\nshipped plans, %s: largest |y - ref| / bnd = %.3g (bar %.3g)' % (name, r, c))


def _gen(key, plan):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr((key, plan)).encode()))


def _math_of(plan):
    m = (plan >> 16) & 7
    return m if m == 7 else m & 3


def _check(y, ref, bnd, sens, c, what):
    """|y - ref| <= c bnd everywhere; >= 1 % of the elements of the reference with one k-block removed break the same bar."""
    assert bool(torch.isfinite(y).all()), '%s: NaN / inf in the output' % what
    y = y.double()
    bar = c * bnd + 1e-30
    err = (y - ref).abs()
    worst = float((err - bar).max())
    ratio = float((err / bnd.clamp_min(1e-300)).max())
    assert worst <= 0, '%s: |y - ref| exceeds %.3g * bnd by %.3g (largest |y - ref| / bnd %.3g)' % (what, c, worst, ratio)
    frac = float(((y - sens).abs() > bar).double().mean())
    assert frac >= 0.01, '%s: only %.4f of the elements tell a missing k-block apart at this bar' % (what, frac)
    return ratio


@pytest.mark.parametrize('key,plan', CONV_ENTRIES)
def test_shipped_conv_plan(lib, key, plan):
    """One conv entry (key (cin, cout, kh, kw, stride, pad, flags, B, H, W) + conv_math tag) with exactly its plan: inputs as the
    product builds them (ops.pack_conv / ops.pack_glu; for the data gradient the transposed-filter pack and dgrad=(H, W) as
    swem_amd/autograd.py calls it, with the ReLU mask for MASK_POS), the arithmetic that ran must be the plan's own
    (ops.MATH_RAN), no fault word, and every element within the bar of its arithmetic against float64."""
    cin, cout, kh, kw, stride, pad, flags, B, Hh, Ww = key[:10]
    tag = key[10:]
    g = _gen(key, plan)
    math = _math_of(plan)
    c = C_ARITH[math]
    rnd = (lambda t: t.bfloat16().double()) if math == 2 else (lambda t: t.double())
    relu_in, relu_out, glu, dgrad = bool(flags & ops.RELU_IN), bool(flags & ops.RELU_OUT), bool(flags & ops.GLU), bool(flags & ops.DGRAD)
    c_in = min(32, cin)                  # the k-block the sensitivity reference leaves out: input channels [cin - c_in, cin), last tap
    ops.MATH_RAN = {}
    if dgrad:
        # data gradient of a forward conv (cout -> cin channels, filters wf [cin][cout][kh][kw]): dY (B, H, W, cin) -> dX at the
        # forward input's size (the EH / EW bits: the rows / columns the strided filter never reached)
        Ho = (Hh - 1) * stride + kh - 2 * pad + (1 if flags & ops.DGRAD_EH else 0)
        Wo = (Ww - 1) * stride + kw - 2 * pad + (1 if flags & ops.DGRAD_EW else 0)
        dy = torch.randn((B, Hh, Ww, cin), generator=g, device=DEV)
        wf = torch.randn((cin, cout, kh, kw), generator=g, device=DEV) / (kh * kw * cin) ** 0.5
        mask = torch.randn((B, Ho, Wo, cout), generator=g, device=DEV) if flags & ops.MASK_POS else None
        pk = ops.ConvPack(wf.permute(1, 2, 3, 0).contiguous(), None, None, cout, kh, kw, stride, pad, lazy_planes=True)
        pk.fast16 = True
        with ops.conv_math(tag[1:]) if tag else contextlib.nullcontext():
            y = ops.conv2d([dy], pk, dgrad=(Ho, Wo), mask=mask, batch=B, plan=plan)
        ops.check_faults()
        torch.cuda.synchronize()
        d64, w64 = rnd(dy).permute(0, 3, 1, 2), rnd(wf)
        size = (B, cout, Ho, Wo)
        grad_in = lambda t, w_: torch.nn.grad.conv2d_input(size, w_, t, stride=stride, padding=pad)
        acc = grad_in(d64, w64)
        bnd = grad_in(d64.abs(), w64.abs())
        delta = grad_in(d64[:, cin - c_in:], _last_tap(w64[cin - c_in:]))
        del d64, w64
        keep = (mask.permute(0, 3, 1, 2) > 0).double() if mask is not None else 1.0
        ref, sens, bnd = acc * keep, (acc - delta) * keep, bnd * keep
    else:
        x = torch.randn((B, Hh, Ww, cin), generator=g, device=DEV)
        wsh = (2 * cout if glu else cout, cin, kh, kw)
        w = torch.randn(wsh, generator=g, device=DEV) / (kh * kw * cin) ** 0.5
        b = torch.randn(wsh[0], generator=g, device=DEV) * 0.1
        if glu:
            pk = ops.pack_glu(w[:cout], b[:cout], w[cout:], b[cout:])
            res = None
        else:
            pk = ops.pack_conv(w, b, stride=stride, pad=pad)
            Ho, Wo = (Hh + 2 * pad - kh) // stride + 1, (Ww + 2 * pad - kw) // stride + 1
            res = torch.randn((B, Ho, Wo, cout), generator=g, device=DEV)
        assert pk.cin == cin and pk.cout == cout
        with ops.conv_math(tag[1:]) if tag else contextlib.nullcontext():
            y = ops.conv2d([x], pk, relu_in=relu_in, relu_out=relu_out, residual=res, plan=plan)
        ops.check_faults()
        torch.cuda.synchronize()
        x64, w64 = rnd(x).permute(0, 3, 1, 2), rnd(w)
        del x
        if relu_in:
            x64 = x64.clamp_min(0)
        conv = lambda t, w_: F.conv2d(t, w_, stride=stride, padding=pad)
        b64 = b.double()[None, :, None, None]
        acc = conv(x64, w64) + b64
        bnd = conv(x64.abs(), w64.abs()) + b64.abs()
        delta = conv(x64[:, cin - c_in:], _last_tap(w64[:, cin - c_in:]))
        del x64, w64
        if glu:
            f, a, bf, ba = acc[:, :cout], acc[:, cout:], bnd[:, :cout], bnd[:, cout:]
            sig = torch.sigmoid(a)
            ref = f * sig
            sens = (f - delta[:, :cout]) * torch.sigmoid(a - delta[:, cout:])
            bnd = bf * sig + f.abs() * sig * (1 - sig) * ba
        else:
            r64 = res.double().permute(0, 3, 1, 2)
            ref, sens, bnd = acc + r64, acc - delta + r64, bnd + r64.abs()
            del r64
            if relu_out:
                ref, sens = ref.clamp_min(0), sens.clamp_min(0)
        del acc, delta
    ran = dict(ops.MATH_RAN)
    ops.MATH_RAN = None
    assert ran == {math: 1}, 'plan %#x (%s) ran %s' % (plan, MATH_NAME[math], {MATH_NAME[k]: n for k, n in ran.items()})
    ratio = _check(y.permute(0, 3, 1, 2), ref, bnd, sens, c, 'plan %#x (%s)' % (plan, MATH_NAME[math]))
    MARGIN[MATH_NAME[math]] = (max(MARGIN.get(MATH_NAME[math], (0.0,))[0], ratio), c)
    del y, ref, sens, bnd
    torch.cuda.empty_cache()


def _last_tap(w):
    """w restricted to its last filter tap (kh - 1, kw - 1): with the channel slice, one 32-channel k-block of the GEMM."""
    t = torch.zeros_like(w)
    t[:, :, -1, -1] = w[:, :, -1, -1]
    return t


@pytest.mark.parametrize('key,plan', MATCH_ENTRIES)
def test_shipped_readout_plan(lib, key, plan):
    """One readout entry of the `match` section (key (N, C, V, P, L, banks) + conv_math tag; ops._match_plan) with exactly its
    plan, through the call the product makes at that key: ops.match for the first matched frame (one bank, modules.py), the
    persistent pack for two banks (ops.match_packed; N = 8 / 12 / 20: the four clips of a lock-step lane in one call,
    evaluator.py).  mem_out against the oracle's get_affinity in float64, per element within C_READOUT * sum_l p_l |nu_l|; with
    32 bases of one bank dropped from the reference >= 1 % of the elements must break that bar."""
    N, Cc, V, P, L, nb = key[:6]
    tag = key[6:]
    g = torch.Generator().manual_seed(zlib.crc32(repr((key, plan)).encode()))
    clips = 4 if N in (8, 12, 20) else 1
    # bases as the reference draws them (modules.py:170-178, normalised keys) with values ~ N(0, 1); structured query keys
    kap = [torch.nn.functional.normalize(torch.randn(N, 2, Cc, L, generator=g), dim=2) for _ in range(nb)]
    nu = [torch.randn(N, 2, V, L, generator=g) for _ in range(nb)]
    qk = torch.stack([H.structured_keys(P, Cc, 6, g)[0] for _ in range(clips)])           # (clips, P, C), raw
    d = lambda t: t.contiguous().to(DEV)
    book = ops.PlanBook(fallback=ops.MODEL_FALLBACK)
    book.match[key] = plan
    with ops.use_book(book), (ops.conv_math(tag[1:]) if tag else contextlib.nullcontext()):
        if nb == 1:
            assert clips == 1
            mem, _ = ops.match(d(qk[0]), d(kap[0]), d(nu[0]), None, None, TOPL, TAU)
        else:
            pack = ops.new_pack(N, Cc, V, L, DEV)
            ops.pack_bank(d(kap[0]), d(nu[0]), pack, 0)
            ops.pack_bank(d(kap[1]), d(nu[1]), pack, 1)
            mem, _ = ops.match_packed(d(qk if clips > 1 else qk[0]), pack, L, TOPL, TAU, clips=clips)
    ops.check_faults()
    torch.cuda.synchronize()
    # float64 oracle: both banks side by side on the base axis (modules.py:282-283), each clip's objects against its own keys
    mk = torch.cat([k.double() for k in kap], -1).to(DEV)                                  # (N, 2, C, Lm)
    mv = torch.cat([v.double() for v in nu], -1).to(DEV)                                   # (N, 2, V, Lm)
    per = N // clips
    refs, bnds, senss = [], [], []
    drop = torch.ones_like(mv)
    drop[:, 0, :, :32] = 0                   # 32 bases of the first class of the first bank
    for s_ in range(clips):
        q = qk[s_].double().t().reshape(1, Cc, P, 1).to(DEV)
        sl = slice(s_ * per, (s_ + 1) * per)
        _, ref = O.get_affinity(O.l2norm(q, 1), O.l2norm(mk[None, sl], -2), mv[None, sl], TAU, TOPL)
        _, bnd = O.get_affinity(O.l2norm(q, 1), O.l2norm(mk[None, sl], -2), mv[None, sl].abs(), TAU, TOPL)
        _, sens = O.get_affinity(O.l2norm(q, 1), O.l2norm(mk[None, sl], -2), (mv * drop)[None, sl], TAU, TOPL)
        refs.append(ref[0, :, :, :, 0])
        bnds.append(bnd[0, :, :, :, 0])
        senss.append(sens[0, :, :, :, 0])
    ref, bnd, sens = torch.cat(refs), torch.cat(bnds), torch.cat(senss)                  # (N, V, P)
    ratio = _check(mem.transpose(1, 2), ref, bnd, sens, C_READOUT, 'readout plan %#x' % plan)
    MARGIN['readout'] = (max(MARGIN.get('readout', (0.0,))[0], ratio), C_READOUT)
