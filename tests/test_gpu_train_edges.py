"""GPU: the training step's pointwise and loss kernels (csrc/train.hip, the CBAM backward of csrc/pointwise.hip, the column and
batch sums of csrc/train_conv.hip) against float64 at the corners tests/test_gpu_train.py does not reach: partial column blocks,
more than 16 row blocks, every `bn_rows` value up to the 512-row clamp, C = 2048, BatchNorm statistics with the conv output
centred ON the mean (the cancellation in dgamma), every `lanes = 256 / (C/4)` of the prediction head from 1 to 256, fewer pixels
than pixel lanes / chunks in the CBAM kernels and ties in both of its maxima, every clamp branch of the decode head, ties and exact
zeros at the radix select's threshold, the AdamW gate.

Every comparison is per kernel, identical inputs on both sides.  The reference is float64: torch CPU autograd of the same stage on
.double() inputs, or the oracle's functions (O.cbam, O.vos_loss) -- where a test needs what they do not offer (first-index ties,
the fp32 values of the clamp bounds, the even sharing of the top-k threshold), the restatement below is checked against them on the
CPU first.  The bars are the per-stage bars of tests/test_gpu_train.py (BARS), measured the way its `close` does: max error over
max |reference|.

Every sweep exists twice: `test_*` marked gpu runs the kernels, `test_standin_*` (no GPU) runs the SAME cases and checks with fp32
torch -- for the column sums a float32 emulation of the kernels' own order (`emu_colsum`) -- standing in for the kernel, and asserts
that the stand-in sits at least 4x under every bar: a bar the fp32 arithmetic itself cannot keep would be a coin toss.  Worst
stand-in error / bar per sweep (CPU, fp32):
    bn / colsum   fold 8.9e-8 / 1e-6, forward 9.7e-8 / 1e-5, dc 5.2e-8 / 1e-5, dz 0 / 1e-6, dgamma 1.1e-6 / 3e-5 (the kernels' order
                  at (40000, 64)), dbeta 4.3e-7 / 3e-5, colsum 4.5e-7 / 3e-5 (both at (600000, 4))
    resampling    2.8e-7 / 2e-6          GLU          1.5e-7 / 2e-6        pred head    5.4e-7 / 1e-4
    CBAM          dx 3.1e-7 / 5e-5, parameters 3.7e-6 / 1e-4               loss         values 1.6e-7 / 2e-6, dlogits 5.0e-7 / 2e-5
    decode head   3.1e-6 / 1e-4 (N >= 2 valid objects)                     AdamW        p 0.50 ulp / 1 ulp, m and v 1.0e-7 / 1e-6
Where a case's stand-in is NOT 4x under the bar, the case's bar is 8x what the stand-in measures on it, never a guess (value and
source in BARS, or computed from the stand-in beside the kernel: Sweep.add(standin=)):
    - bilinear adjoints with 7 -> 13 (6.1e-7) or 27 -> 107 (2.76e-6) on an axis: the fp32 source coordinate;
    - loss rows of ONE pixel (1.1e-6 / 3.0e-6) and the loss values of the 300-pixel zero-threshold rows (1.35e-6): lone rounded
      differences log(1 + e), 1 - IoU; one CBAM tie case's scalar bias gradient (9.1e-5): a cancelling sum;
    - the decode head wherever all VALID objects of a pixel vanish (N = 1, or a zero in `valid` with N = 2) or dprob meets seven
      objects: fp32 resolves 1 - bg and 1 - p to 6e-8 -- fp32 ATen is 1e-3 .. 9e-3 from float64 there, and the kernel lands on
      exactly 1/8 of those bars (the same arithmetic); a wrong clamp branch is O(1).
What a bar is worth, shown once per sweep with a stand-in that drops ONE row / pixel at the sweep's largest case
(`test_standin_with_a_dropped_element_misses_the_bars`): BatchNorm dbeta at (40000, 64) 141x its bar, colsum at (600000, 4) 47x,
resampling 27 -> 107 9100x, pred head dw at C = 1024 713x, CBAM dw1 at (1024, 64, 7x9) 609x, decode head (N = 2) 901x, loss dlogits
at HW = 5000 5e4x.

What the kernels measure is printed and recorded under train_edges/<kernel> (helpers.record_parity) before anything is asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import swem_oracle as O
from swem_amd import _lib, ops
from tests import helpers as H

gpu = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64

# tests/test_gpu_train.py's per-stage bars
BARS = {'bn_fwd': 1e-5, 'dc': 1e-5, 'dgamma': 3e-5, 'dbeta': 3e-5, 'colsum': 3e-5, 'dres': 1e-6, 'maxpool': 1e-6, 'bilinear': 2e-6,
        'glu': 2e-6, 'cbam_fwd': 1e-5, 'cbam_dx': 5e-5, 'cbam_param': 1e-4, 'heads': 1e-4, 'loss': 2e-6, 'dlogits': 2e-5,
        # bn_fold has no bar there: alpha, shift and invstd are three to four fp32 roundings of O(1) values (2.4e-7); 1e-6 = 4x that
        'bn_fold': 1e-6,
        # AdamW (the bars the sweep was given): p in fp32 ulps of the float64 update, the moments relative
        'adam_p_ulp': 1.0, 'adam_mv': 1e-6,
        # bilinear adjoints at the two size pairs where fp32 ATen itself is not 4x under 2e-6 (the source coordinate
        # scale * (dst + 0.5) - 0.5 is an fp32 number up to 27: its rounding is a weight error of 1e-6): 8x what fp32 ATen measures on
        # the same cases against float64 -- 6.1e-7 with 7 -> 13 on an axis, 2.76e-6 with 27 -> 107 (test_standin_bilinear_adjoints)
        'bilinear_7_13': 4.9e-6, 'bilinear_27_107': 2.2e-5,
        # the other cases whose fp32 stand-in is not 4x under its bar, each at 8x what the stand-in measures on that case (the
        # test_standin_* of the sweep prints it): rows of ONE pixel (raw, threshold, sums 1.12e-6; loss values 2.98e-6: the row's only
        # cross entropy log(1 + e) and 1 - IoU are rounded differences with nothing larger beside them), the loss values of the
        # 300-pixel zero-threshold rows (1.35e-6: aux = 1 - IoU with IoU = 0.97), and the spatial conv's bias gradient of ONE tie
        # case, a scalar that is a cancelling sum (9.1e-5)
        'loss_hw1_raw': 9.0e-6, 'loss_hw1_values': 2.4e-5, 'loss_zero_300': 1.1e-5, 'cbam_db7_ties_72': 7.3e-4}


# ------------------------------------------------------------------------------------------------------------ helpers
def dv(t):
    return None if t is None else t.to(DEV).contiguous()


def ptr(t):
    return 0 if t is None else t.data_ptr()


def leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def rel(got, want):
    """the measure of test_gpu_train.close: max |got - want| / max |want|"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


def ulps(got, want64):
    """largest distance of fp32 `got` from float64 `want64` in units of want64's fp32 ulp"""
    _, e = torch.frexp(want64.abs())
    return float(((got.detach().double().cpu() - want64).abs() / torch.ldexp(torch.ones_like(want64), e - 24)).max())


class Sweep:
    """Collects what a sweep measures (floats: the worst over the cases, wanted <= bar * shrink; bools: wanted True), records it,
    then fails with every case that missed.  shrink = 0.25 for the fp32 stand-ins.  bars / prefix: another module's table of
    bars and the prefix of its parity records (tests/test_gpu_frame_edges.py)."""

    def __init__(self, key, shrink=1.0, bars=None, prefix='train_edges/'):
        self.key, self.shrink, self.worst, self.bad = key, shrink, {}, {}
        self.bars, self.prefix = BARS if bars is None else bars, prefix

    def add(self, case, name, value, bar=None, shrink=None, standin=None):
        BARS = self.bars
        if isinstance(value, bool):
            self.worst[name] = self.worst.get(name, True) and value
            fail = not value
        else:
            limit = BARS[bar] * (self.shrink if shrink is None else shrink)
            if standin is not None and not standin <= BARS[bar] / 4:
                # fp32 ATen on this very case is not 4x under the bar: the case's bar is 8x what fp32 ATen measures on it
                limit, name = 8 * standin, name + '/8x_standin'
                value = value / limit                                  # (recorded as a fraction of the case's own bar)
                limit = 1.0
            self.worst[name] = max(self.worst.get(name, 0.0), value)
            fail = not value <= limit
        if fail:
            self.bad.setdefault(str(case), {})[name] = value

    def finish(self, record=True):
        print('%s: %s' % (self.key, self.worst))
        if record:
            H.record_parity(self.prefix + self.key, self.worst)
        assert not self.bad, self.bad


# ====================================================================================== 1. bn_act, bn_act_bwd, bn_fold, colsum
BN_CASES = [(1, 4), (37, 8), (549, 24), (1000, 72), (300, 2048), (40000, 64), (600000, 4)]
EPS = float(np.float32(1e-5))


def bn_rows(M, C):
    """train.hip's bn_rows / train_conv.hip's cs_rows (host code) restated: rows per block of the column-sum stage."""
    rows = (M * (-(-(C // 4) // 16)) + 1023) // 1024
    return min(max((rows + 15) // 16 * 16, 32), 512)


def test_bn_cases_reach_what_they_are_for():
    """(M, C) -> rows per block, row blocks, column blocks: 32-row blocks with a 5-row tail, 18 row blocks (a second pass of the
    final kernel's j += 16 loop), a partial second column block, 32 column blocks, 48-row blocks and 834 partials, the clamp."""
    got = {mc: (bn_rows(*mc), -(-mc[0] // bn_rows(*mc)), -(-(mc[1] // 4) // 16)) for mc in BN_CASES}
    assert got == {(1, 4): (32, 1, 1), (37, 8): (32, 2, 1), (549, 24): (32, 18, 1), (1000, 72): (32, 32, 2),
                   (300, 2048): (32, 10, 32), (40000, 64): (48, 834, 1), (600000, 4): (512, 1172, 1)}, got
    assert 37 - 32 == 5 < 16 and (72 // 4) % 16 != 0


def emu_colsum(a, rows):
    """Column sums of a (M, C) float32 array in the kernels' own order, in float32: blocks of `rows` rows; in a block 16 row lanes,
    lane r adds rows r, r + 16, ... in order, the lanes are added in order; the block partials go through the same 16 lanes."""
    def lanes(t):                                       # (..., n, C) -> (..., C)
        n, C = t.shape[-2:]
        t = np.concatenate([t, np.zeros(t.shape[:-2] + (-n % 16, C), np.float32)], -2)       # (x + 0 is exact)
        t = t.reshape(t.shape[:-2] + (-1, 16, C))
        s = np.zeros(t.shape[:-3] + (16, C), np.float32)
        for i in range(t.shape[-3]):
            s = s + t[..., i, :, :]
        out = s[..., 0, :].copy()
        for j in range(1, 16):
            out = out + s[..., j, :]
        return out
    M, C = a.shape
    nblk = -(-M // rows)
    a = np.concatenate([a, np.zeros((nblk * rows - M, C), np.float32)]).reshape(nblk, rows, C)
    return torch.from_numpy(lanes(lanes(a)))


def bn_case(M, C):
    """c = mean + sqrt(var) randn with |mean| <= 4 std: the conv output is centred on the running mean, so that
    dgamma = invstd (s2 - mean s1) is the difference of two sums 4 x larger than itself.  The fold the stages are handed is the
    fp32 rounding of the float64 fold; gradient buffers start non-zero."""
    g = torch.Generator().manual_seed(1000 + M + C)
    var = torch.rand(C, generator=g) + 0.5
    mean = (torch.rand(C, generator=g) * 8 - 4) * var.sqrt()
    k = dict(M=M, C=C, var=var, mean=mean, gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g),
             c=mean + var.sqrt() * torch.randn(M, C, generator=g), res=torch.randn(M, C, generator=g),
             dy=torch.randn(M, C, generator=g), g0=torch.randn(C, generator=g), b0=torch.randn(C, generator=g))
    inv = 1.0 / (var.double() + EPS).sqrt()
    alpha = k['gamma'].double() * inv
    k['fold64'] = (alpha, k['beta'].double() - mean.double() * alpha, inv)
    k['alpha'], k['shift'], k['invstd'] = (t.float() for t in k['fold64'])
    return k


def bn_fwd64(k, relu, with_res):
    y = k['c'].double() * k['alpha'].double() + k['shift'].double()
    y = y + k['res'].double() if with_res else y
    return y.clamp(min=0) if relu else y


def bn_bwd64(k, y32, relu):
    dz = k['dy'].double() * (y32 > 0) if relu else k['dy'].double()
    s1, s2 = dz.sum(0), (dz * k['c'].double()).sum(0)
    return dict(dz=dz, dc=dz * k['alpha'].double(), dgamma=k['g0'].double() + k['invstd'].double() * (s2 - k['mean'].double() * s1),
                dbeta=k['b0'].double() + s1)


class HipBN:
    """The kernels through the C ABI; the case's maps are uploaded once."""

    def __init__(self, k):
        self.k = k
        self.d = {n: dv(k[n]) for n in ('c', 'res', 'dy', 'alpha', 'shift', 'invstd', 'mean', 'var', 'gamma', 'beta')}
        self.M, self.C = k['M'], k['C']

    def fold(self):
        d, C = self.d, self.C
        out = torch.full((3, C), float('nan'), device=DEV)
        _lib.call('swem_bn_fold_f32', ops._stream(), d['gamma'].data_ptr(), d['beta'].data_ptr(), d['mean'].data_ptr(),
                  d['var'].data_ptr(), EPS, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), C)
        return out.cpu()

    def fwd(self, relu, with_res, planes=None, nplanes=3):
        d = self.d
        y = torch.full((self.M, self.C), float('nan'), device=DEV)
        _lib.call('swem_bn_act_planes_f32', ops._stream(), d['c'].data_ptr(), d['alpha'].data_ptr(), d['shift'].data_ptr(),
                  d['res'].data_ptr() if with_res else 0, y.data_ptr(), self.M, self.C, int(relu), ptr(planes), nplanes,
                  ops._fault_ptr(y.device))
        return y

    def bwd(self, y32, relu, want_dz, which, planes=None, amax=None):
        d, M, C = self.d, self.M, self.C
        nan = float('nan')
        dz = torch.full((M, C), nan, device=DEV) if want_dz else None
        dc = torch.full((M, C), nan, device=DEV)
        dg = dv(self.k['g0']) if 'gamma' in which else None
        db = dv(self.k['b0']) if 'beta' in which else None
        wsb = _lib.query('swem_bn_act_bwd_workspace', M, C) if which else 0
        ws = torch.empty(max(wsb, 4) // 4, device=DEV) if which else None
        args = (ops._stream(), d['dy'].data_ptr(), ptr(y32), d['c'].data_ptr(), d['alpha'].data_ptr(), d['mean'].data_ptr(),
                d['invstd'].data_ptr(), ptr(dz), dc.data_ptr(), ptr(dg), ptr(db), M, C, int(relu))
        if amax is not None:
            _lib.call('swem_bn_act_bwd_amax_f32', *args, amax.data_ptr(), ptr(ws), wsb)
        else:
            _lib.call('swem_bn_act_bwd_f32', *args, ptr(planes), ptr(ws), wsb)
        return dict(dz=dz, dc=dc, dgamma=dg, dbeta=db)

    def colsum(self, a, b, want1, want2, acc):
        M, C = self.M, self.C
        o1 = dv(self.k['g0']) if want1 else None
        o2 = dv(self.k['b0']) if want2 else None
        wsb = _lib.query('swem_colsum_workspace', M, C)
        ws = torch.empty(wsb // 4, device=DEV)
        _lib.call('swem_colsum_f32', ops._stream(), self.d[a].data_ptr(), ptr(self.d[b]) if b else 0, ptr(o1), ptr(o2), M, C,
                  int(acc), ws.data_ptr(), wsb)
        return o1, o2


class EmuBN:
    """fp32 stand-in: torch on the CPU for the pointwise parts, emu_colsum for the sums.  drop = one row left out of the sums."""

    def __init__(self, k, drop=False):
        self.k, self.M, self.C, self.drop = k, k['M'], k['C'], drop

    def fold(self):
        k = self.k
        inv = 1.0 / (k['var'] + EPS).sqrt()
        a = k['gamma'] / (k['var'] + EPS).sqrt()
        return torch.stack([a, k['beta'] - k['mean'] * a, inv])

    def fwd(self, relu, with_res, planes=None, nplanes=3):
        k = self.k
        y = k['c'] * k['alpha'] + k['shift']
        y = y + k['res'] if with_res else y
        return y.clamp(min=0) if relu else y

    def _sum(self, a):
        a = a.clone()
        if self.drop:
            a[self.M - 1] = 0
        return emu_colsum(a.numpy(), bn_rows(self.M, self.C))

    def bwd(self, y32, relu, want_dz, which, planes=None, amax=None):
        k = self.k
        dz = k['dy'] * (y32 > 0) if relu else k['dy']
        out = dict(dz=dz if want_dz else None, dc=dz * k['alpha'], dgamma=None, dbeta=None)
        if which:
            s1, s2 = self._sum(dz), self._sum(dz * k['c'])
            if 'gamma' in which:
                out['dgamma'] = k['g0'] + k['invstd'] * (s2 - k['mean'] * s1)
            if 'beta' in which:
                out['dbeta'] = k['b0'] + s1
        return out

    def colsum(self, a, b, want1, want2, acc):
        k = self.k
        s1, s2 = self._sum(k[a]), (self._sum(k[a] * k[b]) if b else None)
        return ((k['g0'] + s1 if acc else s1) if want1 else None), ((k['b0'] + s2 if acc else s2) if want2 else None)


def bn_check(S, k, run):
    """One (M, C) case: fold, forward, backward and colsum in every combination the entry points take."""
    M, C = k['M'], k['C']
    f = run.fold()
    for i, n in enumerate(('alpha', 'shift', 'invstd')):
        S.add((M, C), 'fold_' + n, rel(f[i], k['fold64'][i]), 'bn_fold')
    for relu in (1, 0):
        for with_res in (1, 0):
            y64 = bn_fwd64(k, relu, with_res)
            S.add((M, C, relu, with_res), 'fwd', rel(run.fwd(relu, with_res), y64), 'bn_fwd')
            y32 = y64.float()                          # the forward output both sides of the backward are handed
            want = bn_bwd64(k, y32, relu)
            got = run.bwd(y32 if isinstance(run, EmuBN) else dv(y32), relu, with_res, ('gamma', 'beta'))
            tag = (M, C, relu, with_res, 'both')
            S.add(tag, 'dc', rel(got['dc'], want['dc']), 'dc')
            S.add(tag, 'dgamma', rel(got['dgamma'], want['dgamma']), 'dgamma')
            S.add(tag, 'dbeta', rel(got['dbeta'], want['dbeta']), 'dbeta')
            if with_res:
                S.add(tag, 'dz', rel(got['dz'], want['dz']), 'dres')
            else:
                S.add(tag, 'dz_not_asked', got['dz'] is None)
    # one parameter gradient alone, and none (no workspace): the other buffer is not touched, dc is the same
    y32 = bn_fwd64(k, 1, 1).float()
    want = bn_bwd64(k, y32, 1)
    yd = y32 if isinstance(run, EmuBN) else dv(y32)
    for which in (('gamma',), ('beta',), ()):
        got = run.bwd(yd, 1, 1, which)
        tag = (M, C, 'only', which)
        S.add(tag, 'dc', rel(got['dc'], want['dc']), 'dc')
        S.add(tag, 'dz', rel(got['dz'], want['dz']), 'dres')
        for n in ('gamma', 'beta'):
            if n in which:
                S.add(tag, 'd' + n, rel(got['d' + n], want['d' + n]), 'd' + n)
    # colsum: a = dy, b = c (not centred: the bias and BatchNorm sums of the convolution's own backward)
    s1, s2 = k['dy'].double().sum(0), (k['dy'].double() * k['c'].double()).sum(0)
    for b, w1, w2, acc in ((None, 1, 0, 0), (None, 1, 0, 1), ('c', 1, 1, 1), ('c', 1, 1, 0), ('c', 0, 1, 0), ('c', 0, 1, 1), ('c', 1, 0, 0)):
        o1, o2 = run.colsum('dy', b, w1, w2, acc)
        tag = (M, C, 'colsum', b, w1, w2, acc)
        if w1:
            S.add(tag, 'colsum1', rel(o1, k['g0'].double() + s1 if acc else s1), 'colsum')
        if w2:
            S.add(tag, 'colsum2', rel(o2, k['b0'].double() + s2 if acc else s2), 'colsum')


@gpu
@pytest.mark.parametrize('M,C', BN_CASES)
def test_bn_and_colsum_vs_float64(lib, M, C):
    """swem_bn_fold_f32, swem_bn_act_f32, swem_bn_act_bwd_f32 (relu x residual, dz NULL and not, dgamma / dbeta / both / neither,
    accumulating into non-zero buffers) and swem_colsum_f32 (b NULL and present, out1 / out2 / both, accumulate 0 / 1) at BN_CASES.
    The host's block arithmetic is pinned to the restatement above through the two size queries."""
    nrow, cb = -(-M // bn_rows(M, C)), -(-(C // 4) // 16)
    assert _lib.query('swem_bn_act_bwd_amax_parts', M, C) == nrow * cb
    assert _lib.query('swem_bn_act_bwd_workspace', M, C) == nrow * 2 * C * 4 == _lib.query('swem_colsum_workspace', M, C)
    k = bn_case(M, C)
    S = Sweep('bn_colsum[M=%d,C=%d]' % (M, C))
    bn_check(S, k, HipBN(k))
    S.finish()


@gpu
@pytest.mark.parametrize('M,C', BN_CASES)
def test_bn_bwd_block_maxima(lib, M, C):
    """swem_bn_act_bwd_amax_f32: entry by * column blocks + bx of amax_parts is EXACTLY the largest |dc| of row block by, column
    block bx (every block has a live lane: none is left unwritten, none holds anything else); dc and the parameter gradients are
    those of swem_bn_act_bwd_f32 bit for bit."""
    k = bn_case(M, C)
    run = HipBN(k)
    rows, cb = bn_rows(M, C), -(-(C // 4) // 16)
    nrow = -(-M // rows)
    y32 = dv(bn_fwd64(k, 1, 0).float())
    parts = torch.full((nrow * cb,), float('nan'), device=DEV)
    a = run.bwd(y32, 1, False, ('gamma', 'beta'), amax=parts)
    b = run.bwd(y32, 1, False, ('gamma', 'beta'))
    dc = a['dc'].cpu().abs()
    cols = torch.stack([dc[:, 64 * bx:64 * bx + 64].amax(1) for bx in range(cb)], 1)          # (M, cb)
    pad = torch.zeros(nrow * rows, cb)
    pad[:M] = cols
    want = pad.view(nrow, rows, cb).amax(1).reshape(-1)
    same = bool(torch.equal(parts.cpu(), want))
    eq = all(torch.equal(a[n], b[n]) for n in ('dc', 'dgamma', 'dbeta'))
    H.record_parity('train_edges/bn_bwd_amax[M=%d,C=%d]' % (M, C), {'parts': nrow * cb, 'block_maxima_exact': same, 'same_as_plain': eq,
                                                                     'max': float(parts.max()), 'max_dc': float(dc.max())})
    assert same and eq and float(parts.max()) == float(dc.max())


@gpu
@pytest.mark.parametrize('M,C', [(37, 8), (1000, 72)])
def test_bn_planes_are_the_split_kernels_planes(lib, M, C):
    """The operand planes the two stages write beside their output -- bf16 x 3 of y and of dc, the fp16 pair of y -- are bit for
    bit swem_split_bf16x3_f32's / swem_split_f16x2_f32's of the same map, at a C below one 64-channel block and across one."""
    k = bn_case(M, C)
    run = HipBN(k)
    st, fault = ops._stream(), ops._fault_ptr(torch.device('cuda', 0))

    def split3(t):
        out = torch.zeros(3, M * C, dtype=torch.bfloat16, device=DEV)
        _lib.call('swem_split_bf16x3_f32', st, t.data_ptr(), out.data_ptr(), M, C, 0)
        return out

    p3 = torch.zeros(3, M * C, dtype=torch.bfloat16, device=DEV)
    y = run.fwd(1, 1, planes=p3, nplanes=3)
    ok_y3 = torch.equal(p3.view(torch.int16), split3(y).view(torch.int16))
    p2 = torch.zeros(2, M * C, dtype=torch.float16, device=DEV)
    y2 = run.fwd(1, 1, planes=p2, nplanes=ops.PLANES_F16)
    want2 = torch.zeros(2, M * C, dtype=torch.float16, device=DEV)
    _lib.call('swem_split_f16x2_f32', st, y2.data_ptr(), want2.data_ptr(), M, C, 0, fault)
    ok_y2 = torch.equal(p2.view(torch.int16), want2.view(torch.int16)) and torch.equal(y, y2)
    pd = torch.zeros(3, M * C, dtype=torch.bfloat16, device=DEV)
    got = run.bwd(y, 1, True, ('gamma', 'beta'), planes=pd)
    ok_dc = torch.equal(pd.view(torch.int16), split3(got['dc']).view(torch.int16))
    ops.check_faults()
    H.record_parity('train_edges/bn_planes[M=%d,C=%d]' % (M, C), {'y_bf16x3': ok_y3, 'y_f16x2': ok_y2, 'dc_bf16x3': ok_dc})
    assert ok_y3 and ok_y2 and ok_dc and bool(p3.view(torch.int16).any()) and bool(pd.view(torch.int16).any())


@pytest.mark.parametrize('M,C', BN_CASES)
def test_standin_bn_and_colsum(M, C):
    k = bn_case(M, C)
    S = Sweep('standin/bn_colsum[M=%d,C=%d]' % (M, C), shrink=0.25)
    bn_check(S, k, EmuBN(k))
    S.finish(record=False)


# ====================================================================================== 2. sum_batch, sum_groups, expand_groups
@gpu
def test_batch_and_group_sums_bit_equal(lib):
    """y (+)= sum_b x[b] left to right (then + y when accumulating), y[g] = sum_j x[g N + j] left to right, y[g N + j] = x[g]:
    bit-equal to the same fp32 additions on the CPU, at one float4 and at 257 of them (a second block, one lane live)."""
    g = torch.Generator().manual_seed(21)
    ok, st = {}, ops._stream()
    for n in (4, 1028):
        for Bn in (1, 2, 5):
            x, y0 = torch.randn(Bn, n, generator=g), torch.randn(n, generator=g)
            for acc in (0, 1):
                want = x[0].clone()
                for b in range(1, Bn):
                    want = want + x[b]
                want = want + y0 if acc else want
                y, xd = dv(y0), dv(x)
                _lib.call('swem_sum_batch_f32', st, xd.data_ptr(), y.data_ptr(), Bn, n, acc)
                ok['sum_batch n=%d B=%d acc=%d' % (n, Bn, acc)] = torch.equal(y.cpu(), want)
            for G in (1, 3):
                xs = torch.randn(G * Bn, n, generator=g)
                want = xs.view(G, Bn, n)[:, 0].clone()
                for j in range(1, Bn):
                    want = want + xs.view(G, Bn, n)[:, j]
                y, xd = torch.full((G, n), float('nan'), device=DEV), dv(xs)
                _lib.call('swem_sum_groups_f32', st, xd.data_ptr(), y.data_ptr(), G, Bn, n)
                ok['sum_groups n=%d G=%d N=%d' % (n, G, Bn)] = torch.equal(y.cpu(), want)
                xe = torch.randn(G, n, generator=g)
                y, xd = torch.full((G * Bn, n), float('nan'), device=DEV), dv(xe)
                _lib.call('swem_expand_groups_f32', st, xd.data_ptr(), y.data_ptr(), G, Bn, n)
                ok['expand_groups n=%d G=%d N=%d' % (n, G, Bn)] = torch.equal(y.cpu(), xe.repeat_interleave(Bn, 0))
    H.record_parity('train_edges/sums', {'cases': len(ok), 'bit_equal': all(ok.values())})
    assert all(ok.values()), [k for k, v in ok.items() if not v]


# ====================================================================================== 3. maxpool backward, both forms
@gpu
def test_maxpool_backward_every_small_size(lib):
    """swem_maxpool3x3s2_bwd_f32 (scans the windows) and swem_maxpool3x3s2_bwd_y_f32 (reads the forward output) at all 49 (H, W)
    in 1..7 -- one-pixel maps, maps narrower than a window, odd and even edges -- C = 4 and 8, B = 2, on randn inputs and on
    inputs quantised to four levels (ties everywhere): bit-equal to each other, within 1e-6 of ATen's float64 autograd (which
    sends a window's gradient to its first maximum)."""
    g = torch.Generator().manual_seed(31)
    S, st = Sweep('maxpool_bwd'), ops._stream()
    for Hh in range(1, 8):
        for Ww in range(1, 8):
            for C in (4, 8):
                for quant in (False, True):
                    x = torch.randn(2, Hh, Ww, C, generator=g)
                    x = (x * 1.5).round().clamp(-2, 1) if quant else x
                    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
                    yr = F.max_pool2d(xr, 3, 2, 1)
                    dy = torch.randn(2, yr.shape[2], yr.shape[3], C, generator=g)
                    yr.backward(dy.permute(0, 3, 1, 2).double())
                    want = xr.grad.permute(0, 2, 3, 1)
                    xd, dyd = dv(x), dv(dy)
                    yd = ops.maxpool(xd)
                    d_old, d_new = torch.full_like(xd, float('nan')), torch.full_like(xd, float('nan'))
                    _lib.call('swem_maxpool3x3s2_bwd_f32', st, xd.data_ptr(), dyd.data_ptr(), d_old.data_ptr(), 2, Hh, Ww, C)
                    _lib.call('swem_maxpool3x3s2_bwd_y_f32', st, xd.data_ptr(), yd.data_ptr(), dyd.data_ptr(), d_new.data_ptr(), 2, Hh, Ww, C)
                    tag = (Hh, Ww, C, quant)
                    S.add(tag, 'forward_exact', torch.equal(yd.cpu().double(), yr.detach().permute(0, 2, 3, 1)))
                    S.add(tag, 'forms_bit_equal', torch.equal(d_old, d_new))
                    S.add(tag, 'dx', rel(d_new, want), 'maxpool')
    S.finish()


# ====================================================================================== 4. bilinear adjoints
PAIRS = [(1, 1), (1, 5), (2, 3), (3, 8), (5, 5), (7, 13), (6, 24), (12, 24), (27, 107)]


def resize_cases():
    """(C, (Hl, Ho), (Wl, Wo)): every pair on H with every pair on W at C = 4, and shifted by four at C = 36 (nine float4 per pixel)."""
    return ([(4, ph, pw) for ph in PAIRS for pw in PAIRS] + [(36, PAIRS[i], PAIRS[(i + 4) % 9]) for i in range(9)])


def resize_bar(ph, pw):
    return 'bilinear_27_107' if (27, 107) in (ph, pw) else 'bilinear_7_13' if (7, 13) in (ph, pw) else 'bilinear'


def resize_ref(dy_nchw, hl, wl, dtype, drop=False):
    Bn, C, ho, wo = dy_nchw.shape
    low = torch.zeros(Bn, C, hl, wl, dtype=dtype, requires_grad=True)
    dy = dy_nchw.to(dtype)
    if drop:                                                         # (stand-in that loses one destination pixel)
        dy = dy.clone()
        dy[:, :, ho - 1, wo - 1] = 0
    F.interpolate(low, size=(ho, wo), mode='bilinear', align_corners=False).backward(dy)
    return low.grad


def resize_check(S, hip):
    g = torch.Generator().manual_seed(41)
    for C, (hl, ho), (wl, wo) in resize_cases():
        dy = torch.randn(2, C, ho, wo, generator=g)
        want = resize_ref(dy, hl, wl, F64)
        tag, bar = (C, hl, ho, wl, wo), resize_bar((hl, ho), (wl, wo))
        if hip:
            st = ops._stream()
            dyd = dv(dy.permute(0, 2, 3, 1))
            dlow = torch.full((2, hl, wl, C), float('nan'), device=DEV)
            _lib.call('swem_upsample_bwd_nhwc_f32', st, dyd.data_ptr(), dlow.data_ptr(), 2, hl, wl, ho, wo, C)
            S.add(tag, 'upsample_bwd_nhwc', rel(dlow.permute(0, 3, 1, 2), want), bar)
            dx = torch.full((2, C, hl, wl), float('nan'), device=DEV)
            dyp = dv(dy)
            _lib.call('swem_resize_bilinear_bwd_f32', st, dyp.data_ptr(), dx.data_ptr(), 2 * C, hl, wl, ho, wo)
            S.add(tag, 'resize_bilinear_bwd', rel(dx, want), bar)
        else:
            S.add(tag, 'aten_fp32[%s]' % bar, rel(resize_ref(dy, hl, wl, F32), want), bar)


@gpu
def test_bilinear_adjoints_vs_float64(lib):
    """swem_upsample_bwd_nhwc_f32 and swem_resize_bilinear_bwd_f32 against float64 autograd of F.interpolate: one launch carries
    one size pair on H and another on W (identity, one source row, x1.5, x2.67, odd sizes, x2, x4, 27 -> 107), so `lerp_span`
    and the edge clamps of both axes are walked independently.  Bar 2e-6, except with 7 -> 13 (4.9e-6) or 27 -> 107 (2.2e-5) on an
    axis: 8x the error of fp32 ATen there (BARS), which is not 4x under 2e-6 itself.  Then the stage with a skip shared by the 3 objects of a frame:
    its gradient is the left-to-right sum of dy (sum_batch)."""
    from swem_amd import autograd as A
    S = Sweep('bilinear_bwd')
    resize_check(S, True)
    g = torch.Generator().manual_seed(42)
    skip, low = torch.randn(1, 36, 7, 13, generator=g), torch.randn(3, 36, 3, 5, generator=g)
    sr, lr = skip.double().requires_grad_(True), low.double().requires_grad_(True)
    yr = sr + F.interpolate(lr, size=(7, 13), mode='bilinear', align_corners=False)
    dy = torch.randn(3, 36, 7, 13, generator=g)
    yr.backward(dy.double())
    hs, hl = dv(skip.permute(0, 2, 3, 1)).requires_grad_(True), dv(low.permute(0, 2, 3, 1)).requires_grad_(True)
    out = A.upsample_add(hs, hl, batch=3)
    S.add('skip', 'upsample_add_fwd', rel(out.permute(0, 3, 1, 2), yr), 'bilinear')
    out.backward(dv(dy.permute(0, 2, 3, 1)))
    S.add('skip', 'dlow', rel(hl.grad.permute(0, 3, 1, 2), lr.grad), 'bilinear')
    S.add('skip', 'dskip', rel(hs.grad.permute(0, 3, 1, 2), sr.grad), 'bilinear')
    S.finish()


def test_standin_bilinear_adjoints():
    S = Sweep('standin/bilinear_bwd', shrink=0.25)
    resize_check(S, False)
    S.finish(record=False)


# ====================================================================================== 5. decode head backward
LO32, HI32 = float(np.float32(1e-7)), float(np.float32(1) - np.float32(1e-7))       # the kernel's clamp bounds, 1 - 1.19e-7 the upper
DECODE_CASES = [(N, hw, val, grads) for N in (1, 2, 7) for hw in (((5, 7), (20, 28)), ((6, 5), (23, 19)))
                for val in (False, True) for grads in ('logits', 'prob', 'both')]


def decode_forward(l4, valid, Bn, N, out):
    up = F.interpolate(l4.view(Bn, N, *l4.shape[-2:]), size=out, mode='bilinear', align_corners=False)
    p = torch.sigmoid(up)
    p = p * valid[:, 1:, None, None].to(p.dtype) if valid is not None else p
    agg = torch.cat([torch.prod(1 - p, dim=1, keepdim=True), p], 1)
    pc = agg.clamp(LO32, HI32)                     # O.aggregate with the bounds the fp32 kernel has: a double-precision
    lg = torch.log(pc / (1 - pc))                  # 1 - 1e-7 would be a different function
    return agg, lg, F.softmax(lg, dim=1)


def decode_maps(N, hw, with_valid, seed, level):
    (h4, w4), out = hw
    g = torch.Generator().manual_seed(seed)
    Bn = 2
    along_w = w4 >= h4
    size, other = (w4, h4) if along_w else (h4, w4)
    l4 = torch.zeros(Bn, N, h4, w4)
    for b in range(Bn):
        for n in range(N):
            flip = (n + b) % 2
            base = torch.where(torch.arange(size) < size / 2, -level, level) * (1 - 2 * flip)
            o = b % (other - 2)
            m = (base.view(1, -1) if along_w else base.view(-1, 1)).expand(h4, w4) + 0.5 * torch.randn(h4, w4, generator=g)
            for s in (0, size - 3):
                lvl = 25.0 if base[s] < 0 else -25.0              # +25 on the negative background, -25 on the positive
                if along_w:
                    m[o:o + 3, s:s + 3] = lvl
                else:
                    m[s:s + 3, o:o + 3] = lvl
            l4[b, n] = m
    valid = None
    if with_valid:
        valid = torch.ones(Bn, N + 1)
        valid[1, 1 + (N - 1) // 2] = 0
    agg, _, _ = decode_forward(l4.double(), valid, Bn, N, out)
    p, bg = agg[:, 1:], agg[:, :1]
    lo, hi = LO32, 1 - HI32

    def near(t):
        return ((t >= lo / 2) & (t <= lo * 2)) | ((1 - t >= hi / 2) & (1 - t <= hi * 2))
    excl = near(p).any(1, keepdim=True) | near(bg)
    live = p if valid is None else p[valid[:, 1:] > 0.5]
    frac = dict(p_low=float((live < LO32).double().mean()), p_high=float((live > HI32).double().mean()),
                bg_low=float((bg < LO32).double().mean()), excluded=float(excl.double().mean()))
    keep = (~excl).float()
    return dict(N=N, Bn=Bn, out=out, l4=l4.view(Bn * N, h4, w4), valid=valid, frac=frac, seed=(seed, level),
                dl=torch.randn(Bn, N + 1, *out, generator=g) * keep, dp=torch.randn(Bn, N + 1, *out, generator=g) * keep)


def decode_case(N, hw, with_valid):
    """logit4 (2 N, h4, w4): a 3x3 plateau of +25 at one end of the longer axis and one of -25 at the other (the ends swap from one
    object to the next, so that a pixel where some objects vanish holds others that do not), over a background of -level (the half of the +25 plateau) / +level (the
    other half) + 0.5 randn per object -- sigmoid(+-25) lies beyond both clamp bounds, the ramps between plateau and background cross them
    steeply.  The pixels whose float64 p, 1 - p or bg lies within a factor 2 of a bound (where fp32 may take the other branch) get
    dlogits = dprob = 0: they are left out on both sides.  The first (level, seed) that meets the conditions (every branch >= 1 % of the
    pixels, <= 1 % left out; both from the float64 forward alone) is the case."""
    for level in (6.0, 4.0, 5.0, 8.0, 10.0, 20.0, 15.0, 12.0, 25.0, 30.0):
        for seed in range(500, 510):
            k = decode_maps(N, hw, with_valid, seed, level)
            fr = k['frac']
            if min(fr['p_low'], fr['p_high'], fr['bg_low']) >= 0.01 and fr['excluded'] <= 0.01:
                return k
    raise AssertionError('no seed meets the conditions: %s' % (k['frac'],))


def decode_ref(k, grads, dtype, drop=False):
    l4 = leaf(k['l4'], dtype)
    _, lg, prob = decode_forward(l4, k['valid'], k['Bn'], k['N'], k['out'])
    dl, dp = k['dl'].to(dtype), k['dp'].to(dtype)
    if drop:
        dl, dp = dl.clone(), dp.clone()
        dl[:, :, k['out'][0] // 2, k['out'][1] // 2] = 0          # (a pixel of the background between the plateaus)
        dp[:, :, k['out'][0] // 2, k['out'][1] // 2] = 0
    loss = (lg * dl).sum() * (grads != 'prob') + (prob * dp).sum() * (grads != 'logits')
    loss.backward()
    return l4.grad


def decode_hip(k, grads):
    Bn, N, (Ho, Wo) = k['Bn'], k['N'], k['out']
    h4, w4 = k['l4'].shape[-2:]
    d4 = torch.full((Bn * N, h4, w4), float('nan'), device=DEV)
    ws = torch.empty(Bn * N * Ho * Wo, device=DEV)
    l4, valid, dl, dp = dv(k['l4']), dv(k['valid']), dv(k['dl']), dv(k['dp'])      # (held until the call has been made)
    _lib.call('swem_decode_head_bwd_f32', ops._stream(), l4.data_ptr(), ptr(valid), ptr(dl) if grads != 'prob' else 0,
              ptr(dp) if grads != 'logits' else 0, d4.data_ptr(), Bn, N, h4, w4, Ho, Wo, ws.data_ptr(), ws.numel() * 4)
    return d4


def decode_check(S, hip):
    table = {}
    for N, hw, val, grads in DECODE_CASES:
        k = decode_case(N, hw, val)
        tag = (N, hw[0], val, grads)
        want = decode_ref(k, grads, F64)
        stand = rel(decode_ref(k, grads, F32), want)
        table[tag] = (k['seed'], round(k['frac']['excluded'], 4), float('%.2g' % stand))
        S.add(tag, 'finite', bool(torch.isfinite(want).all()))
        if hip:
            S.add(tag, 'dlogit4', rel(decode_hip(k, grads), want), 'heads', standin=stand)
        elif N > 1 and not val and (grads == 'logits' or N == 2):
            S.add(tag, 'dlogit4', stand, 'heads')        # (where fp32 has no reason to be off, it is not)
    print('decode head cases (seed, left out, fp32 ATen vs float64): %s' % table)


@gpu
def test_decode_head_backward_every_clamp_branch(lib):
    """swem_decode_head_bwd_f32 against float64 autograd of bilinear -> sigmoid -> valid -> aggregate -> softmax: N = 1, 2, 7
    (MAXN), two size pairs, valid NULL and with a zero entry, dlogits only / dprob only / both, on maps where every clamp branch
    (p below 1e-7, p above 1 - 1.19e-7, bg below 1e-7) holds >= 1 % of the pixels and <= 1 % sit close enough to a bound to be
    left out (asserted from the reference)."""
    S = Sweep('decode_head_bwd')
    decode_check(S, True)
    S.finish()


def test_standin_decode_head_backward():
    S = Sweep('standin/decode_head_bwd', shrink=0.25)
    decode_check(S, False)
    S.finish(record=False)


# ====================================================================================== 6. pred head, forward and backward
PRED_CASES = [(C, bhw) for C in (4, 8, 64, 256, 1024) for bhw in ((1, 1, 1), (1, 1, 9), (2, 7, 9), (3, 5, 13))]


def pred_case(C, bhw):
    Bn, Hh, Ww = bhw
    g = torch.Generator().manual_seed(600 + C + Bn * Hh * Ww)
    return dict(C=C, bhw=bhw, x=torch.randn(Bn, C, Hh, Ww, generator=g), w=torch.randn(1, C, 3, 3, generator=g) * (2.0 / C) ** 0.5,
                b=torch.randn(1, generator=g), dl=torch.randn(Bn, 1, Hh, Ww, generator=g),
                dw0=torch.randn(1, C, 3, 3, generator=g), db0=torch.randn(1, generator=g))


def pred_ref(k, dtype, drop=False):
    x, w, b = (leaf(k[n], dtype) for n in ('x', 'w', 'b'))
    xin = x
    if drop:                                         # (stand-in whose weight gradient loses the last pixel)
        keep = torch.ones_like(x)
        keep[-1, :, -1, -1] = 0
        xin = x * keep
    y = F.conv2d(F.relu(xin), w, b, padding=1)
    y.backward(k['dl'].to(dtype))
    return dict(logit=y.detach()[:, 0], dx=x.grad, dw=k['dw0'].to(dtype) + w.grad, db=k['db0'].to(dtype) + b.grad)


def pred_hip(k):
    C, (Bn, Hh, Ww) = k['C'], k['bhw']
    x = dv(k['x'].permute(0, 2, 3, 1))
    w = dv(k['w'].permute(0, 2, 3, 1))
    logit = ops.pred_head(x, w, dv(k['b']))
    dx = torch.full_like(x, float('nan'))
    dw, db = dv(k['dw0']), dv(k['db0'])
    wsb = _lib.query('swem_pred_head_bwd_workspace', Bn, Hh, Ww, C)
    ws, dl = torch.empty(wsb // 4, device=DEV), dv(k['dl'])
    _lib.call('swem_pred_head_bwd_f32', ops._stream(), x.data_ptr(), w.data_ptr(), dl.data_ptr(), dx.data_ptr(),
              dw.data_ptr(), db.data_ptr(), Bn, Hh, Ww, C, ws.data_ptr(), wsb)
    return dict(logit=logit, dx=dx.permute(0, 3, 1, 2), dw=dw, db=db)


def pred_check(S, hip):
    for C, bhw in PRED_CASES:
        k = pred_case(C, bhw)
        want = pred_ref(k, F64)
        got = pred_hip(k) if hip else pred_ref(k, F32)
        for n in ('logit', 'dx', 'dw', 'db'):
            S.add((C, bhw), n, rel(got[n], want[n]), 'heads')


@gpu
def test_pred_head_every_lane_count(lib):
    """swem_pred_head_f32 / swem_pred_head_bwd_f32 against float64 conv3x3(relu(x)): C = 4 .. 1024 gives the weight-gradient kernel
    256, 128, 16, 4 and 1 pixel lanes (C = 256 also the matrix-core forward), the maps have 1, 9, 126 and 195 pixels -- fewer than
    one 64-pixel chunk, fewer than the lanes, H = 1, a ragged fourth chunk; dw and db accumulate into non-zero buffers."""
    S = Sweep('pred_head')
    pred_check(S, True)
    S.finish()


def test_standin_pred_head():
    S = Sweep('standin/pred_head', shrink=0.25)
    pred_check(S, False)
    S.finish(record=False)


# ====================================================================================== 7. CBAM, forward and backward
CBAM_NAMES = ['ChannelGate.mlp.1.weight', 'ChannelGate.mlp.1.bias', 'ChannelGate.mlp.3.weight', 'ChannelGate.mlp.3.bias',
              'SpatialGate.spatial.conv.weight', 'SpatialGate.spatial.conv.bias']
CBAM_CASES = [(C, hid, Bn, hw, ties) for (C, hid) in ((8, 4), (72, 6), (512, 32), (1024, 64)) for Bn in (1, 3)
              for hw in ((1, 1), (3, 5), (7, 9)) for ties in (False, True) if not ties or (C <= 72 and hw != (1, 1))]


def first_max(x, dim):
    """max over `dim` (kept) whose gradient goes to the FIRST position that attains it, whatever ATen does with ties."""
    m = x.detach().amax(dim, keepdim=True)
    n = x.shape[dim]
    ar = torch.arange(n).view([n if d == dim else 1 for d in range(x.dim())])
    return x.gather(dim, torch.where(x.detach() == m, ar, n).amin(dim, keepdim=True))


def cbam_first(sd, x):
    """oracle.cbam (attentions.py:22-84) with both max-pools as first_max."""
    def mlp(t):
        t = F.linear(t, sd['a.' + CBAM_NAMES[0]], sd['a.' + CBAM_NAMES[1]])
        return F.linear(F.relu(t), sd['a.' + CBAM_NAMES[2]], sd['a.' + CBAM_NAMES[3]])
    att = mlp(x.flatten(2).mean(2)) + mlp(first_max(x.flatten(2), 2)[..., 0])
    x = x * torch.sigmoid(att)[:, :, None, None]
    comp = torch.cat([first_max(x, 1), x.mean(1, keepdim=True)], 1)
    return x * torch.sigmoid(F.conv2d(comp, sd['a.' + CBAM_NAMES[4]], sd['a.' + CBAM_NAMES[5]], padding=3))


def cbam_case(C, hid, Bn, hw, ties):
    """ties: x on the four levels {-3, -2, -1, 0}: each channel's global maximum is attained at many pixels, and the channel
    maximum of the gated map is 0 = 0 * cscale[c] at every channel that holds a 0 (the gate is positive: the products tie exactly,
    in both precisions)."""
    g = torch.Generator().manual_seed(700 + C + Bn + hw[0] * hw[1] + ties)
    x = torch.randn(Bn, C, *hw, generator=g)
    if ties:
        x = (x * 1.5 - 1.0).round().clamp(-3, 0) + 0.0
    shapes = [(hid, C), (hid,), (C, hid), (C,), (1, 2, 7, 7), (1,)]
    scale = [C ** -0.5, 0.3, hid ** -0.5, 0.3, 0.3, 0.3]
    return dict(C=C, hid=hid, x=x, dy=torch.randn(Bn, C, *hw, generator=g), ties=ties,
                sd={'a.' + n: torch.randn(*s, generator=g) * f for n, s, f in zip(CBAM_NAMES, shapes, scale)},
                g0={n: torch.randn(*s, generator=g) * 0.1 for n, s in zip(CBAM_NAMES, shapes)})


def cbam_ref(k, dtype, drop=False):
    x = leaf(k['x'], dtype)
    sd = {n: leaf(t, dtype) for n, t in k['sd'].items()}
    y = x + (cbam_first(sd, x) if k['ties'] else O.cbam(sd, 'a', x))
    dy = k['dy'].to(dtype)
    if drop:
        dy = dy.clone()
        dy[-1, :, -1, -1] = 0
    y.backward(dy)
    out = dict(y=y.detach(), dx=x.grad)
    out.update({n: k['g0'][n].to(dtype) + sd['a.' + n].grad for n in CBAM_NAMES})
    return out


def cbam_hip(k):
    from swem_amd import autograd as A
    x = dv(k['x'].permute(0, 2, 3, 1)).requires_grad_(True)
    ps = []
    for n in CBAM_NAMES:
        p = torch.nn.Parameter(dv(k['sd']['a.' + n]))
        p.grad = dv(k['g0'][n])
        ps.append(p)
    y = A.cbam_residual(x, *ps)
    y.backward(dv(k['dy'].permute(0, 2, 3, 1)))
    out = dict(y=y.detach().permute(0, 3, 1, 2), dx=x.grad.permute(0, 3, 1, 2))
    out.update({n: p.grad for n, p in zip(CBAM_NAMES, ps)})
    return out


def cbam_check(S, hip):
    for case in CBAM_CASES:
        k = cbam_case(*case)
        want = cbam_ref(k, F64)
        got = cbam_hip(k) if hip else cbam_ref(k, F32)
        S.add(case, 'y', rel(got['y'], want['y']), 'cbam_fwd')
        S.add(case, 'dx' + '_ties' * case[4], rel(got['dx'], want['dx']), 'cbam_dx')
        for n in CBAM_NAMES:
            lone = case == (72, 6, 1, (7, 9), True) and n == CBAM_NAMES[5]
            S.add(case, 'd' + n + '_ties' * case[4], rel(got[n], want[n]), 'cbam_db7_ties_72' if lone else 'cbam_param')


def test_first_max_is_the_oracles_cbam_off_ties_and_first_on_ties():
    """The restated CBAM equals O.cbam (value and all gradients, float64) where nothing ties.  On a tie its gradient goes to the
    first position; what ATen's max_pool2d and max(dim) do there is recorded in the assertion message, not relied upon."""
    k = cbam_case(8, 4, 2, (3, 5), False)
    a = cbam_ref(k, F64)
    b = cbam_ref(dict(k, ties=True), F64)
    assert all(rel(b[n], a[n]) < 1e-13 for n in a), {n: rel(b[n], a[n]) for n in a}
    x = torch.zeros(2, 3, 2, 4, dtype=F64, requires_grad=True)
    first_max(x.flatten(2), 2).sum().backward()
    assert torch.equal(x.grad.flatten(2)[..., 0], torch.ones(2, 3, dtype=F64)) and float(x.grad.sum()) == 6.0
    x.grad = None
    first_max(x, 1).sum().backward()
    assert torch.equal(x.grad[:, 0], torch.ones(2, 2, 4, dtype=F64)) and float(x.grad.sum()) == 16.0
    xa = torch.zeros(1, 3, 2, 4, dtype=F64, requires_grad=True)
    F.max_pool2d(xa, (2, 4), stride=(2, 4)).sum().backward()
    pool_first = bool(torch.equal(xa.grad.flatten(2)[..., 0], torch.ones(1, 3, dtype=F64)) and float(xa.grad.sum()) == 3.0)
    xa.grad = None
    xa.max(1, keepdim=True)[0].sum().backward()
    max_first = bool(torch.equal(xa.grad[:, 0], torch.ones(1, 2, 4, dtype=F64)) and float(xa.grad.sum()) == 8.0)
    print('ATen sends a tie to the first position: max_pool2d %s, max(dim) %s' % (pool_first, max_first))


@gpu
def test_cbam_small_maps_ties_and_the_general_mlp(lib):
    """swem_cbam_f32 / swem_cbam_bwd_f32 against the float64 oracle: C = 8 (below a 64-channel block), 72 (across one; hid = 6:
    the general MLP kernel), 512 (the training shape), 1024 (general kernel); maps of 1, 15 and 63 pixels (fewer than the 16 pixel
    lanes, fewer than the 32 chunks: empty chunks with a -inf maximum); B = 1 and 3; and maps FULL of ties in both maxima, where
    the gradient must reach the first position."""
    S = Sweep('cbam')
    cbam_check(S, True)
    S.finish()


def test_standin_cbam():
    S = Sweep('standin/cbam', shrink=0.25)
    cbam_check(S, False)
    S.finish(record=False)


# ====================================================================================== 8. loss kernels
LOSS_HW = [1, 255, 256, 257, 1023, 1025, 5000]
LOSS_CONFIGS = [(1, 2, None), (3, 2, None), (1, 3, None), (3, 3, None), (1, 3, [[1, 1, 0]]), (1, 3, [[1, 0, 1]]),
                (3, 3, [[1, 1, 1], [1, 1, 0], [1, 0, 1]]), (1, 8, None), (3, 8, None)]
AUX_RATIO = 0.5
GAP = 1e-4
GAP_ABS = 1e-6      # (fp32 resolves a cross entropy log(1 + e) to 6e-8 absolute, whatever its size)


def loss_ref(logits, label, valid, k, aux_ratio, gout, dtype, drop=False):
    """losses/__init__.py:34-63 for one frame (T = 1), written out so that the pixels EQUAL to the k-th largest cross entropy
    share the k - #above slots evenly (include/swem_hip_train.h); without a tie this is torch.topk's autograd
    (test_loss_restatement_is_the_oracle).  Returns the tensors the three entry points produce."""
    Bn, N1, HW = logits.shape
    lg = leaf(logits, dtype)
    prob, raw = torch.zeros(Bn, N1, HW, dtype=dtype), torch.zeros(Bn, HW, dtype=dtype)
    iou, stat = torch.zeros(Bn, N1, 2, dtype=dtype), torch.zeros(Bn, 4, dtype=dtype)
    iou[..., 1] = 1e-6
    main, aux, weights = 0.0, 0.0, []
    for b in range(Bn):
        ok = torch.ones(N1, dtype=torch.bool) if valid is None else valid[b] > 0.5
        lsm = F.log_softmax(lg[b][ok], 0)
        p = lsm.exp()
        oh = F.one_hot(label[b], int(ok.sum())).t().to(dtype)
        r = -lsm.gather(0, label[b][None])[0]
        inter, union = torch.min(p, oh).sum(1), torch.max(p, oh).sum(1) + 1e-6
        aux = aux + 1.0 - (inter / union).sum() / int(ok.sum())
        rd = r.detach()
        if k > 0:
            thr = rd.sort(descending=True)[0][k - 1]
            above, eq = rd > thr, rd == thr
            w = above.to(dtype) + eq.to(dtype) * (k - int(above.sum())) / int(eq.sum())
            stat[b] = torch.stack([thr, above.sum().to(dtype), rd[above].sum(), eq.sum().to(dtype)])
        else:
            w = torch.ones(HW, dtype=dtype)
            stat[b] = torch.stack([rd.sum() * 0, rd.sum() * 0 + HW, rd.sum(), rd.sum() * 0])
        if drop and b == Bn - 1:
            w = w.clone()
            w[rd.argmax()] = 0                      # (stand-in that loses the row's hardest pixel)
        main = main + (w * r).sum() / (k if k > 0 else HW)
        weights.append(w)
        prob[b][ok], raw[b] = p.detach(), rd
        iou[b][ok] = torch.stack([inter, union], 1).detach()
    main, aux = main / Bn, aux / Bn
    total = main + aux_ratio * aux
    (total * gout).backward()
    return dict(prob=prob, raw=raw, iou=iou, rowstat=stat, losses=torch.stack([total, main, aux]).detach(), dlogits=lg.grad,
                weights=torch.stack(weights))


def loss_hip(logits, label, valid, k, aux_ratio, gout):
    Bn, N1, HW = logits.shape
    st, nan = ops._stream(), float('nan')
    lg, lb, vd = dv(logits), dv(label), dv(valid)
    prob, raw = torch.full((Bn, N1, HW), nan, device=DEV), torch.full((Bn, HW), nan, device=DEV)
    stat, iou = torch.full((Bn, 4), nan, device=DEV), torch.full((Bn, N1, 2), nan, device=DEV)
    losses, dl = torch.full((3,), nan, device=DEV), torch.full((Bn, N1, HW), nan, device=DEV)
    wsb = _lib.query('swem_vos_loss_workspace', Bn, N1, HW)
    ws = torch.empty(wsb // 4, device=DEV)
    go = torch.tensor([gout], device=DEV) if gout != 1.0 else None
    _lib.call('swem_vos_loss_frame_fwd_f32', st, lg.data_ptr(), lb.data_ptr(), HW, ptr(vd), prob.data_ptr(), raw.data_ptr(),
              stat.data_ptr(), iou.data_ptr(), Bn, N1, HW, k, 0, ws.data_ptr(), wsb)
    _lib.call('swem_vos_loss_reduce_f32', st, stat.data_ptr(), iou.data_ptr(), ptr(vd), losses.data_ptr(), Bn, N1, 1, HW, k, 0,
              aux_ratio)
    _lib.call('swem_vos_loss_frame_bwd_f32', st, prob.data_ptr(), raw.data_ptr(), lb.data_ptr(), HW, ptr(vd), stat.data_ptr(),
              iou.data_ptr(), dl.data_ptr(), Bn, N1, 1, HW, k, 0, aux_ratio, ptr(go))
    return dict(prob=prob, raw=raw, iou=iou, rowstat=stat, losses=losses, dlogits=dl)


def loss_inputs(Bn, N1, HW, valid, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(Bn, N1, HW, generator=g) * 3
    v = None if valid is None else torch.tensor(valid, dtype=F32)
    nv = [N1 if v is None else int((v[b] > 0.5).sum()) for b in range(Bn)]
    label = torch.stack([torch.randint(0, nv[b], (HW,), generator=g) for b in range(Bn)])
    return logits, label, v


def gaps_ok(raw64, ks):
    """the k-th largest cross entropy of every row is >= GAP (relative; and >= GAP_ABS) away from its neighbours on both sides: fp32 cannot
    reorder, merge or split the values at the threshold, so the counts are comparable exactly"""
    s = raw64.sort(dim=1, descending=True)[0]
    HW = s.shape[1]
    for k in ks:
        if k == 0:
            continue
        for lo, hi in ((k - 2, k - 1), (k - 1, k)):
            if lo >= 0 and hi < HW and bool(((s[:, lo] - s[:, hi]) < (GAP * s[:, lo].abs()).clamp(min=GAP_ABS)).any()):
                return False
    return True


def loss_case(Bn, N1, HW, valid):
    """the first seed whose float64 cross entropies keep the gap condition at every k of the case"""
    ks = sorted({0, 1, HW // 3, HW})
    for seed in range(800 + HW, 800 + HW + 400):
        logits, label, v = loss_inputs(Bn, N1, HW, valid, seed)
        if gaps_ok(loss_ref(logits, label, v, 0, AUX_RATIO, 1.0, F64)['raw'], ks):
            return logits, label, v, ks
    raise AssertionError('no seed keeps the gap condition')


def loss_compare(S, tag, got, want, exact_counts=True, bar='loss', value_bar=None):
    nan = any(bool(torch.isnan(got[n]).any()) for n in ('prob', 'raw', 'iou', 'rowstat', 'losses', 'dlogits'))
    S.add(tag, 'nothing_nan', not nan)
    value_bar = value_bar or bar
    for n in ('prob', 'raw', 'iou'):
        S.add(tag, n, rel(got[n], want[n]), bar if n == 'raw' else 'loss')
    gs, ws_ = got['rowstat'].double().cpu(), want['rowstat'].double()
    scale = float(want['raw'].abs().max()) + 1e-30
    S.add(tag, 'threshold', float((gs[:, 0] - ws_[:, 0]).abs().max()) / scale, bar)
    if exact_counts:
        S.add(tag, 'counts_exact', bool(torch.equal(gs[:, 1], ws_[:, 1]) and torch.equal(gs[:, 3], ws_[:, 3])))
        S.add(tag, 'sum_above', rel(gs[:, 2], ws_[:, 2]), bar)
    gl, wl = got['losses'].double().cpu(), want['losses'].double()
    S.add(tag, 'loss_values', float(((gl - wl).abs() / wl.abs()).max()), value_bar)
    S.add(tag, 'dlogits', rel(got['dlogits'], want['dlogits']), 'dlogits')


def loss_check(S, HW, hip):
    for Bn, N1, valid in LOSS_CONFIGS:
        logits, label, v, ks = loss_case(Bn, N1, HW, valid)
        for k in ks:
            gout = 1.0 if k == 1 else 0.375                        # (a device scalar other than 1, exact in fp32)
            want = loss_ref(logits, label, v, k, AUX_RATIO, gout, F64)
            got = loss_hip(logits, label, v, k, AUX_RATIO, gout) if hip else loss_ref(logits, label, v, k, AUX_RATIO, gout, F32)
            loss_compare(S, (HW, Bn, N1, valid, k), got, want, bar='loss_hw1_raw' if HW == 1 else 'loss',
                         value_bar='loss_hw1_values' if HW == 1 else 'loss')


def test_loss_restatement_is_the_oracle():
    """loss_ref is O.vos_loss (values and d/d logits, float64) on a clip of one frame, below start_warm (k = 0) and above
    end_warm (k = int(HW * 0.3)), with and without an invalid middle channel."""
    cfg = dict(NAME='boots_ce', BS_RATIO=0.30, BS_PERIOD=[20, 70], AUX='iou', AUX_RATIO=AUX_RATIO)
    for valid in (None, [[1, 1, 1], [1, 0, 1]]):
        logits, label, v = loss_inputs(2, 3, 6 * 7, valid, 5)
        for it, k in ((5, 0), (90, int(42 * 0.3))):
            sc = logits.double().view(2, 3, 1, 6, 7).requires_grad_(True)
            ref = O.vos_loss(sc, label.view(2, 1, 6, 7), it, v, cfg)
            ref['total_loss'].backward()
            mine = loss_ref(logits, label, v, k, AUX_RATIO, 1.0, F64)
            assert abs(float(mine['losses'][0]) - float(ref['total_loss'])) < 1e-13
            assert abs(float(mine['losses'][1]) - float(ref['main_loss'])) < 1e-13
            assert rel(mine['dlogits'], sc.grad.view(2, 3, 42)) < 1e-12


@gpu
@pytest.mark.parametrize('HW', LOSS_HW)
def test_loss_kernels_vs_float64(lib, HW):
    """swem_vos_loss_frame_fwd_f32 / _reduce_f32 / _frame_bwd_f32 through the C ABI with an explicit k in {0, 1, HW // 3, HW}:
    rows shorter than one 256-pixel block and than the select's 1024 threads, on both sides of each; B = 1, 3; N1 = 2, 3, 8
    (LOSS_MAXC); valid NULL, [1,1,0], [1,0,1] (the invalid MIDDLE channel: labels index the valid channels) and the three mixed
    in one batch; gout 1 and not.  prob, raw, iou, the four row statistics (the two counts exactly), the three loss values and
    dlogits against float64, on seeds whose k-th cross entropy is >= 1e-4 (relative) away from its neighbours."""
    S = Sweep('loss[HW=%d]' % HW)
    loss_check(S, HW, True)
    S.finish()


@pytest.mark.parametrize('HW', LOSS_HW)
def test_standin_loss(HW):
    S = Sweep('standin/loss[HW=%d]' % HW, shrink=0.25)
    loss_check(S, HW, False)
    S.finish(record=False)


def tie_case(dup, HW, N1, seed):
    """rows of HW pixels made of HW / dup distinct pixels, each `dup` times (shuffled): every cross entropy value occurs dup times
    in both precisions"""
    logits, label, _ = loss_inputs(2, N1, HW // dup, None, seed)
    perm = torch.randperm(HW, generator=torch.Generator().manual_seed(seed))
    return logits.repeat(1, 1, dup)[:, :, perm].contiguous(), label.repeat(1, dup)[:, perm].contiguous()


def tie_check(S, hip):
    for dup, HW, N1 in ((2, 600, 3), (4, 1200, 2), (4, 5000, 8)):
        logits, label = tie_case(dup, HW, N1, 900 + HW)
        for k in sorted({dup * (HW // (3 * dup)) + j for j in range(1, dup)}):        # strictly inside a tie group
            for aux_ratio in (AUX_RATIO, 0.0):
                want = loss_ref(logits, label, None, k, aux_ratio, 1.0, F64)
                got = loss_hip(logits, label, None, k, aux_ratio, 1.0) if hip else loss_ref(logits, label, None, k, aux_ratio, 1.0, F32)
                tag = (dup, HW, N1, k, aux_ratio)
                S.add(tag, 'tie_is_in_the_reference', bool((want['rowstat'][:, 3] == dup).all() and (want['rowstat'][:, 1] == k - k % dup).all()))
                loss_compare(S, tag, got, want)
                if aux_ratio == 0.0:
                    # without the IoU term dlogits[target] = w (p_t - 1) / (k B T): the weights of the tied pixels sum to k - cnt
                    p_t = want['prob'].gather(1, label[:, None])[:, 0]
                    w = got['dlogits'].double().cpu().gather(1, label[:, None])[:, 0] / (p_t - 1) * (k * 2)
                    tied = want['raw'] == want['rowstat'][:, :1]
                    S.add(tag, 'tied_weights_sum', float(((w * tied).sum(1) - (k - want['rowstat'][:, 1])).abs().max()) / (k % dup), 'dlogits')


@gpu
def test_loss_ties_at_the_threshold_share_evenly(lib):
    """Rows built from duplicated pixels, k strictly inside a tie group (eq = 2 and 4, k - cnt = 1, 2, 3): the loss value is the
    float64 top-k mean, dlogits the float64 formula with the documented even sharing, the tied weights add up to k - cnt."""
    S = Sweep('loss_ties')
    tie_check(S, True)
    S.finish()


def zero_case(HW, N1, seed):
    """90 % of the pixels carry their label's logit 30 above the others: exp(-30) vanishes against 1 in fp32, the cross entropy is
    exactly 0 there (1e-13 in float64); k = HW // 3 reaches into them: the threshold is 0, shared by 0.9 HW pixels."""
    logits, label, _ = loss_inputs(2, N1, HW, None, seed)
    sure = torch.rand(2, HW, generator=torch.Generator().manual_seed(seed)) < 0.9
    hot = F.one_hot(label, N1).permute(0, 2, 1).float() * 30.0
    return torch.where(sure[:, None], hot, logits).contiguous(), label


def zero_check(S, hip):
    for HW, N1 in ((300, 2), (1025, 3), (5000, 8)):
        logits, label = zero_case(HW, N1, 950 + HW)
        for k in (HW // 3, HW):
            want = loss_ref(logits, label, None, k, AUX_RATIO, 1.0, F64)
            got = loss_hip(logits, label, None, k, AUX_RATIO, 1.0) if hip else loss_ref(logits, label, None, k, AUX_RATIO, 1.0, F32)
            zero = float((got['raw'] == 0).float().mean())
            S.add((HW, N1, k), 'zero_rows_are_exact_zeros', bool(0.85 < zero < 0.95 and float(got['rowstat'][:, 0].abs().max()) == 0.0))
            loss_compare(S, (HW, N1, k), got, want, exact_counts=False, value_bar='loss_zero_300' if HW == 300 else 'loss')


@gpu
def test_loss_zero_threshold_rows(lib):
    """Rows whose k-th largest cross entropy is exactly 0 (and whose zeros are -0.0 in the kernel: -(0 - 0)): the select finds the
    threshold, the 0.9 HW pixels equal to it share what is left of k, the loss values and dlogits are the float64 ones, nothing
    is NaN."""
    S = Sweep('loss_zero_threshold')
    zero_check(S, True)
    S.finish()


def test_standin_loss_ties_and_zero_rows():
    S = Sweep('standin/loss_ties', shrink=0.25)
    tie_check(S, False)
    zero_check(S, False)
    S.finish(record=False)


# ====================================================================================== 9. AdamW, GLU, add, value-input packing
ADAM = dict(lr=2.0 ** -10, b1=float(np.float32(0.9)), b2=float(np.float32(0.999)), eps=float(np.float32(1e-8)), wd=2.0 ** -3)


def adam_case(n, seed):
    """|p| in [1.1, 1.9] on a 2^-10 grid: p (1 - lr wd) = p - p 2^-13 is exact in fp32 and no update leaves the binade, so the
    kernel's p carries ONE rounding (the final subtraction, 0.5 ulp) plus the update's own error (a few ulp of 1e-3: 0.01 ulp of
    p) -- the 1 ulp bar has a factor 2 of room and no more."""
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand(n, generator=g) * 0.8 + 1.1) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    p = (p * 1024).round() / 1024
    return dict(p=p, g=torch.randn(n, generator=g) * 10.0 ** -(torch.arange(n) % 3).float(), m=torch.randn(n, generator=g) * 0.1,
                v=torch.rand(n, generator=g) * 0.01 + 1e-4)


def adam_ref(k, step, dtype):
    a = ADAM
    p, g, m, v = (k[n].to(dtype) for n in 'pgmv')
    m = a['b1'] * m + (1 - a['b1']) * g
    v = a['b2'] * v + (1 - a['b2']) * g * g
    bc1, bc2 = 1 - a['b1'] ** step, 1 - a['b2'] ** step
    p = p * (1 - a['lr'] * a['wd']) - (a['lr'] / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + a['eps']))
    return p, m, v


def adam_hip(k, step, gate=None, applied=None, plain=False):
    a = ADAM
    t = {n: dv(k[n]) for n in 'pgmv'}
    args = (ops._stream(), t['p'].data_ptr(), t['g'].data_ptr(), t['m'].data_ptr(), t['v'].data_ptr(), k['p'].numel(), a['lr'], a['b1'],
            a['b2'], a['eps'], a['wd'], step)
    if plain:
        _lib.call('swem_adamw_f32', *args)
    else:
        _lib.call('swem_adamw_gated_f32', *args, ptr(gate), 0 if gate is None else gate.numel(), ptr(applied))
    return t['p'], t['m'], t['v']


ADAM_N = (1, 2, 3, 4, 5, 1023, 1024, 1027)


def adam_check(S, hip):
    for n in ADAM_N:
        for step in (1, 1000):
            k = adam_case(n, 960 + n + step)
            want = adam_ref(k, step, F64)
            got = adam_hip(k, step, plain=True) if hip else adam_ref(k, step, F32)
            # (no fp32 arithmetic is 4x under ONE ulp: the stand-in is held to the single rounding adam_case leaves, 0.5 ulp + the
            # update's own error)
            S.add((n, step), 'p_ulp', ulps(got[0], want[0]), 'adam_p_ulp', shrink=1.0 if hip else 0.52)
            S.add((n, step), 'm', rel(got[1], want[1]), 'adam_mv')
            S.add((n, step), 'v', rel(got[2], want[2]), 'adam_mv')


@gpu
def test_adamw_vs_float64_and_the_gate(lib):
    """swem_adamw_f32 at every tail of the float4 body (n = 1 .. 5, 1023, 1024, 1027) and at step 1 and 1000 (both bias
    corrections): p within one fp32 ulp of the float64 update, m and v within 1e-6.  swem_adamw_gated_f32: a non-zero flag in
    slot 0 or slot 1 leaves p, m, v and `applied` bit-unchanged; an all-zero gate is the ungated call bit for bit and counts."""
    S = Sweep('adamw')
    adam_check(S, True)
    for n in ADAM_N:
        k = adam_case(n, 990 + n)
        plain = adam_hip(k, 7, plain=True)
        for slot in (0, 1):
            gate = torch.zeros(2, device=DEV)
            gate[slot] = 1.0
            applied = torch.full((1,), 5, dtype=torch.int32, device=DEV)
            got = adam_hip(k, 7, gate, applied)
            S.add((n, 'gate', slot), 'closed_gate_touches_nothing',
                  bool(all(torch.equal(got[i].cpu(), k[c]) for i, c in enumerate('pmv')) and int(applied) == 5))
        applied = torch.full((1,), 5, dtype=torch.int32, device=DEV)
        got = adam_hip(k, 7, torch.zeros(2, device=DEV), applied)
        S.add((n, 'gate', 'open'), 'open_gate_is_the_plain_call', bool(all(torch.equal(got[i], plain[i]) for i in range(3)) and int(applied) == 6))
        got = adam_hip(k, 7, None, None)
        S.add((n, 'gate', None), 'no_gate_is_the_plain_call', bool(all(torch.equal(got[i], plain[i]) for i in range(3))))
    S.finish()


def test_standin_adamw():
    S = Sweep('standin/adamw', shrink=0.25)
    adam_check(S, False)
    S.finish(record=False)


def glu_case(n):
    g = torch.Generator().manual_seed(970 + n)
    f, a, dy = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    a[:2] = torch.tensor([30.0, -100.0])                          # saturated gates: exp(100) overflows fp32
    if n > 4:
        a[2:4] = torch.tensor([100.0, -30.0])
        a[-2:] = torch.tensor([-100.0, 30.0])                     # ... also in the second block's only live lane
    return f, a, dy


def glu_ref(f, a, dy, dtype):
    f, a, dy = f.to(dtype), a.to(dtype), dy.to(dtype)
    s = torch.sigmoid(a)
    return f * s, dy * s, dy * f * s * (1 - s)


def glu_check(S, hip):
    for n in (4, 1028):
        f, a, dy = glu_case(n)
        want = glu_ref(f, a, dy, F64)
        if hip:
            fd, ad, dyd = dv(f), dv(a), dv(dy)
            y, df, da = (torch.full((n,), float('nan'), device=DEV) for _ in range(3))
            _lib.call('swem_glu_f32', ops._stream(), fd.data_ptr(), ad.data_ptr(), y.data_ptr(), n)
            _lib.call('swem_glu_bwd_f32', ops._stream(), dyd.data_ptr(), fd.data_ptr(), ad.data_ptr(), df.data_ptr(), da.data_ptr(), n)
            got = (y, df, da)
        else:
            got = glu_ref(f, a, dy, F32)
        S.add(n, 'finite', bool(all(torch.isfinite(t).all() for t in got)))
        for name, t, w in zip(('y', 'df', 'da'), got, want):
            S.add(n, name, rel(t, w), 'glu')


@gpu
def test_glu_add_and_value_input_packing(lib):
    """swem_glu_f32 / swem_glu_bwd_f32 with gates of +-30 and +-100 (finite, within 2e-6 of float64); swem_add_f32 and
    swem_prep_value_input_bwd_f32 (single_obj 0 and 1, N = 1 and 3, one pixel and 323) bit-equal to the same fp32 operations."""
    S = Sweep('glu_add_prep')
    glu_check(S, True)
    g = torch.Generator().manual_seed(980)
    for n in (4, 1028):
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        y, ad, bd = torch.full((n,), float('nan'), device=DEV), dv(a), dv(b)
        _lib.call('swem_add_f32', ops._stream(), ad.data_ptr(), bd.data_ptr(), y.data_ptr(), n)
        S.add(n, 'add_exact', torch.equal(y.cpu(), a + b))
    for single in (0, 1):
        for N in (1, 3):
            for Hh, Ww in ((1, 1), (17, 19)):
                dxin = torch.randn(2 * N, Hh, Ww, 8, generator=g)
                dm, dxd = torch.full((2, N + 1, Hh, Ww), float('nan'), device=DEV), dv(dxin)
                _lib.call('swem_prep_value_input_bwd_f32', ops._stream(), dxd.data_ptr(), dm.data_ptr(), 2, N, Hh, Ww, single)
                gm, go = dxin.view(2, N, Hh, Ww, 8)[..., 3], dxin.view(2, N, Hh, Ww, 8)[..., 4] * (1 - single)
                bg = torch.zeros(2, Hh, Ww)
                for n in range(N):                               # (the kernel's order: 0 - o_0 - o_1 - ...)
                    bg = bg - go[:, n]
                S.add((single, N, Hh * Ww), 'prep_value_bwd_exact', torch.equal(dm.cpu(), torch.cat([bg[:, None], gm - go], 1)))
    S.finish()


def test_standin_glu():
    S = Sweep('standin/glu', shrink=0.25)
    glu_check(S, False)
    S.finish(record=False)


# ====================================================================================== refusals ahead of the first launch
@gpu
def test_refused_shapes_leave_their_outputs_untouched(lib):
    """swem_pred_head_bwd_f32 refuses C = 96 (C / 4 = 24 does not divide the 256 threads into pixel lanes) and swem_cbam_bwd_f32
    C = 2048 (9 C + 4 hid floats of LDS > 64 KB) with SWEM_E_SHAPE BEFORE any kernel of the call has run: the NaN-prefilled
    outputs are still NaN everywhere."""
    nan, st = float('nan'), ops._stream()
    C, Bn, Hh, Ww = 96, 2, 3, 5
    x, w, dl = torch.randn(Bn, Hh, Ww, C, device=DEV), torch.randn(1, 3, 3, C, device=DEV), torch.randn(Bn, Hh, Ww, device=DEV)
    outs = [torch.full((Bn, Hh, Ww, C), nan, device=DEV), torch.full((1, C, 3, 3), nan, device=DEV), torch.full((1,), nan, device=DEV)]
    wsb = _lib.query('swem_pred_head_bwd_workspace', Bn, Hh, Ww, C)
    ws = torch.empty(wsb // 4, device=DEV)
    with pytest.raises(_lib.SwemHipError, match=r'swem_pred_head_bwd_f32 failed \(-1\)'):
        _lib.call('swem_pred_head_bwd_f32', st, x.data_ptr(), w.data_ptr(), dl.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                  outs[2].data_ptr(), Bn, Hh, Ww, C, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    pred_clean = all(bool(torch.isnan(t).all()) for t in outs)
    C, hid, Bn, Hh, Ww = 2048, 128, 1, 2, 3
    x, dy = torch.randn(Bn, Hh, Ww, C, device=DEV), torch.randn(Bn, Hh, Ww, C, device=DEV)
    shapes = [(hid, C), (hid,), (C, hid), (C,), (1, 2, 7, 7), (1,)]
    ps = [torch.randn(*s, device=DEV) * 0.1 for s in shapes]
    outs = [torch.full((Bn, Hh, Ww, C), nan, device=DEV)] + [torch.full(s, nan, device=DEV) for s in shapes]
    wsb = _lib.query('swem_cbam_bwd_workspace', Bn, Hh, Ww, C)
    ws = torch.empty(wsb // 4, device=DEV)
    with pytest.raises(_lib.SwemHipError, match=r'swem_cbam_bwd_f32 failed \(-1\)'):
        _lib.call('swem_cbam_bwd_f32', st, x.data_ptr(), *[p.data_ptr() for p in ps], dy.data_ptr(), *[o.data_ptr() for o in outs],
                  Bn, Hh, Ww, C, hid, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    cbam_clean = all(bool(torch.isnan(t).all()) for t in outs)
    H.record_parity('train_edges/refusals', {'pred_head_bwd_C96_outputs_untouched': pred_clean, 'cbam_bwd_C2048_outputs_untouched': cbam_clean})
    assert pred_clean, 'pred_head_bwd wrote before it refused'
    assert cbam_clean, 'cbam_bwd wrote before it refused'


# ====================================================================================== what a bar is worth
def test_standin_with_a_dropped_element_misses_the_bars():
    """Once per sweep, at its largest case: the fp32 stand-in with ONE row / pixel / chunk left out lies far beyond the bar (the
    ratios are in the module docstring) -- the bars separate arithmetic from indexing."""
    ratio = {}
    k = bn_case(40000, 64)
    y32 = bn_fwd64(k, 1, 0).float()
    got, want = EmuBN(k, drop=True).bwd(y32, 1, False, ('gamma', 'beta')), bn_bwd64(k, y32, 1)
    ratio['bn dbeta (40000, 64)'] = rel(got['dbeta'], want['dbeta']) / BARS['dbeta']
    k = bn_case(600000, 4)
    ratio['colsum (600000, 4)'] = rel(EmuBN(k, drop=True).colsum('dy', None, 1, 0, 0)[0], k['dy'].double().sum(0)) / BARS['colsum']
    dy = torch.randn(2, 4, 107, 107, generator=torch.Generator().manual_seed(1))
    ratio['bilinear 27 -> 107'] = rel(resize_ref(dy, 27, 27, F32, drop=True), resize_ref(dy, 27, 27, F64)) / BARS['bilinear_27_107']
    k = pred_case(1024, (3, 5, 13))
    ratio['pred head dw C=1024'] = rel(pred_ref(k, F32, drop=True)['dw'], pred_ref(k, F64)['dw']) / BARS['heads']
    k = cbam_case(1024, 64, 3, (7, 9), False)
    n = CBAM_NAMES[0]
    ratio['cbam dw1 (1024, 64, 7x9)'] = rel(cbam_ref(k, F32, drop=True)[n], cbam_ref(k, F64)[n]) / BARS['cbam_param']
    k = decode_case(2, ((5, 7), (20, 28)), False)
    ratio['decode head N=2'] = rel(decode_ref(k, 'both', F32, drop=True), decode_ref(k, 'both', F64)) / BARS['heads']
    logits, label, v, _ = loss_case(3, 8, 5000, None)
    ratio['loss dlogits HW=5000'] = rel(loss_ref(logits, label, v, 1666, AUX_RATIO, 1.0, F32, drop=True)['dlogits'],
                                        loss_ref(logits, label, v, 1666, AUX_RATIO, 1.0, F64)['dlogits']) / BARS['dlogits']
    print('one dropped element / bar: %s' % {n: round(r, 1) for n, r in ratio.items()})
    assert min(ratio.values()) > 10, ratio
