"""GPU: the three entry points only training calls -- swem_match_bwd_f32 (csrc/match.hip), swem_nu_update_bwd_f32 and
swem_memorize_train_f32 (csrc/em.hip) -- against float64 at the corners tests/test_gpu_train.py does not reach: P = 1 .. 577 (below,
on and past the 128-row pad, several GEMM row tiles, training's own 576), every group shape of the d qn GEMM (N = 1 .. 7: a partial
group, a full one, full + 1 with the re-pack into the second half of the mknT slot, two full, two full + 1), C = 64 / 128, all four
Lm with one bank and two, V = 4 .. 512, tau = 1, dS NULL, dmem all zero, topl = 1, 5, 32, 64 (= Lm and at Lm = 512), stale
workspaces, non-zero pad rows of dmem, every refusal, one-hot responsibilities at the pad edges, z_out against the forward that
made it, three clips through swem_amd.autograd.

Conventions are those of tests/test_gpu_train_edges.py.  Every comparison goes through the C ABI (_lib.call) with identical fp32
inputs on both sides; the reference is float64 (the oracle's get_affinity / e_step under torch autograd on .double() inputs, or the
two-line value update restated below).  Errors are measured the way test_gpu_train.close does (max error over max |reference|)
and are printed and recorded under match_bwd_edges/<kernel> (helpers.record_parity) before anything is asserted.

Bars (BARS): S, mem_out, d nu 1e-4 and d qk max(3 x the fp32 CPU oracle's own distance to float64 on the same pixels, 2e-4 x scale)
-- test_match_backward's; z 1e-4, nu (mass-weighted) and zita 1e-4 -- tests/test_gpu_em_edges.py's; the value update's backward has
no project bar: 8x the worst of its fp32 stand-in over the sweep (below).

Every GPU sweep exists a second time as test_standin_* (no GPU): the SAME cases with fp32 torch on the CPU standing in for the kernel
(the oracle under autograd; torch.matmul for the value update), at least 4x under every fixed bar.  Worst stand-in error / bar, and
what the kernels measured on an MI355X beside it:
    readout path (dS NULL, every pixel)  S 8.2e-6, mem_out 5.2e-6, d nu 9.7e-6 / 1e-4, d qk 3.5e-6 / 2e-4 of its scale
                                 kernel  S 6.8e-6, mem_out 4.7e-6, d nu 8.5e-6, d qk 3.5e-6 (0.018 of max(3 err_cpu_fp32, 2e-4 scale))
    top-l path (near ties left out)      S 1.4e-6, mem_out 1.2e-6, d nu 2.0e-6 / 1e-4, d qk 1.3e-6 / 2e-4 of its scale
                                 kernel  S 1.3e-6, mem_out 1.4e-6, d nu 2.0e-6, d qk 1.0e-6 (0.005 of its bar); d nu exactly 0 with dmem = 0
    value update backward                dv 7.4e-7 at (577, 5, 512, 128) -> bar 6.0e-6, dnu_prev 7.5e-8 at (129, 7, 512, 64) -> bar 6.1e-7
                                 kernel  dv 4.5e-7, dnu_prev 7.5e-8; one-hot probes 9.0e-8
    E step of the prior (T = 1)          z 3.4e-5 / 1e-4 (the fp32 oracle at C = 128 is 2.9x under, not 4x: the bar is test_ew_vs_float64's
                                         and stays; test_standin_memorize_estep asserts 2x)
                                 kernel  z 3.4e-5; nu from the returned z_out 1.0e-7, zita 9.4e-8 / 1e-4
V = 4 in swem_match_bwd_f32 and L = 32 in swem_nu_update_bwd_f32 are accepted and right (status 0, inside the sweeps' bars).
Bit-equal on the MI355X: both backward entries on a 0xFF-filled workspace against a zeroed one, swem_match_bwd_f32 with dmem's pad
rows at 3.0 against zero, memorize_train's bases against swem_memorize_f32's, three clips through autograd against three calls (30
tensors); the eleven refusals return their own status with every output untouched.
No case needs a bar of its own.  Share of the pixels the top-l sweep compares (pixels whose sorted float64 affinities come within 5e-6
logit units are discontinuities of d qk; wanted >= 0.75, from the reference alone): 0.822 at (P 129, N 7, C 128, Lm 512, topl 64),
0.849 at (577, 7, 128, 512, 64), 0.969 at (129, 4, 64, Lm 64, topl 64), >= 0.98 everywhere else.
What a bar is worth (test_standin_with_a_dropped_element_misses_the_bars, each sweep's largest case, P = 577 with seven objects and
Lm = 512): one pixel's row of dmem zeroed puts d nu 690x (readout sweep) / 1200x (top-l sweep) beyond its bar, one object left out of
the d qk sum 1900x / 4000x; one pixel of z left out of the value update at (577, 7, 32, 256) 1.0e5x."""
import functools

import pytest
import torch

from oracle import swem_oracle as O
from swem_amd import _lib, ops
from tests import helpers as H
from tests.test_gpu_em_edges import near_data_bases, pad128, z_to_oracle

gpu = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
TAU = 0.05
E_SHAPE, E_WORKSPACE, E_ARG = -1, -2, -4                       # include/swem_hip.h

BARS = {'S': 1e-4, 'mem': 1e-4, 'dnu': 1e-4,                   # test_gpu_train.test_match_backward
        'dqk': 2e-4,                                           # ... the fixed part of max(3 err_cpu_fp32, 2e-4 scale)
        'z': 1e-4, 'nu': 1e-4, 'zita': 1e-4,                   # test_gpu_em_edges: test_ew_vs_float64, test_memorize_vs_float64
        # swem_nu_update_bwd_f32 has no bar of its own elsewhere: 8x the worst of the fp32 CPU stand-in (torch.matmul of the same
        # operation against float64) over NU_CASES -- dv 7.43e-7 at (577, 5, 512, 128), dnu_prev 7.52e-8 at (129, 7, 512, 64) -- the
        # margin covers the conv kernel's accumulation order over a reduction of at most 512 (test_standin_nu_update_backward
        # asserts that the stand-in still sits 8x under)
        'nu_dv': 6.0e-6, 'nu_dprev': 6.1e-7}
KEPT = 0.75                                                    # least share of the pixels a top-l case compares


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


class Sweep:
    """tests/test_gpu_train_edges.Sweep with this module's BARS and record key: floats are the worst over the cases, wanted <=
    bar * shrink (bar: a key of BARS or a number); bools are wanted True.  shrink = 0.25 for the fp32 stand-ins."""

    def __init__(self, key, shrink=1.0):
        self.key, self.shrink, self.worst, self.bad = key, shrink, {}, {}

    def add(self, case, name, value, bar=None):
        if isinstance(value, bool):
            self.worst[name] = self.worst.get(name, True) and value
            fail = not value
        else:
            limit = (BARS[bar] if isinstance(bar, str) else bar) * self.shrink
            self.worst[name] = max(self.worst.get(name, 0.0), value)
            fail = not value <= limit
        if fail:
            self.bad.setdefault(str(case), {})[name] = value

    def low(self, name, value):
        self.worst[name] = min(self.worst.get(name, value), value)

    def finish(self, record=True):
        print('%s: %s' % (self.key, self.worst))
        if record:
            H.record_parity('match_bwd_edges/' + self.key, self.worst)
        assert not self.bad, self.bad


# ================================================================================================ 1. swem_match_bwd_f32
# (P, N, C, L, banks, V, tau, keys): the readout path alone (dS NULL), every pixel compared
A_CASES = [
    (1, 1, 128, 64, 1, 64, TAU, 'structured'),      # one pixel, one object, one bank (dnu_update NULL), Lm = 64: every count at its least
    (5, 2, 64, 64, 2, 32, TAU, 'gauss'),            # two pixel-kernel blocks per object, C = 64, Lm = 128, the smallest V of training
    (127, 3, 128, 128, 2, 64, TAU, 'structured'),   # one row short of the pad, one FULL group of the d qn GEMM, Lm = 256
    (128, 4, 128, 64, 2, 128, TAU, 'gauss'),        # exactly the pad (no zero row at all), full + 1: the first re-packed filters
    (129, 4, 64, 128, 1, 64, TAU, 'structured'),    # one row past the pad (Pm = 256, 127 pad rows), re-pack at C = 64, one bank Lm = 128
    (129, 6, 128, 64, 1, 32, TAU, 'gauss'),         # two full groups (the second accumulates onto the first), one bank Lm = 64
    (257, 7, 128, 64, 2, 64, TAU, 'structured'),    # three row tiles, two full groups + 1: all three copies into the half slot
    (576, 2, 128, 256, 2, 512, TAU, 'structured'),  # training's own P, a partial group of two, Lm = 512, V = 512
    (577, 7, 128, 256, 2, 64, TAU, 'structured'),   # the largest: P prime, seven objects, Lm = 512
    (577, 3, 64, 256, 1, 128, TAU, 'gauss'),        # one bank Lm = 256 at C = 64, five row tiles
    (129, 2, 128, 64, 2, 64, 1.0, 'gauss'),         # tau = 1: a flat softmax, every base carries gradient
    (576, 6, 64, 128, 2, 32, TAU, 'gauss'),         # training's P with two full groups at C = 64, Lm = 256
    (257, 1, 64, 256, 2, 128, TAU, 'gauss'),        # ONE object over several tiles (no concatenated source), Lm = 512 at C = 64
    (128, 7, 64, 64, 1, 512, TAU, 'structured'),    # seven objects at the smallest Lm and the largest V, no pad row
    (127, 6, 128, 256, 2, 32, 1.0, 'structured'),   # tau = 1 on clustered keys, two full groups at Lm = 512
]
TOPL_A = 8                                          # (only the forward's S sees it when dS is NULL)
# the smallest V the entry takes (a multiple of 4, as the forward): accepted and right, as include/swem_hip_train.h says
V4_CASE = (129, 2, 128, 64, 2, 4, TAU, 'gauss')
# (P, N, C, L, banks, V, topl, seed): the top-l path; Gaussian keys and bases, near ties left out
B_CASES = [
    (5, 1, 128, 64, 2, 32, 1, 1),                   # topl = 1: only rank 0 carries d c
    (127, 3, 64, 128, 2, 128, 5, 1),                # an odd topl, one full group, C = 64
    (128, 2, 128, 128, 1, 64, 32, 1),               # one bank, exactly the pad
    (129, 4, 64, 64, 1, 64, 64, 1),                 # topl = 64 = Lm: every base is in the list, the cut is the last element
    (257, 6, 128, 64, 2, 32, 5, 1),                 # two full groups, three row tiles
    (129, 7, 128, 256, 2, 64, 64, 1),               # topl = 64 at Lm = 512, seven objects, one row past the pad
    (577, 7, 128, 256, 2, 64, 64, 1),               # the largest
]


@functools.lru_cache(maxsize=None)
def match_inputs(P, N, C, L, banks, V, keys, topl, seed):
    """q (P, C) raw query key, banks of l2-normalised key bases (1, N, 2, C, L) and value bases (1, N, 2, V, L), dmem (N, P, V),
    dS (N, P, 2 topl).  'structured': test_match_backward's peaked-softmax regime (clustered keys, bases near pixels)."""
    g = torch.Generator().manual_seed(9000 + 131 * seed + P + 7 * N + C + L + 3 * banks + V + topl)
    if keys == 'structured':
        q, _ = H.structured_keys(P, C, 5, g)
        kap = [O.l2norm(torch.randn(1, N, 2, C, L, generator=g) * 0.3 + q[torch.randint(0, P, (L,), generator=g)].t(), -2)
               for _ in range(banks)]
    else:
        q = torch.randn(P, C, generator=g)
        kap = [O.l2norm(torch.randn(1, N, 2, C, L, generator=g), -2) for _ in range(banks)]
    nu = [torch.randn(1, N, 2, V, L, generator=g) for _ in range(banks)]
    return dict(P=P, N=N, C=C, L=L, banks=banks, V=V, q=q, kap=kap, nu=nu, dmem=torch.randn(N, P, V, generator=g),
                dS=torch.randn(N, P, 2 * topl, generator=g))


def match_ref(k, tau, topl, dtype, use_dS, use_dmem, zero_row=None, drop_obj=False):
    """O.get_affinity(O.l2norm(q, 1), O.l2norm(mk, -2), mv, tau, topl) under autograd in `dtype` -> S (N, P, 2 topl), mem (N, P, V),
    dqk (P, C), dnu per bank (N, 2, V, L).  zero_row / drop_obj: the stand-ins that lose one pixel's row of dmem / the last object."""
    P, N, C = k['P'], k['N'], k['C']
    q = leaf(k['q'].t().reshape(1, C, 1, P), dtype)
    nus = [leaf(n_, dtype) for n_ in k['nu']]
    mk = torch.cat(k['kap'], -1).to(dtype)
    S, mem = O.get_affinity(O.l2norm(q, 1), O.l2norm(mk, -2), torch.cat(nus, -1), tau, topl)
    S, mem = S.view(N, 2 * topl, P).permute(0, 2, 1), mem[0].flatten(2).permute(0, 2, 1)
    dmem, dS = k['dmem'].to(dtype), k['dS'].to(dtype)
    if zero_row is not None:
        dmem = dmem.clone()
        dmem[:, zero_row] = 0
    w = torch.ones(N, 1, 1, dtype=dtype)
    if drop_obj:
        w[N - 1] = 0
    loss = (S * dS * w).sum() * float(use_dS) + (mem * dmem * w).sum() * float(use_dmem)
    loss.backward()
    return dict(S=S.detach(), mem=mem.detach(), dqk=q.grad[0, :, 0].t().contiguous(),
                dnu=[torch.zeros_like(n_[0]) if n_.grad is None else n_.grad[0] for n_ in nus])


def kept_pixels(k, tau, topl):
    """test_match_backward's near-tie filter, from float64 alone: a pixel is compared when, for every (object, class), the sorted
    affinities of ranks 0 .. topl (the list and the cut) lie more than 5e-6 logit units apart."""
    C, P = k['C'], k['P']
    with torch.no_grad():
        qn = O.l2norm(k['q'].t().reshape(1, C, 1, P).double(), 1).flatten(2)[:, None, None]
        mk = O.l2norm(torch.cat(k['kap'], -1).double(), -2)
        srt = torch.matmul(mk.transpose(-2, -1), qn).sort(dim=3, descending=True)[0]          # 1,N,2,Lm,P
        kk = min(topl, mk.shape[-1] - 1)
        gap = ((srt[:, :, :, :kk] - srt[:, :, :, 1:kk + 1]) / tau).amin(dim=3)
        return (gap > 5e-6).all(dim=1).all(dim=1)[0]


@functools.lru_cache(maxsize=None)
def a_refs(case):
    P, N, C, L, banks, V, tau, keys = case
    k = match_inputs(P, N, C, L, banks, V, keys, TOPL_A, 0)
    return k, match_ref(k, tau, TOPL_A, F64, False, True), match_ref(k, tau, TOPL_A, F32, False, True)


@functools.lru_cache(maxsize=None)
def b_refs(case, use_dmem):
    P, N, C, L, banks, V, topl, seed = case
    k = match_inputs(P, N, C, L, banks, V, 'gauss', topl, seed)
    return (k, match_ref(k, TAU, topl, F64, True, use_dmem), match_ref(k, TAU, topl, F32, True, use_dmem),
            kept_pixels(k, TAU, topl))


class HipMatch:
    """swem_match_f32 / swem_match_bwd_f32 through the C ABI on one case's inputs (uploaded once).  Every output starts as NaN."""

    def __init__(self, k):
        self.k = k
        self.q = dv(k['q'])
        self.kap = [dv(t[0]) for t in k['kap']] + [None]
        self.nu = [dv(t[0]) for t in k['nu']] + [None]
        self.dims = (k['N'], k['C'], k['V'], k['P'], k['L'])
        self.Pm = _lib.query('swem_match_pad', k['P'])
        assert self.Pm == pad128(k['P'])

    def forward(self, tau, topl):
        N, C, V, P, L = self.dims
        mem = torch.full((N, self.Pm, V), float('nan'), device=DEV)
        S = torch.full((N, P, 2 * topl), float('nan'), device=DEV)
        wsb = _lib.query('swem_match_workspace', N, C, V, P, L, self.k['banks'], 0)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        _lib.call('swem_match_f32', ops._stream(), self.q.data_ptr(), self.kap[0].data_ptr(), self.nu[0].data_ptr(), ptr(self.kap[1]),
                  ptr(self.nu[1]), mem.data_ptr(), S.data_ptr(), N, C, V, P, L, topl, tau, 0, ws.data_ptr(), wsb)
        return S.cpu(), mem.cpu()

    def backward(self, tau, topl, use_dS, use_dmem, ws_byte=None, pad_rows=0.0, raw=False, over=None):
        """ws_byte: fill the workspace with this byte first; pad_rows: the value of dmem's rows [P, Pm); raw: return the status
        and the output buffers (pre-filled with the sentinel 7.0) without raising; over: arguments replaced (N, topl, tau, short)."""
        N, C, V, P, L = self.dims
        k, over = self.k, over or {}
        dmem = torch.full((N, self.Pm, V), pad_rows, device=DEV)
        dmem[:, :P] = dv(k['dmem']) if use_dmem else 0.0
        dS = dv(k['dS']) if use_dS else None
        fill = 7.0 if raw else float('nan')
        dqk = torch.full((P, C), fill, device=DEV)
        dnu = [torch.full_like(n_, fill) for n_ in self.nu[:k['banks']]] + [None]
        wsb = _lib.query('swem_match_bwd_workspace', N, C, V, P, L, k['banks'])
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        if ws_byte is not None:
            ws.fill_(ws_byte)
        args = [ops._stream(), self.q.data_ptr(), self.kap[0].data_ptr(), self.nu[0].data_ptr(), ptr(self.kap[1]), ptr(self.nu[1]),
                dmem.data_ptr(), ptr(dS), dqk.data_ptr(), dnu[0].data_ptr(), ptr(dnu[1]), over.get('N', N), over.get('C', C), V, P,
                over.get('L', L), over.get('topl', topl), over.get('tau', tau), ws.data_ptr(), wsb - over.get('short', 0)]
        for i in over.get('null', ()):
            args[i] = 0
        if raw:
            rc = _lib.load().swem_match_bwd_f32(*args)
            torch.cuda.synchronize()
            return rc, [dqk.cpu()] + [t.cpu() for t in dnu[:k['banks']]]
        _lib.call('swem_match_bwd_f32', *args)
        return dict(dqk=dqk.cpu(), dnu=[t.cpu() for t in dnu[:k['banks']]])


def dqk_errors(got, want, cpu32, keep):
    """(error of `got`, the fp32 CPU oracle's own error, scale) of d qk on the kept pixels, all against float64"""
    ref = want[keep]
    return (float((got.double()[keep] - ref).abs().max()), float((cpu32.double()[keep] - ref).abs().max()),
            float(ref.abs().max()) + 1e-30)


def judge_match(S, tag, got, want, cpu32, keep, hip, dmem_zero=False):
    """One case's S, mem_out, d nu and d qk into the sweep.  hip: d qk against max(3 err_cpu_fp32, 2e-4 scale), recorded as a
    fraction of that bar; stand-in: err_cpu_fp32 against 2e-4 scale."""
    if 'S' in got:
        S.add(tag, 'S', rel(got['S'], want['S']), 'S')
        S.add(tag, 'mem', rel(got['mem'], want['mem']), 'mem')
    for i, (a, b) in enumerate(zip(got['dnu'], want['dnu'])):
        if dmem_zero:                                      # (the value bases enter through mem_out alone: an exact zero)
            S.add(tag, 'dnu_exactly_zero', not bool(a.any()) and not bool(b.any()))
        else:
            S.add(tag, 'dnu', rel(a, b), 'dnu')
    S.add(tag, 'finite', bool(torch.isfinite(got['dqk']).all()) and all(bool(torch.isfinite(t).all()) for t in got['dnu']))
    err, err_cpu, scale = dqk_errors(got['dqk'], want['dqk'], cpu32['dqk'], keep)
    if hip:
        S.add(tag, 'dqk/bar', err / max(3 * err_cpu, BARS['dqk'] * scale), 1.0)
        S.add(tag, 'dqk', err / scale, float('inf'))       # (recorded beside it; the line above judges)
    else:
        S.add(tag, 'dqk', err_cpu / scale, 'dqk')


def readout_check(S, hip):
    for case in A_CASES + [V4_CASE]:
        k, want, cpu32 = a_refs(case)
        tau = case[6]
        keep = torch.ones(k['P'], dtype=torch.bool)
        if hip:
            run = HipMatch(k)
            if case is V4_CASE:
                rc, _ = run.backward(tau, TOPL_A, False, True, raw=True)
                S.add(case, 'v4_accepted', rc == 0)              # (the header: V any multiple of 4; compared like every case)
                if rc != 0:
                    continue
            got = run.backward(tau, TOPL_A, False, True)
            got['S'], got['mem'] = run.forward(tau, TOPL_A)
            got['mem'] = got['mem'][:, :k['P']]
        else:
            got = cpu32
        judge_match(S, case, got, want, cpu32, keep, hip)


def topl_check(S, hip):
    for case in B_CASES:
        topl = case[6]
        for use_dmem in (False, True):
            k, want, cpu32, keep = b_refs(case, use_dmem)
            share = float(keep.float().mean())
            tag = case + ('both' if use_dmem else 'dmem_zero',)
            S.low('kept_share', share)
            S.add(tag, 'kept_share_ok', share >= KEPT)
            if hip:
                run = HipMatch(k)
                got = run.backward(TAU, topl, True, use_dmem)
                if use_dmem:
                    got['S'], got['mem'] = run.forward(TAU, topl)
                    got['mem'] = got['mem'][:, :k['P']]
            else:
                got = dict(cpu32)
                if not use_dmem:
                    got.pop('S'), got.pop('mem')
            judge_match(S, tag, got, want, cpu32, keep, hip, dmem_zero=not use_dmem)
        print('top-l case %s: %d of %d pixels compared' % (case, int(keep.sum()), k['P']))


@gpu
def test_match_bwd_readout_path_vs_float64(lib):
    """swem_match_bwd_f32 with dS = NULL at A_CASES (and swem_match_f32's S and mem_out beside it): d qk, dnu_first and dnu_update
    are smooth in every input here, so EVERY pixel is compared, on clustered and on Gaussian keys.  V = 4, the smallest V the entry
    takes, is accepted and right, as include/swem_hip_train.h says."""
    S = Sweep('match_bwd_readout')
    readout_check(S, True)
    S.finish()


@gpu
def test_match_bwd_topl_path_vs_float64(lib):
    """swem_match_bwd_f32 with dS random at B_CASES, once with dmem all zero (dnu_* must come back exactly zero) and once with both
    gradients: topl = 1, 5, 32, 64, 64 = Lm, 64 at Lm = 512.  Near ties of the top-l are left out as in test_match_backward; every
    case compares at least 75 % of its pixels."""
    S = Sweep('match_bwd_topl')
    topl_check(S, True)
    S.finish()


def test_standin_match_bwd_readout_path():
    S = Sweep('standin/match_bwd_readout', shrink=0.25)
    readout_check(S, False)
    S.finish(record=False)


def test_standin_match_bwd_topl_path():
    S = Sweep('standin/match_bwd_topl', shrink=0.25)
    topl_check(S, False)
    S.finish(record=False)


# ================================================================================ 2. what swem_match_bwd_f32 must not depend on
STALE_CASE = (129, 4, 128, 64, 2, 64, 32)           # P one past the pad, N = 4 (the re-packed filters)


def _stale_inputs():
    P, N, C, L, banks, V, topl = STALE_CASE
    return match_inputs(P, N, C, L, banks, V, 'gauss', topl, 2), topl


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip([a['dqk']] + a['dnu'], [b['dqk']] + b['dnu']))


@gpu
def test_match_bwd_ignores_a_stale_workspace(lib):
    """The whole workspace filled with 0xFF bytes (NaN patterns) before the call, at P = 129 and N = 4: d qk and dnu_* are finite and
    bit-equal to the call on a zeroed workspace -- no slot is read before it is written, no pad row is left as it was."""
    k, topl = _stale_inputs()
    run = HipMatch(k)
    clean, stale = run.backward(TAU, topl, True, True, ws_byte=0), run.backward(TAU, topl, True, True, ws_byte=255)
    finite = all(bool(torch.isfinite(t).all()) for t in [stale['dqk']] + stale['dnu'])
    H.record_parity('match_bwd_edges/match_bwd_stale_workspace', {'finite': finite, 'bit_equal': same_bits(clean, stale)})
    assert finite and same_bits(clean, stale) and bool(stale['dqk'].any())


@gpu
def test_match_bwd_ignores_the_pad_rows_of_dmem(lib):
    """include/swem_hip_train.h: rows [P, Pm) of dmem may hold any finite values.  With those rows at 3.0, d qk and dnu_* are
    bit-equal to the call with them zero (the probabilities of the pad rows are exact zeros, and the pad rows of dP and d qn are
    never read back)."""
    k, topl = _stale_inputs()
    run = HipMatch(k)
    zero, filled = run.backward(TAU, topl, True, True, pad_rows=0.0), run.backward(TAU, topl, True, True, pad_rows=3.0)
    H.record_parity('match_bwd_edges/match_bwd_dmem_pad_rows', {'bit_equal': same_bits(zero, filled)})
    assert same_bits(zero, filled) and bool(filled['dnu'][0].any())


# (name, replaced arguments, status): each is refused before the first launch -- the outputs keep their sentinel
REFUSALS = [('N = 0', dict(N=0), E_SHAPE), ('N = 8', dict(N=8), E_SHAPE),
            ('kappa_update without nu_update', dict(null=(5,)), E_ARG), ('nu_update without kappa_update', dict(null=(4,)), E_ARG),
            ('both given, dnu_update NULL', dict(null=(10,)), E_ARG),
            ('workspace one byte short', dict(short=1), E_WORKSPACE),
            # what swem_match_f32 refuses (match_check), the backward refuses too
            ('topl = 0', dict(topl=0), E_SHAPE), ('topl = 65', dict(topl=65), E_SHAPE), ('tau = 0', dict(tau=0.0), E_ARG),
            ('C = 96', dict(C=96), E_SHAPE), ('Lm = 96', dict(L=48), E_SHAPE)]


@gpu
def test_match_bwd_refusals_write_nothing(lib):
    """Every refusal returns its own status and leaves d qk, dnu_first and dnu_update untouched (pre-filled with 7.0)."""
    k, topl = _stale_inputs()
    run = HipMatch(k)
    got = {}
    for name, over, want in REFUSALS:
        rc, outs = run.backward(TAU, topl, True, True, raw=True, over=over)
        got[name] = (rc, all(bool((t == 7.0).all()) for t in outs))
    ops.check_faults()
    H.record_parity('match_bwd_edges/match_bwd_refusals', {n: list(v) for n, v in got.items()})
    assert got == {name: (want, True) for name, _, want in REFUSALS}, got


# ============================================================================================== 3. swem_nu_update_bwd_f32
# (P, N, V, L, with dnu_prev)
NU_CASES = [(1, 1, 32, 64, True), (127, 2, 128, 128, True), (128, 5, 32, 256, True), (129, 7, 512, 64, True),
            (576, 2, 128, 64, True), (577, 7, 32, 256, True), (577, 5, 512, 128, False)]
NU_L32 = (129, 2, 128, 32, True)                    # L = 32 (L % 32 == 0 is all the entry asks): accepted and right, as the header says


@functools.lru_cache(maxsize=None)
def nu_inputs(P, N, V, L):
    """z (N, Pz, 2L) >= 0 with rows >= P zero, zita_prev in [1e-6, 3], zita = zita_prev + the column sums of z (as m_step makes it;
    up to 4), dnu.  Every 13th base holds the oracle's floor zita_prev = 1e-6 and a z column scaled by 1e-7: zita = 1e-6 plus a
    little there, dnu / zita of order 1e6."""
    g = torch.Generator().manual_seed(7000 + P + 3 * N + V + L)
    w = torch.rand(N, 1, 2 * L, generator=g) * 2
    w[..., ::13] = 1e-7
    z = torch.zeros(N, pad128(P), 2 * L)
    z[:, :P] = torch.rand(N, P, 2 * L, generator=g) * w / P
    zita_prev = torch.rand(N, 2 * L, generator=g) * 3 + 1e-6
    zita_prev[:, ::13] = 1e-6
    zita = (zita_prev + z.sum(1)).view(N, 2, L)
    assert float(zita.min()) < 1.2e-6 and float(zita.max()) > 3
    return dict(P=P, N=N, V=V, L=L, z=z, zita_prev=zita_prev.view(N, 2, L), zita=zita, dnu=torch.randn(N, 2, V, L, generator=g))


def nu_ref(k, dtype, drop=None):
    """dv = z . (dnu / zita), dnu_prev = dnu zita_prev / zita (modules.py:164-165 differentiated) in `dtype`; drop: one pixel of
    z left out."""
    N, V, L, P = k['N'], k['V'], k['L'], k['P']
    z = k['z'][:, :P].to(dtype)
    if drop is not None:
        z = z.clone()
        z[:, drop] = 0
    G = k['dnu'].to(dtype) / k['zita'].to(dtype)[:, :, None]                    # (N, 2, V, L)
    return torch.matmul(z, G.permute(0, 1, 3, 2).reshape(N, 2 * L, V)), G * k['zita_prev'].to(dtype)[:, :, None]


def nu_hip(k, with_prev=True, ws_byte=None, z=None, raw=False):
    N, V, L, P = k['N'], k['V'], k['L'], k['P']
    fill = 7.0 if raw else float('nan')
    zd, zp, zt, dnu = dv(k['z'] if z is None else z), dv(k['zita_prev']), dv(k['zita']), dv(k['dnu'])
    dvv = torch.full((N, P, V), fill, device=DEV)
    dprev = torch.full((N, 2, V, L), fill, device=DEV) if with_prev else None
    wsb = _lib.query('swem_nu_update_bwd_workspace', N, V, P, L)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    if ws_byte is not None:
        ws.fill_(ws_byte)
    args = (ops._stream(), zd.data_ptr(), zp.data_ptr(), zt.data_ptr(), dnu.data_ptr(), dvv.data_ptr(), ptr(dprev), N, V, P, L,
            ws.data_ptr(), wsb)
    if raw:
        rc = _lib.load().swem_nu_update_bwd_f32(*args)
        torch.cuda.synchronize()
        return rc, dvv.cpu(), dprev.cpu()
    _lib.call('swem_nu_update_bwd_f32', *args)
    return dvv.cpu(), None if dprev is None else dprev.cpu()


def nu_check(S, hip):
    for case in NU_CASES + [NU_L32]:
        k = nu_inputs(*case[:4])
        want = nu_ref(k, F64)
        if hip:
            if case is NU_L32:
                rc, _, _ = nu_hip(k, raw=True)
                S.add(case, 'l32_accepted', rc == 0)             # (the header: L % 32 == 0; compared like every case)
                if rc != 0:
                    continue
            got = nu_hip(k, with_prev=case[4])
        else:
            got = nu_ref(k, F32)
        S.add(case, 'dv', rel(got[0], want[0]), 'nu_dv')
        if case[4]:
            S.add(case, 'dnu_prev', rel(got[1], want[1]), 'nu_dprev')
        print('value update backward %s: dv %.3g%s' % (case, rel(got[0], want[0]), ', dnu_prev %.3g' % rel(got[1], want[1]) if case[4] else ''))
        S.add(case, 'finite', bool(torch.isfinite(got[0]).all()))


@gpu
def test_nu_update_backward_vs_float64(lib):
    """swem_nu_update_bwd_f32 on its own, given z: P on both sides of the pad and of training's 576, N = 1 .. 7, V = 32 .. 512,
    L = 32 .. 256, zita from the oracle's floor 1e-6 to 4, dnu_prev NULL once.  L = 32 is right (the header says L % 32 == 0)."""
    S = Sweep('nu_update_bwd')
    nu_check(S, True)
    S.finish()


def test_standin_nu_update_backward():
    """fp32 torch.matmul standing in: the bars of BARS are 8x what it measures, so it sits 8x under them (shrink 1/8)."""
    S = Sweep('standin/nu_update_bwd', shrink=0.125)
    nu_check(S, False)
    S.finish(record=False)


@gpu
def test_nu_update_backward_one_hot_probes(lib):
    """z with a SINGLE non-zero entry -- at pixel 0, 127, 128 (the pad edge inside P = 200) and P - 1, for the first and the last
    of three objects: dv is non-zero in exactly that pixel's row of that object, and is the reference there."""
    P, N, V, L = 200, 3, 32, 64
    k = dict(nu_inputs(P, N, V, L))
    ok, worst = {}, 0.0
    for n in (0, N - 1):
        for pix in (0, 127, 128, P - 1):
            z = torch.zeros(N, pad128(P), 2 * L)
            col = (37 * pix + 5 * n) % (2 * L)
            z[n, pix, col] = 0.75
            k['z'] = z
            want, _ = nu_ref(k, F64)
            got, _ = nu_hip(k, z=z)
            rows = got.abs().amax(-1).nonzero().tolist()
            e = rel(got[n, pix], want[n, pix])
            worst = max(worst, e)
            ok[(n, pix)] = rows == [[n, pix]] and e <= BARS['nu_dv']
    print('one-hot probes of the value update backward: %s, worst %.3g' % (ok, worst))
    H.record_parity('match_bwd_edges/nu_update_bwd_one_hot', {'placed': all(ok.values()), 'worst': worst})
    assert all(ok.values()), ok


@gpu
def test_nu_update_backward_ignores_a_stale_workspace(lib):
    k = nu_inputs(129, 4, 128, 64)
    clean, stale = nu_hip(k, ws_byte=0), nu_hip(k, ws_byte=255)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(clean, stale))
    finite = all(bool(torch.isfinite(t).all()) for t in stale)
    H.record_parity('match_bwd_edges/nu_update_bwd_stale_workspace', {'finite': finite, 'bit_equal': same})
    assert same and finite and bool(stale[0].any())


# ============================================================================================= 4. swem_memorize_train_f32
# (h, w, C, L, N): P = 54, 129, 577
MEM_CASES = [((6, 9), 128, 64, 1), ((6, 9), 64, 256, 3), ((3, 43), 64, 64, 3), ((3, 43), 128, 256, 1), ((1, 577), 128, 64, 3),
             ((1, 577), 64, 256, 1)]
MEM_V = 64


@functools.lru_cache(maxsize=None)
def mem_inputs(hw, C, L, N):
    g = torch.Generator().manual_seed(400 + hw[0] * hw[1] + C + L + N)
    x, v, m = H.em_inputs(hw[0], hw[1], C, MEM_V, N, g)
    x_t = x.flatten(2)[:, None, None].transpose(-2, -1)                         # 1,1,1,P,C
    return dict(P=hw[0] * hw[1], C=C, L=L, N=N, x=x, v=v, m=m, x_t=x_t, kappa=near_data_bases(x_t[0, 0, 0], (1, N, 2, C, L), g),
                nu=torch.randn(1, N, 2, MEM_V, L, generator=g), zita=torch.rand(1, N, 2, 1, L, generator=g) * 3 + 1e-6)


def mem_estep(k, dtype):
    """the E step of the prior bases with w_in = masks: what z_out holds at T = 1 (1, N, 2, P, L)"""
    return O.e_step(k['x_t'].to(dtype), k['kappa'].to(dtype), k['m'].flatten(3).unsqueeze(-1).to(dtype), TAU)


def mem_hip(k, T, train):
    N, C, L, P, V = k['N'], k['C'], k['L'], k['P'], MEM_V
    ins = [dv(k['x'][0].flatten(1).t()), dv(k['v'][0].flatten(2).transpose(1, 2)), dv(k['m'][0].flatten(2)), dv(k['kappa'][0]),
           dv(k['nu'][0]), dv(k['zita'][0, :, :, 0])]
    outs = [torch.full_like(ins[3], float('nan')), torch.full_like(ins[4], float('nan')), torch.full_like(ins[5], float('nan'))]
    wsb = _lib.query('swem_memorize_workspace', N, C, V, P, L)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    z = torch.full((N, _lib.query('swem_em_pad', P), 2 * L), float('nan'), device=DEV) if train else None
    _lib.call('swem_memorize_train_f32' if train else 'swem_memorize_f32', ops._stream(), *[t.data_ptr() for t in ins + outs],
              *([z.data_ptr()] if train else []), N, C, V, P, L, T, TAU, ws.data_ptr(), wsb)
    return [t.cpu() for t in outs] + [None if z is None else z.cpu()]


@gpu
@pytest.mark.parametrize('case', MEM_CASES, ids=lambda c: 'P%d-C%d-L%d-N%d' % (c[0][0] * c[0][1], c[1], c[2], c[3]))
def test_memorize_train_hands_out_the_forwards_z(lib, case):
    """swem_memorize_train_f32 at T = 1 and 4: kappa_out, nu_out and zita_out are swem_memorize_f32's bit for bit ("the same", says
    the header); z_out, pre-filled with NaN, comes back finite in rows < P and exactly zero in rows [P, Pz); at T = 1 it is the
    float64 E step of the prior bases to 1e-4; and it IS the z behind nu_out: (zita_prev nu_prev + v^T z_out) / zita_out in
    float64 from the returned buffers equals nu_out (mass-weighted, 1e-4), zita_prev + the column sums of z_out equals zita_out --
    what swem_nu_update_bwd_f32 relies on."""
    k = mem_inputs(*case)
    P, N, L = k['P'], k['N'], k['L']
    S = Sweep('memorize_train[P=%d,C=%d,L=%d,N=%d]' % (P, k['C'], L, N))
    for T in (1, 4):
        kap, nu, zita, z = mem_hip(k, T, True)
        plain = mem_hip(k, T, False)
        S.add(T, 'bases_bit_equal', all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((kap, nu, zita), plain)))
        S.add(T, 'pad_rows_zero', z.shape[1] == pad128(P) and not bool(z[:, P:].any()))
        S.add(T, 'rows_finite', bool(torch.isfinite(z[:, :P]).all()) and bool((z[:, :P] >= 0).all()) and bool(z.any()))
        if T == 1:
            S.add(T, 'z_vs_float64', rel(z_to_oracle(z, P), mem_estep(k, F64)), 'z')
        z64, mass = z[:, :P].double(), zita.double()[:, :, None]                    # (N, P, 2L), (N, 2, 1, L)
        vz = torch.einsum('npv,npk->nvk', k['v'][0].flatten(2).transpose(1, 2).double(), z64).view(N, MEM_V, 2, L).permute(0, 2, 1, 3)
        nu64 = (k['zita'][0].double() * k['nu'][0].double() + vz) / mass
        S.add(T, 'nu_from_z_out', float(((nu.double() - nu64) * mass).abs().max() / (nu64 * mass).abs().max()), 'nu')
        S.add(T, 'zita_from_z_out', rel(zita, k['zita'][0, :, :, 0].double() + z64.sum(1).view(N, 2, L)), 'zita')
    S.finish()


def test_standin_memorize_estep():
    """the fp32 CPU oracle's E step of the same priors against float64: 4x under the z bar at every case"""
    S = Sweep('standin/memorize_train', shrink=0.5)
    for case in MEM_CASES:
        k = mem_inputs(*case)
        S.add(case, 'z_vs_float64', rel(mem_estep(k, F32), mem_estep(k, F64)), 'z')
    S.finish(record=False)


# ===================================================================================================== 5. clips through autograd
@gpu
def test_three_clips_through_autograd_equal_three_calls(lib):
    """autograd.match and autograd.memorize with G = 3 clips of N = 3 objects at P = 129 (the hand-written per-clip byte offsets
    of _Match / _Memorize, forward and backward): outputs and every gradient are bit-equal to three G = 1 calls on the clips'
    slices."""
    from swem_amd import autograd as A
    G, N, P, C, V, L, topl, T = 3, 3, 129, 128, 64, 64, 32, 4
    g = torch.Generator().manual_seed(55)
    bad = []

    def eq(what, a, b):
        if not (torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a).all()) and bool(a.any())):
            bad.append(what)

    # matching
    q = dv(torch.randn(G, P, C, generator=g))
    kap = [dv(O.l2norm(torch.randn(G * N, 2, C, L, generator=g), -2)) for _ in range(2)]
    nu = [dv(torch.randn(G * N, 2, V, L, generator=g)) for _ in range(2)]
    dmem, dS = dv(torch.randn(G * N, pad128(P), V, generator=g)), dv(torch.randn(G * N, P, 2 * topl, generator=g))
    dmem[:, P:] = 0

    def run_match(q_, nu_, kap_, dm_, ds_):
        leaves = [q_.clone().requires_grad_(True)] + [t.clone().requires_grad_(True) for t in nu_]
        mem, S_ = A.match(leaves[0], leaves[1], leaves[2], kap_[0], kap_[1], topl, TAU)
        ((mem * dm_).sum() + (S_ * ds_).sum()).backward()
        return [mem.detach(), S_.detach()] + [t.grad for t in leaves]
    whole = run_match(q, nu, kap, dmem, dS)
    for c in range(G):
        s = slice(c * N, (c + 1) * N)
        part = run_match(q[c], [t[s] for t in nu], [t[s] for t in kap], dmem[s], dS[s])
        for name, a, b in zip(('mem_out', 'S', 'dqk', 'dnu_first', 'dnu_update'), whole, part):
            eq('match %s clip %d' % (name, c), a[c] if name == 'dqk' else a[s], b)
    # memorize
    ins = [H.em_inputs(3, 43, C, V, N, g) for _ in range(G)]
    x = dv(torch.stack([i[0][0].flatten(1).t() for i in ins]))                                   # (G, P, C)
    v = dv(torch.cat([i[1][0].flatten(2).transpose(1, 2) for i in ins]))                          # (G N, P, V)
    m = dv(torch.cat([i[2][0].flatten(2) for i in ins]))                                          # (G N, 2, P)
    kprev = dv(O.l2norm(torch.randn(G * N, 2, C, L, generator=g), -2))
    nprev, zprev = dv(torch.randn(G * N, 2, V, L, generator=g)), dv(torch.rand(G * N, 2, L, generator=g) * 3 + 1e-6)
    dnu = dv(torch.randn(G * N, 2, V, L, generator=g))

    def run_mem(x_, v_, m_, k_, n_, z_, d_):
        leaves = [v_.clone().requires_grad_(True), n_.clone().requires_grad_(True)]
        kap_, nu_, zita_ = A.memorize(leaves[0], leaves[1], x_, m_.contiguous(), k_.contiguous(), z_.contiguous(), T, TAU)
        (nu_ * d_).sum().backward()
        return [kap_.detach(), nu_.detach(), zita_.detach()] + [t.grad for t in leaves]
    whole = run_mem(x, v, m, kprev, nprev, zprev, dnu)
    for c in range(G):
        s = slice(c * N, (c + 1) * N)
        part = run_mem(x[c], v[s], m[s], kprev[s], nprev[s], zprev[s], dnu[s])
        for name, a, b in zip(('kappa', 'nu', 'zita', 'dv', 'dnu_prev'), whole, part):
            eq('memorize %s clip %d' % (name, c), a[s], b)
    ops.check_faults()
    H.record_parity('match_bwd_edges/clips_through_autograd', {'bit_equal': not bad, 'compared': 2 * 5 * G})
    assert not bad, bad


# ================================================================================================ 6. what the bars are worth
def test_standin_with_a_dropped_element_misses_the_bars():
    """At each sweep's largest case the fp32 stand-in with ONE pixel's row of dmem zeroed (d nu), ONE object left out of the d qk
    sum, ONE pixel of z left out of the value update lies at least 10x beyond the bar (the ratios are in the module docstring)."""
    ratio = {}
    k, want, cpu32 = a_refs(A_CASES[8])
    row = k['P'] // 2
    lost = match_ref(k, TAU, TOPL_A, F32, False, True, zero_row=row)
    ratio['readout: d nu, a dmem row zeroed'] = min(rel(a, b) for a, b in zip(lost['dnu'], want['dnu'])) / BARS['dnu']
    lost = match_ref(k, TAU, TOPL_A, F32, False, True, drop_obj=True)
    keep = torch.ones(k['P'], dtype=torch.bool)
    err, err_cpu, scale = dqk_errors(lost['dqk'], want['dqk'], cpu32['dqk'], keep)
    ratio['readout: d qk, an object dropped'] = err / max(3 * err_cpu, BARS['dqk'] * scale)
    k, want, cpu32, keep = b_refs(B_CASES[-1], True)
    topl = B_CASES[-1][6]
    lost = match_ref(k, TAU, topl, F32, True, True, zero_row=row)
    ratio['top-l: d nu, a dmem row zeroed'] = min(rel(a, b) for a, b in zip(lost['dnu'], want['dnu'])) / BARS['dnu']
    lost = match_ref(k, TAU, topl, F32, True, True, drop_obj=True)
    err, err_cpu, scale = dqk_errors(lost['dqk'], want['dqk'], cpu32['dqk'], keep)
    ratio['top-l: d qk, an object dropped'] = err / max(3 * err_cpu, BARS['dqk'] * scale)
    k = nu_inputs(*NU_CASES[5][:4])
    ratio['value update: dv, a pixel of z dropped'] = rel(nu_ref(k, F32, drop=k['P'] // 2)[0], nu_ref(k, F64)[0]) / BARS['nu_dv']
    print('one dropped element / bar: %s' % {n: round(r, 1) for n, r in ratio.items()})
    assert min(ratio.values()) > 10, ratio
