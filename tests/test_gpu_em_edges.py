"""GPU: the EM / matching kernels (csrc/em.hip, csrc/match.hip) against float64 at the corners tests/test_gpu_em.py does not reach:
the LOOPING M step (P > 1632) and every load-group boundary of both forms, the C = 64 template instances, ragged pixel counts per
kernel, the M step's tile order over its whole (N, R, L) domain, the fused top-l at topl < 64, T = 1, the pad rows of matching.

The float64 references are the oracle's own functions on .double() inputs (oracle/swem_oracle.py: e_step, w_step, m_step, swem,
get_affinity, l2norm) -- per step, identical inputs on both sides.  Tolerances are the suite's per-step bars (tests/test_gpu_em.py):
1e-5 / 1e-6 for the steps without an exp (M step, zita, l2norm), 1e-4 behind an exp((s - max) / tau), 1e-5 for the W step's
weights, matching <= 1e-4 absolute; the fp32 CPU oracle itself sits 40x below them on these inputs (1.2e-7 .. 2.7e-7 on kappa,
1.5e-5 .. 4.9e-5 on z, 2e-6 .. 4e-6 on S), one dropped pixel of 1633 sits 60x above (6e-4).  What the kernels measure is printed
and recorded under em_edges/... (helpers.record_parity) before anything is asserted.

The layout helpers at the top restate include/swem_hip.h's layouts on the host; their round-trip tests need no GPU."""
import pytest
import torch

from oracle import swem_oracle as O
from swem_amd import _lib, ops
from tests import helpers as H

gpu = pytest.mark.gpu
DEV = 'cuda:0'
TAU = 0.05
PRESPLIT_PLAN = 2 | 2 << 4 | 1 << 8 | 3 << 16       # fused top-l + pre-split (f16x3) readout, 64x64 wave tile


# ------------------------------------------------------------------------------------------------------------ layouts
def pad128(P):
    """swem_em_pad / swem_match_pad: rows of a z / mem_out buffer per object."""
    return (P + 127) // 128 * 128


def z_to_oracle(zp, P):
    """pixel-major z (N, Pz, 2L), z[n][p][cls*L + l]  ->  the oracle's (1, N, 2, P, L)."""
    N, _, L2 = zp.shape
    return zp[:, :P].reshape(N, P, 2, L2 // 2).permute(0, 2, 1, 3).unsqueeze(0).contiguous()


def z_from_oracle(z, Pz=None):
    """the oracle's z (1, N, 2, P, L)  ->  pixel-major (N, Pz, 2L), rows [P, Pz) zero."""
    _, N, _, P, L = z.shape
    zp = torch.zeros(N, pad128(P) if Pz is None else Pz, 2 * L, dtype=z.dtype)
    zp[:, :P] = z[0].permute(0, 2, 1, 3).reshape(N, P, 2 * L)
    return zp


def unpack_keys(kp):
    """packed keys (NK, C/4 + 1, R, 4), kp[nk][c/4][l][c%4]  ->  rows (NK, C, R) and the four norm slots (NK, R, 4)."""
    NK, G, R, _ = kp.shape
    return kp[:, :G - 1].permute(0, 1, 3, 2).reshape(NK, 4 * (G - 1), R).contiguous(), kp[:, G - 1].contiguous()


def pack_keys(kappa):
    """(NK, C, L)  ->  packed keys: the re-layout plus the squared norms as C/32 partial sums (the other slots zero)."""
    NK, C, L = kappa.shape
    kp = torch.zeros(NK, C // 4 + 1, L, 4, dtype=kappa.dtype)
    kp[:, :C // 4] = kappa.reshape(NK, C // 4, 4, L).permute(0, 1, 3, 2)
    kp[:, C // 4, :, :C // 32] = (kappa * kappa).reshape(NK, C // 32, 32, L).sum(2).permute(0, 2, 1)
    return kp


def test_z_layout_round_trip():
    g = torch.Generator().manual_seed(1)
    for N, P, L in ((1, 5, 64), (3, 37, 128), (2, 250, 64)):
        z = torch.rand(1, N, 2, P, L, generator=g)
        zp = z_from_oracle(z)
        assert zp.shape == (N, pad128(P), 2 * L) and not zp[:, P:].any()
        assert torch.equal(z_to_oracle(zp, P), z)
        for n, cls, p, l in ((0, 0, 0, 0), (N - 1, 1, P - 1, L - 1), (N - 1, 0, P // 2, 3), (0, 1, 1, L - 2)):
            assert zp[n, p, cls * L + l] == z[0, n, cls, p, l]
        assert torch.equal(z_from_oracle(z_to_oracle(zp, P)), zp)


def test_packed_keys_round_trip():
    g = torch.Generator().manual_seed(2)
    for NK, C, L in ((2, 64, 64), (6, 128, 128), (4, 64, 256)):
        kappa = torch.randn(NK, C, L, generator=g, dtype=torch.float64)
        kp = pack_keys(kappa)
        assert kp.shape == (NK, C // 4 + 1, L, 4)
        for nk, c, l in ((0, 0, 0), (NK - 1, C - 1, L - 1), (1, 37, 5), (NK - 1, 2, L - 3)):
            assert kp[nk, c // 4, l, c % 4] == kappa[nk, c, l]
        rows, slots = unpack_keys(kp)
        assert torch.equal(rows, kappa)
        assert not slots[..., C // 32:].any() and slots[..., :C // 32].all()
        assert float((slots.sum(-1) - (kappa * kappa).sum(1)).abs().max()) < 1e-12 * C


# ------------------------------------------------------------------------------------------------------------ helpers
def d(t):
    return t.to(DEV).contiguous()


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.double()
    return float((a - b).abs().max() / b.abs().max())


def ulps(got, want64):
    """largest distance of fp32 `got` from float64 `want64` in units of want64's fp32 ulp."""
    _, e = torch.frexp(want64.abs())
    ulp = torch.ldexp(torch.ones_like(want64), e - 24)
    return float(((got.detach().double().cpu() - want64).abs() / ulp).max())


def near_data_bases(x_pc, shape, g, spread=None):
    """Bases near randomly chosen pixels of x (P, C) -- a softmax with structure, like an EM in progress; `spread`: per-base
    norms in [0.5, spread] (the kernels normalise the rows themselves; real bases grow to norm ~24)."""
    P = x_pc.shape[0]
    L = shape[-1]
    k = O.l2norm(torch.randn(*shape, generator=g) * 0.3 + x_pc[torch.randint(0, P, (L,), generator=g)].t(), -2)
    if spread:
        k = k * (torch.rand(*shape[:-2], 1, L, generator=g) * (spread - 0.5) + 0.5)
    return k


def mstep_case(P, N, C, V, L, seed):
    """x, v, z (the float64 E step of clustered keys, rounded to fp32: identical inputs for both sides), priors."""
    g = torch.Generator().manual_seed(seed)
    x, v, m = H.em_inputs(1, P, C, V, N, g)
    xf = x.flatten(2)[:, None, None]                                        # 1,1,1,C,P
    x_t = xf.transpose(-2, -1)
    kap = near_data_bases(x_t[0, 0, 0], (1, N, 2, C, L), g)
    z = O.e_step(x_t.double(), kap.double(), m.flatten(3).unsqueeze(-1).double(), TAU).float()
    return dict(xf=xf, mv=v.flatten(3).unsqueeze(2), z=z, zp=d(z_from_oracle(z)),
                zita_prev=torch.rand(1, N, 2, 1, L, generator=g) * (3 - 1e-6) + 1e-6,
                kappa_prev=O.l2norm(torch.randn(1, N, 2, C, L, generator=g), -2),
                nu_prev=torch.randn(1, N, 2, V, L, generator=g))


def mstep_errors(c, P, rows_k=None, rows_v=None):
    """One key launch (shared A, packed keys wanted) and one value launch (per-object A) of a case -> distances to O.m_step in
    float64; rows_k / rows_v: use only the first rows of the key / value space."""
    N, L = c['z'].shape[1], c['z'].shape[-1]
    zprev = d(c['zita_prev'].reshape(2 * N, L))
    e = {}
    if rows_k != 0:
        xf, kprev = c['xf'][..., :rows_k, :], c['kappa_prev'][..., :rows_k, :]
        R = xf.shape[-2]
        out, zita, kn = ops.em_mstep(d(xf[0, 0, 0].t()), False, c['zp'], d(kprev[0].reshape(2 * N, R, L)), zprev, P, want_kn=True)
        k64, z64 = O.m_step(c['z'].double(), xf.double(), kprev.double(), c['zita_prev'].double())
        rows, slots = unpack_keys(kn.cpu())
        e['kappa'] = relmax(out.view(1, N, 2, R, L), k64)
        e['zita'] = relmax(zita.view(1, N, 2, 1, L), z64)
        e['kn_rows'] = relmax(rows.view(1, N, 2, R, L), k64)
        e['kn_norm'] = relmax(slots.double().sum(-1).view(1, N, 2, L), (k64 * k64).sum(-2))
        # the pack the M step keeps IS the pack em_pack_bases builds from its output (em_norm_bases_kernel's tree order), and at
        # C = 64 both leave norm slots 2 and 3 zero
        e['kn_is_pack'] = bool(torch.equal(rows, out.cpu()) and torch.equal(kn, ops.em_pack_bases(out))
                               and not slots[..., R // 32:].any())
    if rows_v != 0:
        mv, nprev = c['mv'][..., :rows_v, :], c['nu_prev'][..., :rows_v, :]
        R = mv.shape[-2]
        out, zita, _ = ops.em_mstep(d(mv[0, :, 0].transpose(1, 2)), True, c['zp'], d(nprev[0].reshape(2 * N, R, L)), zprev, P)
        n64, z64 = O.m_step(c['z'].double(), mv.double(), nprev.double(), c['zita_prev'].double())
        e['nu'] = relmax(out.view(1, N, 2, R, L), n64)
        e['zita_v'] = relmax(zita.view(1, N, 2, 1, L), z64)
    return e


MSTEP_BARS = {'kappa': 1e-5, 'nu': 1e-5, 'kn_rows': 1e-5, 'kn_norm': 1e-5, 'zita': 1e-6, 'zita_v': 1e-6}


def over_the_bars(e, bars=MSTEP_BARS):
    return {k: v for k, v in e.items() if (v is False if isinstance(v, bool) else not v <= bars[k])}


# ------------------------------------------------------------------------------------------------------------ 1. M step
@gpu
@pytest.mark.parametrize('P', [5, 37, 545, 1632, 1633, 3264, 3265, 3600])
def test_mstep_vs_float64(lib, P):
    """Both forms of em_mstep_kernel at every boundary of their 544-pixel load groups (17 steps x 32 pixels): 1632 = the last
    straight-line size (three groups), 1633 = the first looping one (a full iteration, then one with two empty groups), 3264 =
    two iterations exactly, 3265 = one pixel into a third, 3600 = 720p at stride 16; 5, 37, 3265: P % 4 != 0."""
    assert ops.em_pad(P) == pad128(P)
    e = mstep_errors(mstep_case(P, 2, 128, 64, 128, 40 + P), P)
    print('M step P=%d vs float64: %s' % (P, e))
    H.record_parity('em_edges/mstep[P=%d]' % P, e)
    assert not over_the_bars(e), over_the_bars(e)


@gpu
@pytest.mark.parametrize('P', [1632, 1633, 3265])
def test_mstep_one_hot_probes(lib, P):
    """A dropped, doubled or misplaced pixel as an O(1) error: in ONE launch with 8 objects every (object, class) pair has z = 1 at
    a single pixel p* (all bases) and 0 elsewhere, prev = 0, zita_prev = 2^-20: out = A[p*] / (1 + 2^-20) to 2 ulp, zita = 1 +
    2^-20 exactly.  The 16 pixels sit on both sides of every wave-step, load-group and loop-iteration boundary."""
    N, C, V, L = 8, 128, 64, 64
    pix = [min(p, P - 1) for p in (0, 3, 4, 31, 32, 543, 544, 1087, 1088, 1631, 1632, 1633, 2175, 3263, P - 2, P - 1)]
    g = torch.Generator().manual_seed(60 + P)
    x, v = torch.randn(P, C, generator=g), torch.randn(N, P, V, generator=g)
    zp = torch.zeros(N, pad128(P), 2 * L)
    for nk, p in enumerate(pix):
        zp[nk // 2, p, (nk % 2) * L:(nk % 2 + 1) * L] = 1.0
    zprev = d(torch.full((2 * N, L), 2.0 ** -20))
    kap, zk, kn = ops.em_mstep(d(x), False, d(zp), d(torch.zeros(2 * N, C, L)), zprev, P, want_kn=True)
    nu, zv, _ = ops.em_mstep(d(v), True, d(zp), d(torch.zeros(2 * N, V, L)), zprev, P)
    want_k = (x[pix].double() / (1 + 2.0 ** -20)).unsqueeze(-1).expand(2 * N, C, L)
    want_v = torch.stack([v[nk // 2, p] for nk, p in enumerate(pix)]).double().div(1 + 2.0 ** -20).unsqueeze(-1).expand(2 * N, V, L)
    per_pair = [max(ulps(kap[nk], want_k[nk]), ulps(nu[nk], want_v[nk])) for nk in range(2 * N)]
    print('one-hot probes P=%d: ulp distance per (object, class) pair / pixel: %s' % (P, list(zip(pix, per_pair))))
    H.record_parity('em_edges/mstep_one_hot[P=%d]' % P, {'pixels': pix, 'ulps': per_pair})
    assert max(per_pair) <= 2.0, [(p, u) for p, u in zip(pix, per_pair) if u > 2.0]
    one = torch.full((2 * N, L), 1 + 2.0 ** -20)
    assert torch.equal(zk.cpu(), one) and torch.equal(zv.cpu(), one)
    assert torch.equal(unpack_keys(kn.cpu())[0], kap.cpu())


@gpu
def test_mstep_tile_order_sweep(lib):
    """blockIdx -> (row group, base tile, row tile) depends on NK, L / 16, the row tiles R / 32 and the divisor `rpg` nearest
    sqrt(total / 16): every (N, R, L) below against float64 at P = 37 (value rows at every R, key rows with their packed keys
    at R = 64 and 128) walks every rpg the search picks for these shapes."""
    P, worst, bad = 37, {}, {}
    for N in (1, 3, 5, 8):
        for L in (64, 128, 256):
            c = mstep_case(P, N, 128, 512, L, 7000 + 10 * N + L)
            for R in (32, 64, 96, 128, 512):
                e = mstep_errors(c, P, rows_k=R if R in (64, 128) else 0, rows_v=R)
                for k, v in e.items():
                    worst[k] = (worst.get(k, True) and v) if isinstance(v, bool) else max(worst.get(k, 0.0), v)
                if over_the_bars(e):
                    bad[(N, R, L)] = over_the_bars(e)
    print('M step tile-order sweep, worst over (N, R, L): %s' % worst)
    H.record_parity('em_edges/mstep_sweep[P=37]', worst)
    assert not bad, bad


@gpu
def test_mstep_refuses_packed_keys_beyond_four_row_tiles(lib):
    """The pack's norm group has four slots per base (C / 32 partial sums, C <= 128): asking for packed keys with more row
    tiles is an error of the call, not a write past the slots."""
    z = torch.zeros(1, 128, 128, device=DEV)
    with pytest.raises(_lib.SwemHipError):
        ops.em_mstep(torch.zeros(37, 512, device=DEV), False, z, torch.zeros(2, 512, 64, device=DEV),
                     torch.ones(2, 64, device=DEV), 37, want_kn=True)


# ------------------------------------------------------------------------------------------------------------ 2. E / W
@gpu
@pytest.mark.parametrize('L', [64, 128, 256])
@pytest.mark.parametrize('C', [64, 128])
def test_ew_vs_float64(lib, C, L):
    """em_ew16_kernel<L / 64, C / 16> as E step, W step and both from one GEMM, at ragged P (pad pixels: `pin`, zscale = 0, the
    range-checked loads) and, for P = 1633, many blocks; bases of norm 0.5 .. 20 (the kernel normalises from the pack's norm
    slots); object 1 has an all-zero mask: its z and weights are exactly 0.  Rows [P, Pz) of z are exactly zero."""
    N, bad = 3, {}
    for P in (5, 37, 250, 1633):
        # (seeds at which the fp32 CPU oracle itself lies 1e-5 .. 5e-5 from float64 on z: P = 5 has so few pixels that one seed in
        # six leaves max z near 0.1 and puts the reference's own fp32 arithmetic at 1.1e-4 relative to it, beyond the bar)
        g = torch.Generator().manual_seed(1003 + C + L + P)
        x, _, m = H.em_inputs(1, P, C, 32, N, g)
        m[:, 1] = 0
        x_t = x.flatten(2)[:, None, None].transpose(-2, -1)                 # 1,1,1,P,C
        mk = m.flatten(3).unsqueeze(-1)                                     # 1,N,2,P,1
        w_in = torch.rand(1, N, 2, P, 1, generator=g)
        w_in[:, 1] = 0
        kap = near_data_bases(x_t[0, 0, 0], (1, N, 2, C, L), g, spread=20.0)
        x64, k64 = x_t.double(), kap.double()
        kp = ops.em_pack_bases(d(kap[0].reshape(2 * N, C, L)))
        xd, md, wd = d(x_t[0, 0, 0]), d(mk[0, ..., 0].reshape(2 * N, P)), d(w_in[0, ..., 0].reshape(2 * N, P))
        _, z_e = ops.em_ew(xd, kp, None, wd, TAU, 0, 1)
        w_w, _ = ops.em_ew(xd, kp, md, None, TAU, 1, 0)
        w_b, z_b = ops.em_ew(xd, kp, md, None, TAU, 1, 1)
        w64 = O.w_step(k64, x64, mk.double(), TAU)
        e = {'z_e': relmax(z_to_oracle(z_e.cpu(), P), O.e_step(x64, k64, w_in.double(), TAU)),
             'w_w': relmax(w_w.view(1, N, 2, P, 1), w64), 'w_both': relmax(w_b.view(1, N, 2, P, 1), w64),
             'z_both': relmax(z_to_oracle(z_b.cpu(), P), O.e_step(x64, k64, w64, TAU))}
        exact = (not z_e[:, P:].any() and not z_b[:, P:].any() and z_e.shape[1] == pad128(P)
                 and not z_e[1].any() and not z_b[1].any() and not w_w[2:4].any() and not w_b[2:4].any()
                 and bool(torch.isfinite(z_e).all()) and bool(torch.isfinite(z_b).all()))
        print('E/W C=%d L=%d P=%d vs float64: %s, exact zeros: %s' % (C, L, P, e, exact))
        H.record_parity('em_edges/ew[C=%d,L=%d,P=%d]' % (C, L, P), e)
        over = {k: v for k, v in e.items() if not v <= (1e-4 if k[0] == 'z' else 1e-5)}
        if over or not exact:
            bad[P] = (over, exact)
    assert not bad, bad


@gpu
@pytest.mark.parametrize('L', [64, 128, 256])
def test_pack_and_norm_bases_at_c64(lib, L):
    """em_norm_bases_kernel at C = 64, both forms: the packed keys are the bases re-laid bit for bit with the squared norms in
    slots 0 and 1 and slots 2 and 3 exactly zero (two row tiles of 32 channels); the normalised form against float64."""
    g = torch.Generator().manual_seed(64 + L)
    NK, C = 6, 64
    kappa = torch.randn(NK, C, L, generator=g) * (torch.rand(NK, 1, L, generator=g) * 19.5 + 0.5)
    rows, slots = unpack_keys(ops.em_pack_bases(d(kappa)).cpu())
    assert torch.equal(rows, kappa)
    assert not slots[..., 2:].any() and slots[..., :2].all()
    sq = (kappa.double() ** 2).reshape(NK, 2, 32, L).sum(2).permute(0, 2, 1)
    kn = ops.em_norm_bases(d(kappa)).cpu()                                  # (NK, C/4, L, 4)
    e = {'norm_slots': relmax(slots[..., :2], sq), 'l2norm': relmax(kn.permute(0, 1, 3, 2).reshape(NK, C, L),
                                                                   O.l2norm(kappa.double(), 1))}
    print('pack / norm bases C=64 L=%d vs float64: %s' % (L, e))
    H.record_parity('em_edges/pack_bases[C=64,L=%d]' % L, e)
    assert e['norm_slots'] < 1e-6 and e['l2norm'] < 1e-6, e


# ------------------------------------------------------------------------------------------------------------ 3. memorize
@gpu
@pytest.mark.parametrize('C,L,T,h,w,packed', [(64, 64, 3, 10, 25, False), (64, 256, 5, 10, 25, False), (128, 128, 1, 10, 25, False),
                                              (128, 64, 3, 30, 55, True)])
def test_memorize_vs_float64(lib, C, L, T, h, w, packed):
    """swem() end to end at C = 64, at T = 1 (no W step at all: w_in = masks) and at P = 1650 (the looping M step with the value
    rows and a pack), by the yardstick of test_gpu_train.py::test_memorize_backward: the mass-weighted kappa / nu error and the zita
    error against float64 may be max(1e-4, twice the fp32 CPU oracle's own distance to float64 on the same input).  The packed
    case also keeps a pack: it is the pack of the returned bases, and the bases are the unpacked call's, bit for bit."""
    N, V, P = 2, 64, h * w
    g = torch.Generator().manual_seed(300 + C + L + T)
    x, v, m = H.em_inputs(h, w, C, V, N, g)
    prior = {'kappa': O.l2norm(torch.randn(1, N, 2, C, L, generator=g), -2), 'nu': torch.randn(1, N, 2, V, L, generator=g),
             'zita': torch.rand(1, N, 2, 1, L, generator=g) * 3 + 1e-6}
    ref32 = O.swem(x, v, m, prior, L, T, TAU, V)
    r64 = O.swem(x.double(), v.double(), m.double(), {k: t.double() for k, t in prior.items()}, L, T, TAU, V)
    mass = r64['zita']

    def err64(b):
        e = [float(((b[k].double().cpu().view_as(r64[k]) - r64[k]) * mass).abs().max() / (r64[k] * mass).abs().max())
             for k in ('kappa', 'nu')]
        return e + [relmax(b['zita'].view_as(r64['zita']), r64['zita'])]
    args = (d(x[0].flatten(1).t()), d(v[0].flatten(2).transpose(1, 2)), d(m[0].flatten(2)), d(prior['kappa'][0]),
            d(prior['nu'][0]), d(prior['zita'][0, :, :, 0]), T, TAU)
    plain = ops.memorize(*args)
    got = err64(dict(zip(('kappa', 'nu', 'zita'), plain)))
    floor = err64(ref32)
    print('memorize C=%d L=%d T=%d P=%d vs float64 (kappa*zita, nu*zita, zita): hip %s   fp32 oracle %s' % (C, L, T, P, got, floor))
    H.record_parity('em_edges/memorize[C=%d,L=%d,T=%d,P=%d]' % (C, L, T, P), {'hip': got, 'fp32_oracle': floor})
    assert all(a <= max(1e-4, 2 * f) for a, f in zip(got, floor)), (got, floor)
    if packed:
        with ops.use_book(ops.PlanBook(fallback=ops.MODEL_FALLBACK)):
            pack, pack2 = ops.new_pack(N, C, V, L, DEV), ops.new_pack(N, C, V, L, DEV)
            kept = ops.memorize(*args, pack=pack, prior_packed=False, bank=1)
            ops.pack_bank(kept[0], kept[1], pack2, 1)
        for a, b in zip(kept, plain):
            assert torch.equal(a, b)
        assert torch.equal(pack[0], pack2[0]) and torch.equal(pack[1], pack2[1]) and pack[2].any()
        assert pack[2].dtype == torch.float16 and torch.equal(pack[2].view(torch.int16), pack2[2].view(torch.int16))
        ops.check_faults()


# ------------------------------------------------------------------------------------------------------------ 4. matching
def match_case(C, L, banks, P, hw, N, V):
    g = torch.Generator().manual_seed(2000 + C + L + 7 * banks + P)
    qx, _ = H.structured_keys(P, C, 6, g)
    kap = [near_data_bases(qx, (1, N, 2, C, L), g, spread=20.0) for _ in range(banks)]
    nus = [torch.randn(1, N, 2, V, L, generator=g) for _ in range(banks)]
    qn = O.l2norm(qx.t().reshape(1, C, *hw).double(), 1)
    return qx, kap, nus, qn, O.l2norm(torch.cat(kap, -1).double(), -2), torch.cat(nus, -1).double()


def split_planes(flat, npix, Cc, npl):
    """swem_split_f16x2_f32 / swem_split_bf16x3_f32 of a (npix, Cc) fp32 map."""
    if npl == ops.PLANES_F16:
        sp = torch.empty((2, npix * Cc), dtype=torch.float16, device=DEV)
        _lib.call('swem_split_f16x2_f32', ops._stream(), flat.data_ptr(), sp.data_ptr(), npix, Cc, 0, 0)
    else:
        sp = torch.empty((3, npix * Cc), dtype=torch.bfloat16, device=DEV)
        _lib.call('swem_split_bf16x3_f32', ops._stream(), flat.data_ptr(), sp.data_ptr(), npix, Cc, 0)
    return sp


@gpu
@pytest.mark.parametrize('L,banks', [(64, 1), (64, 2), (128, 1), (256, 1), (256, 2)])
@pytest.mark.parametrize('C', [64, 128])
def test_match_vs_float64(lib, C, L, banks):
    """match_affinity16_kernel<Lm / 64, C / 16> for all four Lm at ragged P, topl = 8 / 32 / 64, on both paths: ops.match (fp32
    readout, S from match_topl_kernel) and, for two banks, ops.match_packed under a model's book with the pre-split readout plan
    (S from the fused top-l inside the affinity kernel).  Against float64 get_affinity: S <= 1e-4 absolute, mem_out <= 1e-4 x
    max(1, |mem|max).  Between the paths: S bit-equal at every topl, mem_out within 1e-6 relative; the fused path's S planes
    are the split kernels' planes of S, bit for bit, at topl = 8 and 32.
    (A one-bank ops.match_packed does not exist: a pack always holds two banks, so banks = 1 runs through ops.match only.)"""
    N, V, Lm, bad = 3, 128, banks * L, []
    book = ops.PlanBook(fallback=ops.MODEL_FALLBACK)
    worst = {t: {'S': 0.0, 'mem': 0.0, 'S_fused': 0.0, 'mem_presplit': 0.0, 'mem_presplit_vs_fp32': 0.0} for t in (8, 32, 64)}
    for P, hw in ((37, (1, 37)), (250, (5, 50))):
        qx, kap, nus, qn, mk64, mv64 = match_case(C, L, banks, P, hw, N, V)
        dq, dk, dn = d(qx), [d(k[0]) for k in kap], [d(n_[0]) for n_ in nus]
        if banks == 2:
            with ops.use_book(book):
                book.match[(N, C, V, P, L, 2)] = PRESPLIT_PLAN
                pack = ops.new_pack(N, C, V, L, DEV)
                ops.pack_bank(dk[0], dn[0], pack, 0)
                ops.pack_bank(dk[1], dn[1], pack, 1)
        for topl in (8, 32, 64):
            S64, mem64 = O.get_affinity(qn, mk64, mv64, TAU, topl)
            S64, mem64 = S64.view(N, 2 * topl, P).permute(0, 2, 1), mem64[0].flatten(2).permute(0, 2, 1)
            mscale = max(1.0, float(mem64.abs().max()))
            wt = worst[topl]

            def judge(tag, mem, S):
                e_S, e_m = float((S.double().cpu() - S64).abs().max()), float((mem.double().cpu() - mem64).abs().max()) / mscale
                wt['S' + tag[0]], wt['mem' + tag[1]] = max(wt['S' + tag[0]], e_S), max(wt['mem' + tag[1]], e_m)
                if not (e_S <= 1e-4 and e_m <= 1e-4):
                    bad.append((P, topl, tag, e_S, e_m))
            mem_a, S_a = ops.match(dq, dk[0], dn[0], dk[1] if banks == 2 else None, dn[1] if banks == 2 else None, topl, TAU)
            judge(('', ''), mem_a, S_a)
            if banks == 1:
                continue
            with ops.use_book(book):
                mem_b, S_b = ops.match_packed(dq, pack, L, topl, TAU)
                judge(('_fused', '_presplit'), mem_b, S_b)
                rel = float((mem_b - mem_a).abs().max()) / float(mem_a.abs().max())
                wt['mem_presplit_vs_fp32'] = max(wt['mem_presplit_vs_fp32'], rel)
                if not torch.equal(S_b, S_a) or not rel < 1e-6:
                    bad.append((P, topl, 'fused S bit-equal: %s, pre-split mem_out rel %.3g' % (torch.equal(S_b, S_a), rel)))
                if topl == 64:
                    continue
                mem_i, S_i = ops.match_packed(dq, pack, L, topl, TAU, hw=hw)
                if not (torch.equal(S_i.flatten(1, 2), S_b) and torch.equal(mem_i.flatten(1, 2), mem_b)):
                    bad.append((P, topl, 'the NHWC form differs'))
                try:
                    for want in (ops.PLANES_F16, 3):
                        book.hints[S_i._swem_site] = {False: want}
                        _, S_j = ops.match_packed(dq, pack, L, topl, TAU, hw=hw)
                        planes, n_ = S_j.__dict__['_swem_split'][ops._pkey(False, want)]
                        sp = split_planes(S_j, N * P, 2 * topl, want)
                        if not (n_ == want and torch.equal(S_j, S_i) and torch.equal(planes.view(torch.int16), sp.view(torch.int16))):
                            bad.append((P, topl, 'S planes (%d) differ from the split kernel\'s' % want))
                finally:
                    book.hints.clear()
    ops.check_faults()
    for topl, wt in worst.items():
        print('matching C=%d Lm=%d topl=%d vs float64 (worst over P): %s' % (C, Lm, topl, wt))
        H.record_parity('em_edges/match[C=%d,Lm=%d,topl=%d]' % (C, Lm, topl), wt if banks == 2 else {k: wt[k] for k in ('S', 'mem')})
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ 5. pad rows
@gpu
def test_match_pad_rows_are_zero(lib):
    """mem_out's rows [P, Pm) are exactly zero on both readout paths at P = 37 (Pm = 128): the affinity kernel's pad tiles write
    the probabilities of rows [P, Pm) as zeros and the readout GEMM's last row tile reads them.  A larger call first grows the
    workspace, which is then filled with NaN bit patterns, and the block the output will be allocated from is NaN too: a pad row
    left unwritten, or read from what an earlier call left, cannot pass by luck."""
    N, C, V, L, topl, P = 3, 128, 128, 64, 32, 37
    book = ops.PlanBook(fallback=ops.MODEL_FALLBACK)
    dev = torch.device(DEV)
    out = {}
    for Pc, hw in ((500, (10, 50)), (P, (1, P))):
        qx, kap, nus, _, _, _ = match_case(C, L, 2, Pc, hw, N, V)
        dq, dk, dn = d(qx), [d(k[0]) for k in kap], [d(n_[0]) for n_ in nus]
        with ops.use_book(book):
            book.match[(N, C, V, Pc, L, 2)] = PRESPLIT_PLAN
            pack = ops.new_pack(N, C, V, L, DEV)
            ops.pack_bank(dk[0], dn[0], pack, 0)
            ops.pack_bank(dk[1], dn[1], pack, 1)
        for path in ('fp32', 'presplit'):
            if Pc == P:
                torch.cuda.synchronize()
                ops.workspace(1, dev).fill_(255)
                poison = torch.full((N, pad128(P), V), float('nan'), device=DEV)
                del poison
            if path == 'fp32':
                mem, _ = ops.match(dq, dk[0], dn[0], dk[1], dn[1], topl, TAU)
            else:
                with ops.use_book(book):
                    mem, _ = ops.match_packed(dq, pack, L, topl, TAU)
            out[(Pc, path)] = mem
    for path in ('fp32', 'presplit'):
        mem = out[(P, path)]
        Pm = mem.stride(0) // V
        full = torch.as_strided(mem, (N, Pm, V), (Pm * V, V, 1))
        assert Pm == 128 and bool(torch.isfinite(full).all()), path
        assert not full[:, P:].any(), path
        assert full[:, :P].abs().max() > 0, path
    ops.check_faults()


# ------------------------------------------------------------------------------------------------------------ 6. clips
@gpu
def test_clips_forms_equal_the_single_clip_calls_at_c64(lib):
    """swem_memorize_packed_clips_f32 / swem_match_packed_clips_f32 with C = 64 and P = 37 (P % 16 != 0; the per-clip key map is
    offset by P * C elements): bases, pack and matching's outputs are bit-identical to one packed call per clip, over two frames,
    with the pre-split readout on the book's default tile and on the planned one."""
    g = torch.Generator().manual_seed(564)
    h, w, C, V, N, T, S, L = 1, 37, 64, 128, 2, 3, 2, 64
    P = h * w
    pm = lambda x: d(x[0].flatten(1).t())                                   # (P, C)
    pv = lambda v: d(v[0].flatten(2).transpose(1, 2))                        # (N, P, V)
    pk = lambda m: d(m[0].flatten(2))                                        # (N, 2, P)
    frames = [[H.em_inputs(h, w, C, V, N, g) for _ in range(S)] for _ in range(2)]
    torch.manual_seed(64)
    prior = []
    for _ in range(S):
        kap, nu, zita = [d(t[0]) for t in O.random_init((1, N, 2, C, L), V)]
        prior.append((kap, nu, zita[:, :, 0].contiguous()))
    qx = [d(H.structured_keys(P, C, 6, g)[0]) for _ in range(S)]
    with ops.use_book(ops.PlanBook(fallback=ops.MODEL_FALLBACK)) as book:
        packs = [ops.new_pack(N, C, V, L, DEV) for _ in range(S)]
        ref = []
        for s_ in range(S):
            b0 = ops.memorize(pm(frames[0][s_][0]), pv(frames[0][s_][1]), pk(frames[0][s_][2]), *prior[s_], T, TAU,
                              pack=packs[s_], prior_packed=False, bank=0)
            ops.pack_bank(b0[0], b0[1], packs[s_], 1)
            b1 = ops.memorize(pm(frames[1][s_][0]), pv(frames[1][s_][1]), pk(frames[1][s_][2]), *b0, T, TAU,
                              pack=packs[s_], prior_packed=True, bank=1)
            ref.append((b0, b1))
        cat = lambda ts: torch.cat(list(ts)).contiguous()
        pack_all = ops.new_pack(S * N, C, V, L, DEV)
        xs = [torch.stack([pm(frames[f][s_][0]) for s_ in range(S)]).contiguous() for f in (0, 1)]
        vs = [cat(pv(frames[f][s_][1]) for s_ in range(S)) for f in (0, 1)]
        ms = [cat(pk(frames[f][s_][2]) for s_ in range(S)) for f in (0, 1)]
        pr = [cat(prior[s_][i] for s_ in range(S)) for i in range(3)]
        a0 = ops.memorize(xs[0], vs[0], ms[0], *pr, T, TAU, pack=pack_all, prior_packed=False, bank=0, clips=S)
        ops.pack_bank(a0[0], a0[1], pack_all, 1)
        a1 = ops.memorize(xs[1], vs[1], ms[1], *a0, T, TAU, pack=pack_all, prior_packed=True, bank=1, clips=S)
        for s_ in range(S):
            for i in range(3):
                assert torch.equal(a0[i][s_ * N:(s_ + 1) * N], ref[s_][0][i]), (s_, i)
                assert torch.equal(a1[i][s_ * N:(s_ + 1) * N], ref[s_][1][i]), (s_, i)
            assert torch.equal(pack_all[0][2 * N * s_:2 * N * (s_ + 1)], packs[s_][0])
            assert torch.equal(pack_all[1][N * s_:N * (s_ + 1)], packs[s_][1])
            assert torch.equal(pack_all[2][N * s_:N * (s_ + 1)].view(torch.int16), packs[s_][2].view(torch.int16))
        assert pack_all[2].any() and bool(torch.isfinite(a1[0]).all()) and bool(torch.isfinite(a1[1]).all())
        qall = torch.stack(qx).contiguous()
        for plan in (0, PRESPLIT_PLAN):
            book.match.clear()
            if plan:
                book.match[(N, C, V, P, L, 2)] = plan
                book.match[(S * N, C, V, P, L, 2)] = plan
            mem_a, S_a = ops.match_packed(qall, pack_all, L, 32, TAU, hw=(h, w), clips=S)
            for s_ in range(S):
                mem_r, S_r = ops.match_packed(qx[s_], packs[s_], L, 32, TAU, hw=(h, w))
                assert torch.equal(mem_a[s_ * N:(s_ + 1) * N], mem_r) and torch.equal(S_a[s_ * N:(s_ + 1) * N], S_r), (plan, s_)
            assert bool(torch.isfinite(mem_a).all()) and bool(torch.isfinite(S_a).all())
    ops.check_faults()
