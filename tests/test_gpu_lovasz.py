"""GPU: the Lovasz-softmax auxiliary loss (csrc/lovasz.hip; LOSS.AUX = 'lovasz') -- the segmented stable radix sort exactly, the
weights and losses along the device's own order against float64, the whole loss and its gradient against the float64 yardstick
(tests/lovasz_ref.py) on inputs no arithmetic can reorder, the tie rule, that the other auxiliary losses did not move, and the
training step eager and replayed.

Bars: the project's per-stage bars (tests/test_gpu_train_edges.py, BARS): loss values 2e-6 relative, dlogits 2e-5 of the largest
gradient, with that file's stand-in rule -- where fp32 arithmetic done the reference's way (lovasz_ref's F32 mode) is not 4x under
a bar on the very case, the case's bar is 8x what the F32 mode measures there."""
import os

import numpy as np
import pytest
import torch

from oracle import swem_oracle as O
from swem_amd import _lib, losses, ops
from tests import helpers as H
from tests import lovasz_ref as LR
from tests.test_gpu_train_edges import BARS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CFG = dict(NAME='boots_ce', BS_RATIO=0.30, BS_PERIOD=[20, 70], AUX='lovasz', AUX_RATIO=1.0)
TILE = 2048            # keys of one sort block (csrc/lovasz.hip: LV_TILE)


def bar_for(name, standin):
    """BARS[name], or 8x the stand-in's own error where the stand-in is not 4x under the bar (test_gpu_train_edges.Sweep.add)"""
    return BARS[name] if standin <= BARS[name] / 4 else 8 * standin


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))


def ranks_of(valid_row, N1):
    """channel -> rank among the valid channels (-1: invalid)"""
    out, r = [], 0
    for c in range(N1):
        ok = valid_row is None or float(valid_row[c]) > 0.5
        out.append(r if ok else -1)
        r += 1 if ok else 0
    return out


def frame_on_device(logits, label, valid):
    """One frame through swem_vos_loss_frame_fwd_f32 (for the device's own prob) and swem_lovasz_frame_fwd_f32 with every test
    output.  logits (B,N1,HW) fp32, label (B,HW) int64, valid (B,N1) or None -- CPU tensors in, CPU tensors out."""
    B, N1, HW = logits.shape
    lg, lb = logits.to(DEV).contiguous(), label.to(DEV).contiguous()
    vd = None if valid is None else valid.to(DEV).contiguous()
    prob = torch.empty((B, N1, HW), dtype=torch.float32, device=DEV)
    raw = torch.empty((B, HW), dtype=torch.float32, device=DEV)
    rowstat = torch.empty((B, 4), dtype=torch.float32, device=DEV)
    iou = torch.empty((B, N1, 2), dtype=torch.float32, device=DEV)
    wsb = max(_lib.query('swem_vos_loss_workspace', B, N1, HW), _lib.query('swem_lovasz_workspace', B, N1, HW))
    ws = ops.workspace(wsb, torch.device(DEV))
    _lib.call('swem_vos_loss_frame_fwd_f32', ops._stream(), lg.data_ptr(), lb.data_ptr(), HW, ops._ptr(vd), prob.data_ptr(),
              raw.data_ptr(), rowstat.data_ptr(), iou.data_ptr(), B, N1, HW, 0, 0, ws.data_ptr(), wsb)
    glov = torch.full((B, N1, HW), float('nan'), dtype=torch.float32, device=DEV)
    lov = torch.full((B, N1, 2), float('nan'), dtype=torch.float32, device=DEV)
    keys = torch.full((B, N1, HW), -1, dtype=torch.int32, device=DEV)
    pay = torch.full((B, N1, HW), -1, dtype=torch.int32, device=DEV)
    _lib.call('swem_lovasz_frame_fwd_f32', ops._stream(), prob.data_ptr(), lb.data_ptr(), HW, ops._ptr(vd), glov.data_ptr(),
              lov.data_ptr(), keys.data_ptr(), pay.data_ptr(), B, N1, HW, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    return prob.cpu(), glov.cpu(), lov.cpu(), keys.cpu(), pay.cpu()


def mixed_logits(B, N1, HW, g):
    """3 * randn, mixed with pixels whose logit gaps are 20 to 100: every byte of the key varies, denormal errors included, and
    exact zeros and ones occur."""
    lg = torch.randn(B, N1, HW, generator=g) * 3
    pick = torch.rand(B, HW, generator=g) < 0.3
    win = torch.randint(0, N1, (B, HW), generator=g)
    gap = 20 + 80 * torch.rand(B, HW, generator=g)
    lg = lg + torch.nn.functional.one_hot(win, N1).permute(0, 2, 1) * (gap * pick)[:, None]
    return lg.float().contiguous()


# (name, B, N1, valid, how the labels are drawn)
CHANNEL_CASES = [
    ('n2', 1, 2, None, 'rand'),
    ('n3_class_absent', 1, 3, None, 'absent1'),            # class 1 does not occur in the frame
    ('n8', 1, 8, None, 'rand'),
    # clip 0 all background; clip 1 has an invalid channel and label values (2) outside its two valid channels
    ('b2_invalid_channel', 2, 3, torch.tensor([[1., 1., 1.], [1., 0., 1.]]), 'bg_and_outside'),
]


def labels_for(how, B, N1, HW, g):
    lb = torch.randint(0, N1, (B, HW), generator=g)
    if how == 'absent1':
        lb[lb == 1] = 0
    elif how == 'bg_and_outside':
        lb[0] = 0
    return lb


def check_frame(case, logits, label, valid):
    """Sections 1 and 2 on one frame: the order exactly, then glov and the channel losses against float64 along that order."""
    B, N1, HW = logits.shape
    prob, glov, lov, keys, pay = frame_on_device(logits, label, valid)
    worst = {'glov': 0.0, 'loss': 0.0}
    sorted_segments = 0
    for b in range(B):
        rk = ranks_of(None if valid is None else valid[b], N1)
        for c in range(N1):
            fg = (label[b] == rk[c]) if rk[c] >= 0 else torch.zeros(HW, dtype=torch.bool)
            G = int(fg.sum())
            if G == 0:                                               # invalid channel or absent class: skipped, not sorted
                assert float(lov[b, c, 1]) == 0.0 and float(lov[b, c, 0]) == 0.0, (case, b, c)
                assert float(glov[b, c].abs().max()) == 0.0, (case, b, c)
                assert bool((keys[b, c] == -1).all()) and bool((pay[b, c] == -1).all()), (case, b, c, 'skipped rows are not written')
                continue
            sorted_segments += 1
            assert float(lov[b, c, 1]) == float(np.float32(G)), (case, b, c)
            k = keys[b, c].to(torch.int64)                           # errors are >= 0: the int32 bits are the unsigned bits
            px = (pay[b, c].to(torch.int64) & 0x7fffffff)
            fgbit = (pay[b, c].to(torch.int64) >> 31) & 1
            # ---- 1. the order, exactly
            assert bool((k[1:] <= k[:-1]).all()), (case, b, c, 'keys must be non-increasing')
            same = k[1:] == k[:-1]
            assert bool((px[1:][same] > px[:-1][same]).all()), (case, b, c, 'equal keys carry ascending pixel indices')
            assert torch.equal(px.sort().values, torch.arange(HW)), (case, b, c, 'payloads are a permutation of the pixels')
            assert torch.equal(fgbit.bool(), fg[px]), (case, b, c, 'fg bits')
            e = (fg.float() - prob[b, c]).abs()
            assert torch.equal(keys[b, c], e[px].view(torch.int32)), (case, b, c, 'keys are the bits of |fg - prob|')
            # ---- 2. values given the device's order (float64 closed form along the device's own permutation)
            g64 = LR.weights_closed_form(fg[px])
            g32 = LR.weights_differenced_f32(fg[px]).double()        # the stand-in: fp32 the reference's way
            want = torch.zeros(HW, dtype=torch.float64)
            want[px] = g64
            scale = float(g64.abs().max())
            err = float((glov[b, c].double() - want).abs().max()) / scale
            sg = float((g32 - g64).abs().max()) / scale
            worst['glov'] = max(worst['glov'], err / bar_for('dlogits', sg))
            e_sorted = e[px].double()
            l64 = float(torch.dot(e_sorted, g64))
            l32 = float(torch.dot(e[px], LR.weights_differenced_f32(fg[px])))
            sl = abs(l32 - l64) / (abs(l64) + 1e-300)
            errl = abs(float(lov[b, c, 0]) - l64) / (abs(l64) + 1e-300)
            if l64 == 0.0:
                assert float(lov[b, c, 0]) == 0.0
            else:
                worst['loss'] = max(worst['loss'], errl / bar_for('loss', sl))
    print('%s HW=%d: %d sorted segments, worst error / bar: %s' % (case, HW, sorted_segments, worst))
    assert worst['glov'] <= 1.0 and worst['loss'] <= 1.0, (case, worst)
    return sorted_segments


@pytest.mark.parametrize('HW', [1, 63, 37 * 53, TILE - 1, 3 * TILE + 77])
def test_sort_order_and_values(lib, HW):
    """Sections 1 and 2 of the issue at every size: one pixel, under a wave, an odd image, one below a sort tile, four tiles with
    a ragged tail; N1 in {2, 3, 8}, two clips with an invalid channel, an absent class, an all-background frame, labels outside
    the valid channels."""
    g = torch.Generator().manual_seed(100 + HW)
    n = 0
    for name, B, N1, valid, how in CHANNEL_CASES:
        n += check_frame(name, mixed_logits(B, N1, HW, g), labels_for(how, B, N1, HW, g), valid)
    assert n >= 3


def test_sort_order_and_values_at_the_training_shape(lib):
    """384 x 384, B=1, N1=3: 72 tiles a segment."""
    g = torch.Generator().manual_seed(7)
    HW = 384 * 384
    assert check_frame('train384', mixed_logits(1, 3, HW, g), labels_for('rand', 1, 3, HW, g), None) == 3


def test_same_inputs_same_bits(lib):
    g = torch.Generator().manual_seed(8)
    lg, lb = mixed_logits(2, 3, 5000, g), labels_for('rand', 2, 3, 5000, g)
    a = frame_on_device(lg, lb, None)
    b = frame_on_device(lg, lb, None)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 3. end to end vs float64
_E2E = {}


def e2e_case(use_valid):
    """The safe clip and its float64 / F32 references per iteration, computed once."""
    if use_valid not in _E2E:
        valid = torch.tensor([[1., 1., 1.], [1., 1., 0.]]) if use_valid else None
        scores, target = LR.safe_clip(2, 2, 3, 37, 53, seed=31 + int(use_valid), valid=valid)
        _E2E[use_valid] = {'scores': scores, 'target': target, 'valid': valid, 'ref': {}}
    return _E2E[use_valid]


def e2e_refs(case, it):
    if it not in case['ref']:
        r64 = LR.loss_and_dlogits(case['scores'], case['target'], it, case['valid'], CFG, LR.F64)
        r32 = LR.loss_and_dlogits(case['scores'], case['target'], it, case['valid'], CFG, LR.F32)
        case['ref'][it] = (r64, r32)
    return case['ref'][it]


def run_clip(cfg, scores, target, it, valid):
    crit = losses.VOSLoss(cfg, 100, DEV)
    T = scores.shape[2]
    frames = [scores[:, :, t].contiguous().to(DEV).requires_grad_(True) for t in range(T)]
    out = crit.clip_loss(frames, target.to(DEV), it, None if valid is None else valid.to(DEV))
    out['total_loss'].backward()
    return crit, out, [f.grad for f in frames]


@pytest.mark.parametrize('it', [5, 45, 90])
@pytest.mark.parametrize('use_valid', [True, False])
def test_lovasz_loss_forward_backward_vs_float64(lib, it, use_valid):
    case = e2e_case(use_valid)
    (l64, d64, p64), (l32, d32, _) = e2e_refs(case, it)
    crit, out, grads = run_clip(CFG, case['scores'], case['target'], it, case['valid'])
    assert out['p'] == pytest.approx(p64)
    bad = {}
    for k in ('total_loss', 'main_loss', 'aux_loss'):
        standin = abs(l32[k] - l64[k]) / abs(l64[k])
        err = abs(float(out[k].detach()) - l64[k]) / abs(l64[k])
        print('%s: hip %.3e  F32 stand-in %.3e  bar %.3e' % (k, err, standin, bar_for('loss', standin)))
        if not err <= bar_for('loss', standin):
            bad[k] = (err, standin)
    for t in range(len(grads)):
        standin = rel(d32[:, :, t], d64[:, :, t])
        err = rel(grads[t], d64[:, :, t])
        print('dlogits frame %d: hip %.3e  F32 stand-in %.3e  bar %.3e' % (t, err, standin, bar_for('dlogits', standin)))
        if not err <= bar_for('dlogits', standin):
            bad['dlogits%d' % t] = (err, standin)
    assert not bad, bad
    # the reference-shaped call (stacked scores) gives the same numbers
    vd = None if case['valid'] is None else case['valid'].to(DEV)
    out2 = crit(case['scores'].to(DEV), case['target'].to(DEV), it, vd)
    assert torch.equal(out2['_vec'].detach(), out['_vec'].detach())


def test_loss_matches_the_reference_on_the_golden_clip(golden, lib):
    """The auxiliary loss of the golden's tie-free clip against what the reference's own lovasz_softmax computed for it."""
    fx = golden('g11_lovasz.npz')
    _, out, _ = run_clip(CFG, fx['safe_scores'], fx['safe_target'], 5, None)
    assert float(out['aux_loss']) == pytest.approx(float(fx['safe_loss']), rel=BARS['loss'])


# ------------------------------------------------------------------------------------------------------------ 4. ties
def test_ties(golden, lib):
    """Saturated logits (errors exactly 0 and 1) and blocks of bit-identical logit vectors: the loss is the reference's, the
    gradient is the float64 yardstick's under the stated tie rule, and pixels whose errors are all 0 get no Lovasz gradient."""
    fx = golden('g11_lovasz.npz')
    scores, target = fx['tie_scores'], fx['tie_target']
    _, out, grads = run_clip(CFG, scores, target, 5, None)
    assert float(out['aux_loss']) == pytest.approx(float(fx['tie_loss']), rel=BARS['loss'])
    l64, d64, _ = LR.loss_and_dlogits(scores, target, 5, None, CFG, LR.F64)
    l32, d32, _ = LR.loss_and_dlogits(scores, target, 5, None, CFG, LR.F32)
    assert float(out['aux_loss']) == pytest.approx(l64['aux_loss'], rel=bar_for('loss', abs(l32['aux_loss'] - l64['aux_loss']) / l64['aux_loss']))
    for t in range(len(grads)):
        standin = rel(d32[:, :, t], d64[:, :, t])
        err = rel(grads[t], d64[:, :, t])
        print('ties, dlogits frame %d: hip %.3e  F32 stand-in %.3e' % (t, err, standin))
        assert err <= bar_for('dlogits', standin), (t, err, standin)
    # e == 0 on every channel (saturated and labelled with the winner): d e / d p = sign(0) = 0, so the pixel's gradient is the
    # cross-entropy gradient alone -- bit for bit what AUX=None computes there
    _, _, plain = run_clip(dict(CFG, AUX=None), scores, target, 5, None)
    n = 0
    for t in range(len(grads)):
        p = torch.softmax(scores[0, :, t].to(DEV), 0)                                      # exactly 0 / 1 on saturated pixels
        fg = torch.nn.functional.one_hot(target[0, t].to(DEV), scores.shape[1]).permute(2, 0, 1).float()
        zero = ((fg - p).abs() == 0).all(0)
        n += int(zero.sum())
        assert torch.equal(grads[t][0][:, zero], plain[t][0][:, zero])
    assert n > 100


# ------------------------------------------------------------------------------------------------ 5. nothing else moved
def test_other_aux_losses_did_not_move(lib):
    g = torch.Generator().manual_seed(21)
    scores = torch.randn(2, 3, 2, 37, 53, generator=g) * 3
    target = torch.randint(0, 3, (2, 2, 37, 53), generator=g)
    valid = torch.tensor([[1., 1., 1.], [1., 1., 0.]])
    target[1] = target[1].clamp(max=1)
    iou_cfg = dict(CFG, AUX='iou')
    _, a, ga = run_clip(iou_cfg, scores, target, 45, valid)
    run_clip(CFG, scores, target, 45, valid)                       # the Lovasz stage on the same stream and workspace in between
    _, b, gb = run_clip(iou_cfg, scores, target, 45, valid)
    assert torch.equal(a['_vec'].detach(), b['_vec'].detach())
    for x, y in zip(ga, gb):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # AUX_RATIO = 0: the Lovasz backward's cross-entropy half is the existing kernel's (equal as numbers: the two kernels may
    # differ in the sign of a zero, which torch.equal does not tell apart)
    _, c, gc = run_clip(dict(CFG, AUX_RATIO=0.0), scores, target, 45, valid)
    _, d, gd = run_clip(dict(CFG, AUX=None), scores, target, 45, valid)
    assert torch.equal(c['_vec'].detach()[:2], d['_vec'].detach()[:2])
    for x, y in zip(gc, gd):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------ 6. the step
def _step_setup():
    tc = H.train_cases()
    case = dict(tc['cases']['r18'], hw=[64, 64])
    cfg = O.make_cfg(**case['cfg'])
    assert cfg.BACKBONE == 'resnet18' and cfg.NUM_BASES == 64 and case['b'] == 2
    return tc, case, cfg, dict(tc['loss_cfg'], AUX='lovasz')


def test_one_step_matches_the_oracle_with_the_lovasz_yardstick(lib, monkeypatch):
    """SWEMTrainer.one_step with LOSS.AUX = 'lovasz' against oracle.swem_oracle.train_one_step whose vos_loss is replaced, here in
    the test, by tests/lovasz_ref.py's.  Tolerances: test_one_step_matches_reference_trainer's (losses 1e-4 or 5x the reference's
    own fp32-vs-float64 floor of the r18 fixture; gradient norms as the oracle-run steps of tests/test_gpu_train.py)."""
    from swem_amd.train import SWEMTrainer
    tc, case, cfg, loss_cfg = _step_setup()
    model, sd = H.make_model_and_sd(cfg, case['wseed'], DEV, pred_scale=tc['pred_scale'])
    frames, init_mask, label, valid = H.train_batch(case)
    monkeypatch.setattr(O, 'vos_loss', lambda s, t, it, v, lc: LR.vos_loss(s, t, it, v, lc))
    torch.manual_seed(23)
    ref_l, ref_res, ref_g, _ = O.train_one_step(H.trainable_sd(sd, model), cfg, frames, init_mask, valid, label, 45, loss_cfg)
    tr = SWEMTrainer(dict(SOLVER=tc['solver_cfg'], LOSS=loss_cfg, AMP=False), model, use_graph=False)
    torch.manual_seed(23)
    out, results = tr.one_step(frames.to(DEV), init_mask.to(DEV), valid.to(DEV), label.to(DEV), 45)
    with np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g9_train_r18_it45.npz')) as fx:
        floor = float(fx['floor64_loss'])
    got = {k: float(out[k]) for k in ('total_loss', 'main_loss', 'aux_loss')}
    want = {k: float(ref_l[k].detach()) for k in got}
    print('losses', got, 'oracle', want, 'tolerance', max(1e-4, 5 * floor))
    for k in got:
        assert got[k] == pytest.approx(want[k], rel=max(1e-4, 5 * floor)), k
    assert want['aux_loss'] > 0.05
    params = dict(model.named_parameters())
    rels = sorted(abs(float(params[k].grad.double().norm()) - float(g_.double().norm())) / (float(g_.double().norm()) + 1e-12)
                  for k, g_ in ref_g.items() if g_ is not None)
    print('gradient norms: median rel err %.2e, 90%% %.2e, worst %.2e' % (rels[len(rels) // 2], rels[int(len(rels) * 0.9)], rels[-1]))
    assert rels[len(rels) // 2] < 1e-3 and rels[int(len(rels) * 0.9)] < 2e-2


@pytest.mark.parametrize('lanes', [None, 1])
def test_replayed_steps_equal_eager_steps_and_the_loss_goes_down(lib, lanes):
    """In the manner of test_graph_replay_equals_eager_steps: five steps eager and five with the step captured after the second
    (three replays) -- same losses, same parameters, bit for bit.  The replaying trainer then goes on to twenty steps on the fixed
    batch (same random bases every step): aux_loss goes down.  lanes=None: a lane per clip; lanes=1: both clips as one batch
    through the loss (the clip-batched step)."""
    from swem_amd import train
    from swem_amd.train import SWEMTrainer
    tc, case, cfg, loss_cfg = _step_setup()
    frames, init_mask, label, valid = [t.to(DEV) for t in H.train_batch(case)]
    torch.manual_seed(4)
    fixed = train.random_init_host(2, case['n'], 128, cfg.NUM_BASES)
    real = train.random_init_host
    train.random_init_host = lambda B, N, Cc, Lb: fixed.clone()
    out = {}
    try:
        for mode in (False, True):
            model, _ = H.make_model_and_sd(cfg, case['wseed'], DEV, pred_scale=tc['pred_scale'])
            solver = dict(tc['solver_cfg'], BASE_LR=1e-4, PRETRAIN_ITERS=[1000, 2000])
            tr = SWEMTrainer(dict(SOLVER=solver, LOSS=loss_cfg, AMP=False), model, use_graph=mode, lanes=lanes)
            hist = []
            for it in (18, 19, 45, 71, 5):
                ls, results = tr.one_step(frames, init_mask, valid, label, it)
                hist.append((float(ls['total_loss']), float(ls['main_loss']), float(ls['aux_loss']), ls['p'], int(results.sum())))
            assert (tr._graph is not None) == mode
            out[mode] = (hist, tr.optimizer.param.detach().clone())
            if mode:
                aux = [h[2] for h in hist]
                for _ in range(15):
                    ls, _r = tr.one_step(frames, init_mask, valid, label, 45)
                    aux.append(float(ls['aux_loss']))
    finally:
        train.random_init_host = real
    for a, b in zip(out[False][0], out[True][0]):
        assert a == b, (a, b)
    assert torch.equal(out[False][1], out[True][1])
    print('aux_loss over twenty steps:', ' '.join('%.5f' % v for v in aux))
    assert len(aux) == 20 and aux[-1] < aux[0] and len(set(aux)) == 20
