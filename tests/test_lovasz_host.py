"""CPU: the Lovasz-softmax auxiliary loss without a GPU -- the float64 yardstick (tests/lovasz_ref.py) against what the REFERENCE's
own lovasz_softmax computed (tests/golden/g11_lovasz.npz, fp32 on the CPU), the public switch LOSS.AUX = 'lovasz', the new entry
points' exports, workspace query and argument checks."""
import ctypes

import pytest
import torch

from swem_amd import _lib, losses
from tests import lovasz_ref as LR

CFG = dict(NAME='boots_ce', BS_RATIO=0.30, BS_PERIOD=[20, 70], AUX='lovasz', AUX_RATIO=1.0)


def test_float64_yardstick_matches_the_reference_loss(golden):
    """The loss on both golden clips.  The reference's value is an fp32 dot of 960 products per class: its own distance from the
    float64 value is a few 1e-8 relative (the F32 mode of lovasz_ref, which restates its arithmetic, measures it); the bar is the
    project's loss bar, 2e-6.  Under ties the loss does not depend on the order within a group of equal errors."""
    fx = golden('g11_lovasz.npz')
    for tag in ('safe', 'tie'):
        s, t = fx[tag + '_scores'], fx[tag + '_target']
        want = float(fx[tag + '_loss'])
        got = float(LR.aux_loss(s.double(), t))
        f32 = float(LR.aux_loss(s, t, None, LR.F32))
        print('%s: float64 %.10g  F32 mode %.10g  reference %.10g' % (tag, got, f32, want))
        assert got == pytest.approx(want, rel=2e-6), tag
        assert f32 == pytest.approx(want, rel=2e-6), tag


def test_float64_yardstick_matches_the_reference_gradient_where_there_are_no_ties(golden):
    """d loss / d scores on the tie-free clip.  The reference subtracts neighbouring fp32 Jaccard values: its gradient is some 4e-5
    of the largest entry from the float64 closed form (3.8e-5 on this clip).  So: the F32 mode -- the same arithmetic -- reproduces
    the reference's gradient to rounding (1e-6), and the float64 closed form is within 8x the reference's own measured distance
    of 4e-5 on this shape."""
    fx = golden('g11_lovasz.npz')
    s, t, want = fx['safe_scores'], fx['safe_target'], fx['safe_dlogits'].double()
    s32 = s.clone().requires_grad_(True)
    LR.aux_loss(s32, t, None, LR.F32).backward()
    s64 = s.double().requires_grad_(True)
    LR.aux_loss(s64, t).backward()
    scale = float(want.abs().max())
    e32 = float((s32.grad.double() - want).abs().max()) / scale
    e64 = float((s64.grad - want).abs().max()) / scale
    print('gradient vs the reference: F32 mode %.3g, float64 closed form %.3g' % (e32, e64))
    assert e32 <= 1e-6
    assert e64 <= 8 * 4e-5
    # the order of the safe clip is the same in fp32 and in float64 (that is what safe_case is for)
    for ti in range(s.shape[2]):
        p32 = torch.softmax(s[0, :, ti], 0).flatten(1)
        p64 = torch.softmax(s[0, :, ti].double(), 0).flatten(1)
        lab = t[0, ti].flatten()
        for c in range(s.shape[1]):
            fg = lab == c
            assert torch.equal(LR.class_loss(p32[c], fg, LR.F32)[1], LR.class_loss(p64[c], fg)[1])


def test_closed_form_equals_the_differenced_jaccard_index():
    g = torch.Generator().manual_seed(4)
    for n in (1, 2, 7, 300):
        fg = torch.rand(n, generator=g) < 0.4
        if not fg.any():
            fg[n // 2] = True
        a = LR.weights_closed_form(fg)
        fgd = fg.double()
        jac = 1.0 - (fgd.sum() - fgd.cumsum(0)) / (fgd.sum() + (1.0 - fgd).cumsum(0))
        jac[1:] = jac[1:] - jac[:-1].clone()
        assert float((a - jac).abs().max()) <= 1e-14
        assert float(a.sum()) == pytest.approx(1.0, abs=1e-13)          # (the differences telescope to the last Jaccard value, 1)


def test_safe_case_keeps_its_margin():
    lg, lb, draws = LR.safe_case(400, 3, seed=2)
    e = (torch.nn.functional.one_hot(lb, 3).double() - torch.softmax(lg.double().t(), 1)).abs()
    for c in range(3):
        v = e[:, c].sort().values
        assert float((v[1:] - v[:-1]).min()) >= LR.MARGIN
    assert draws >= 400 and lg.dtype == torch.float32 and lg.shape == (3, 400)


def test_vos_loss_accepts_lovasz():
    crit = losses.VOSLoss(CFG, 100, 'cpu')
    assert crit.aux_alpha == 1.0 and crit._fn is losses._ClipLossLovasz
    assert losses.VOSLoss(dict(CFG, AUX='iou'), 100, 'cpu')._fn is losses._ClipLoss
    assert losses.VOSLoss(dict(CFG, AUX=None), 100, 'cpu')._fn is losses._ClipLoss
    assert losses.get_criterion(CFG).top_k(90, 1000) == (0.3, 300)


def test_unknown_aux_loss_still_raises():
    with pytest.raises(NotImplementedError):
        losses.VOSLoss(dict(CFG, AUX='dice'), 100, 'cpu')


def test_exports_and_workspace_query(lib):
    for name in ('swem_lovasz_workspace', 'swem_lovasz_frame_fwd_f32', 'swem_lovasz_reduce_f32', 'swem_lovasz_frame_bwd_f32'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    w = lib.swem_lovasz_workspace
    base = w(1, 3, 1961)
    assert base >= 1 * 3 * 1961 * 16                    # two (key, payload) buffers of every segment
    assert w(2, 3, 1961) > base and w(1, 8, 1961) > base and w(1, 3, 384 * 384) > base
    assert w(1, 3, 384 * 384) >= 3 * 384 * 384 * 16
    # sizes that cannot be served ask for nothing (and the calls below refuse them)
    assert w(1, 9, 100) == 0 and w(0, 3, 100) == 0 and w(1, 3, 0) == 0 and w(1, 3, 1 << 31) == 0


def test_bad_shapes_are_refused_before_any_launch(lib):
    """Argument validation happens before any HIP call (as tests/test_abi.py::test_version_and_error_channel): no GPU needed."""
    f = ctypes.c_float
    fwd = lib.swem_lovasz_frame_fwd_f32
    assert fwd(None, None, None, 0, None, None, None, None, None, 1, 3, 100, None, 0) == -4
    assert b'null pointer' in lib.swem_last_error()
    assert fwd(None, 1, 1, 0, None, None, 1, None, None, 1, 9, 100, 1, 1 << 30) == -1 and b'N1=9' in lib.swem_last_error()
    assert fwd(None, 1, 1, 0, None, None, 1, None, None, 1, 3, 1 << 31, 1, 1 << 30) == -1 and b'HW=' in lib.swem_last_error()
    assert fwd(None, 1, 1, 0, None, None, 1, None, None, 0, 3, 100, 1, 1 << 30) == -1
    need = lib.swem_lovasz_workspace(2, 3, 5000)
    assert fwd(None, 1, 1, 0, None, None, 1, None, None, 2, 3, 5000, 8, need - 1) == -2 and b'workspace' in lib.swem_last_error()
    assert fwd(None, 1, 1, 0, None, None, 1, None, None, 2, 3, 5000, None, need) == -2
    assert lib.swem_lovasz_reduce_f32(None, None, None, None, 1, 3, 1, 100, 0, None, f(1.0)) == -4
    assert lib.swem_lovasz_reduce_f32(None, 1, 1, 1, 1, 9, 1, 100, 0, None, f(1.0)) == -1
    bwd = lib.swem_lovasz_frame_bwd_f32
    assert bwd(None, 1, 1, 1, 0, None, 1, 1, None, 1, 1, 3, 1, 100, 0, None, f(1.0), None) == -4       # glov missing
    assert bwd(None, 1, 1, 1, 0, None, 1, 1, 1, 1, 1, 3, 1, 1 << 31, 0, None, f(1.0), None) == -1
    with pytest.raises(_lib.SwemHipError, match='lovasz_fwd'):
        _lib.call('swem_lovasz_frame_fwd_f32', None, 1, 1, 0, None, None, 1, None, None, 1, 1, 100, 1, 1 << 30)
