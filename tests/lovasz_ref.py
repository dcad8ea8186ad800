"""The yardstick of the Lovasz-softmax auxiliary loss (LOSS.AUX = 'lovasz'): a float64 restatement, by reading, of what the
reference computes (losses/__init__.py:34-63 calling lovasz_losses.py:155-220 with classes='present', per_image=True), with the
two choices the HIP build fixes:

  - the order is STABLE: descending error, ties by ascending pixel (the reference's torch.sort leaves ties undefined);
  - the weight of position k comes from INTEGER counts in closed form -- G foreground pixels, cf of them before k,
    U = G + (k - cf):  g = 1 / U on a foreground pixel, (G - cf) / (U (U + 1)) on a background pixel -- which equals the
    reference's jaccard[k] - jaccard[k-1] (jaccard[0] undifferenced) without the cancellation of two neighbouring quotients.

d|x|/dx is 0 at 0 (torch.abs).  `F32` mode does the same in fp32 the REFERENCE's way (fp32 softmax, fp32 cumulative sums,
neighbouring fp32 Jaccard values subtracted): the stand-in that says what fp32 arithmetic itself can keep on a case.
The reference's own function runs in fp32 only (lovasz_grad calls .float(), so torch.dot refuses float64 inputs): the golden
(tests/golden/g11_lovasz.npz) pins this file to it on the CPU, tests/test_lovasz_host.py.
"""
import math

import torch
import torch.nn.functional as F

from oracle import swem_oracle as O

F64, F32 = 'f64', 'f32'
MARGIN = 2e-5          # about 100 fp32 ulps of a probability: errors this far apart cannot be reordered by fp32 rounding


def weights_closed_form(fg_sorted):
    """g along the sorted order from integer counts (float64).  fg_sorted: bool / 0-1 tensor (P,)."""
    fg = fg_sorted.to(torch.int64)
    G = int(fg.sum())
    cf = torch.cumsum(fg, 0) - fg                                   # foreground pixels strictly before k
    k = torch.arange(fg.numel(), dtype=torch.int64)
    U = (G + (k - cf)).double()
    return torch.where(fg > 0, 1.0 / U, (G - cf).double() / (U * (U + 1.0)))


def weights_differenced_f32(fg_sorted):
    """The same weights as fp32 Jaccard values subtracted from their neighbours (what lovasz_losses.py:19-31 does)."""
    fg = fg_sorted.float()
    total = fg.sum()
    jac = 1.0 - (total - fg.cumsum(0)) / (total + (1.0 - fg).cumsum(0))
    if fg.numel() > 1:
        jac[1:] = jac[1:] - jac[:-1]
    return jac


def class_loss(prob_c, fg, mode=F64):
    """One image, one class: prob_c (P,) with grad, fg (P,) bool.  Returns (loss, permutation)."""
    e = (fg.to(prob_c.dtype) - prob_c).abs()
    e_sorted, perm = torch.sort(e, dim=0, descending=True, stable=True)   # stable + descending: ties keep ascending pixel order
    g = weights_closed_form(fg[perm]) if mode == F64 else weights_differenced_f32(fg[perm])
    return torch.dot(e_sorted, g.to(e.dtype)), perm


def image_loss(prob, label, mode=F64):
    """One image: prob (C,H,W), label (H,W).  Mean over the classes present in the image, 0 (no gradient) without one."""
    C = prob.shape[0]
    lab = label.reshape(-1)
    out = []
    for c in range(C):
        fg = lab == c
        if int(fg.sum()) == 0:
            continue
        out.append(class_loss(prob[c].reshape(-1), fg, mode)[0])
    if not out:
        return prob.sum() * 0.0
    return sum(out) / len(out)


def aux_loss(scores, target, valid_obj=None, mode=F64):
    """losses/__init__.py:45-56 with aux_loss = lovasz_softmax.  scores (B,N+1,T,H,W) logits, target (B,T,H,W) int64, valid_obj
    (B,N+1) or None.  The softmax runs in scores' dtype: pass .double() logits for the float64 yardstick, fp32 ones for F32."""
    B, _, T = scores.shape[:3]
    tot = 0.0
    for b in range(B):
        cur = scores[b] if valid_obj is None else scores[b][valid_obj[b] > 0.5]
        pred = F.softmax(cur.transpose(0, 1), dim=1)                 # T x Nv x H x W
        tot = tot + sum(image_loss(pred[t], target[b, t], mode) for t in range(T)) / T
    return tot / B


def vos_loss(scores, target, it, valid_obj, loss_cfg, mode=F64):
    """oracle.swem_oracle.vos_loss with the Lovasz-softmax loss as the auxiliary loss (same signature and dict)."""
    main, p = O.bootstrapped_ce(scores, target, it, valid_obj, loss_cfg['BS_PERIOD'][0], loss_cfg['BS_PERIOD'][1],
                                loss_cfg['BS_RATIO'])
    aux = aux_loss(scores, target, valid_obj, mode)
    return {'total_loss': main + loss_cfg['AUX_RATIO'] * aux, 'main_loss': main, 'aux_loss': aux, 'p': p}


def loss_and_dlogits(scores, target, it, valid_obj, loss_cfg, mode=F64):
    """Losses (floats) and d total / d scores.  F64: everything in float64; F32: everything in fp32, the reference's way."""
    s = scores.detach().to(torch.float64 if mode == F64 else torch.float32).clone().requires_grad_(True)
    out = vos_loss(s, target, it, valid_obj, loss_cfg, mode)
    out['total_loss'].backward()
    return {k: float(out[k].detach()) for k in ('total_loss', 'main_loss', 'aux_loss')}, s.grad, out['p']


# ------------------------------------------------------------------------------------------------------------------ inputs
def safe_case(n_pixels, C, seed, margin=MARGIN, scale=3.0):
    """Logits (C, n_pixels) float32 and labels (n_pixels,) of ONE image whose per-class errors |fg - softmax| (taken in float64
    from the fp32 logits) are pairwise at least `margin` apart within every class: fp32 rounding cannot reorder the pixels, so
    every correct implementation sorts them alike.  Pixels are drawn one at a time and rejected otherwise; errors are bucketed at
    `margin`, only the three neighbouring buckets are looked at.  Returns (logits, labels, draws)."""
    g = torch.Generator().manual_seed(seed)
    buckets = [dict() for _ in range(C)]
    cols, labs, draws = [], [], 0
    while len(cols) < n_pixels:
        m = 4096
        lg = (torch.randn(m, C, generator=g) * scale).float()
        lb = torch.randint(0, C, (m,), generator=g)
        e = (F.one_hot(lb, C).double() - F.softmax(lg.double(), dim=1)).abs().tolist()
        for i in range(m):
            draws += 1
            ok = True
            for c in range(C):
                x = e[i][c]
                q = int(math.floor(x / margin))
                for nb in (q - 1, q, q + 1):
                    for y in buckets[c].get(nb, ()):
                        if abs(x - y) < margin:
                            ok = False
                if not ok:
                    break
            if not ok:
                continue
            for c in range(C):
                buckets[c].setdefault(int(math.floor(e[i][c] / margin)), []).append(e[i][c])
            cols.append(lg[i])
            labs.append(int(lb[i]))
            if len(cols) == n_pixels:
                break
    return torch.stack(cols, 1).contiguous(), torch.tensor(labs, dtype=torch.int64), draws


def safe_clip(B, T, C, H, W, seed, valid=None):
    """scores (B,C,T,H,W) float32 and target (B,T,H,W): every frame a safe_case over the clip's VALID channels (labels index them
    in order); an invalid channel holds plain random logits."""
    scores = torch.zeros(B, C, T, H, W)
    target = torch.zeros(B, T, H, W, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed + 7919)
    for b in range(B):
        on = [c for c in range(C) if valid is None or float(valid[b][c]) > 0.5]
        for t in range(T):
            lg, lb, _ = safe_case(H * W, len(on), seed + 101 * b + 13 * t)
            scores[b, :, t] = torch.randn(C, H, W, generator=g) * 3
            scores[b, on, t] = lg.view(len(on), H, W)
            target[b, t] = lb.view(H, W)
    return scores, target


def tie_clip(T, C, H, W, seed):
    """A clip full of ties: saturated pixels (logit gaps of +-200: probabilities exactly 0 and 1 in fp32 and in float64, errors
    exactly 0 and 1) and blocks of pixels with bit-identical logit vectors.  scores (1,C,T,H,W) float32, target (1,T,H,W)."""
    g = torch.Generator().manual_seed(seed)
    P = H * W
    scores = torch.zeros(1, C, T, P)
    target = torch.zeros(1, T, P, dtype=torch.int64)
    for t in range(T):
        lg = (torch.randn(C, P, generator=g) * 3).float()
        lb = torch.randint(0, C, (P,), generator=g)
        third = P // 3
        win = torch.randint(0, C, (third,), generator=g)            # saturated: one channel at +200, the others at 0
        sat = torch.zeros(C, third)
        sat[win, torch.arange(third)] = 200.0
        lg[:, :third] = sat
        # (two thirds of the saturated pixels are labelled with their winner: errors exactly 0; the rest exactly 1 and 0)
        lb[:third] = torch.where(torch.arange(third) % 3 < 2, win, (win + 1) % C)
        for s in range(third, 2 * third, 16):                        # blocks of 16 identical logit vectors, labels mixed
            lg[:, s:s + 16] = lg[:, s:s + 1]
        scores[0, :, t] = lg
        target[0, t] = lb
    return scores.view(1, C, T, H, W).contiguous(), target.view(1, T, H, W).contiguous()
