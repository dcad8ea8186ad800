#!/usr/bin/env python
"""Generates tests/golden/g11_lovasz.npz by RUNNING THE REFERENCE's own losses/lovasz_losses.py::lovasz_softmax (defaults:
classes='present', per_image=True) on the CPU in fp32, as losses/__init__.py:45-48 calls it with valid_obj=None:

    python tests/golden/make_golden_lovasz.py        (build container only: the reference never travels)

The module is loaded by file path (importlib.util.spec_from_file_location) and needs torch and numpy only.

  safe_*   a tests/lovasz_ref.py::safe_clip (B=1, T=2, C=3, 24x40: no two errors of a class closer than 2e-5, so the order is
           the same in every arithmetic): scores, target, the reference's loss and its d loss / d scores
  tie_*    a tests/lovasz_ref.py::tie_clip (saturated pixels and blocks of identical logits): scores, target and the loss only --
           the reference's gradient under ties depends on the order an unstable sort happens to leave

The fixture holds inputs and outputs (data), never reference source.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
REF = os.environ.get('SWEM_REFERENCE') or os.path.abspath(os.path.join(ROOT, '..', 'reference'))   # a checkout beside this one
sys.path.insert(0, ROOT)

from tests import lovasz_ref as LR  # noqa: E402


def reference_loss(mod, scores, target, grad):
    """losses/__init__.py:45-48 for valid_obj=None: softmax over the channels, the (B*T) images averaged."""
    s = scores.clone().requires_grad_(grad)
    B, N, T, H, W = s.shape
    pred = F.softmax(s.transpose(1, 2), dim=2).reshape(B * T, N, H, W)
    loss = mod.lovasz_softmax(pred, target.contiguous().view(B * T, H, W))
    if grad:
        loss.backward()
    return float(loss.detach()), (s.grad if grad else None)


def main():
    spec = importlib.util.spec_from_file_location('ref_lovasz_losses', os.path.join(REF, 'losses', 'lovasz_losses.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    out = {}
    scores, target = LR.safe_clip(1, 2, 3, 24, 40, seed=11)
    loss, grad = reference_loss(mod, scores, target, True)
    out.update(safe_scores=scores.numpy(), safe_target=target.numpy(), safe_loss=np.float64(loss), safe_dlogits=grad.numpy())
    scores, target = LR.tie_clip(2, 3, 24, 40, seed=12)
    loss, _ = reference_loss(mod, scores, target, False)
    out.update(tie_scores=scores.numpy(), tie_target=target.numpy(), tie_loss=np.float64(loss))
    path = os.path.join(HERE, 'g11_lovasz.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes; safe loss %.9g, tie loss %.9g' % (out['safe_loss'], out['tie_loss']))


if __name__ == '__main__':
    main()
