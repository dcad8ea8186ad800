"""Measures the image tolerance of the stage-0 device tests (tests/test_gpu_synth.py) -- it is measured, not chosen: the numpy
restatement of the static chain (tests/synth_ref.py) in float32 against float64 on each case's own inputs, outside the exclusion
set; the bar is 4x that maximum (the rule of tools/augment_parity.py).  Writes profiles/synth_parity.json, which the tests read:

    python tools/synth_parity.py [--out profiles/synth_parity.json] [--device]

The bars need no GPU.  With --device the device's own error against float64 is measured too and written beside each bar (the
restatement is fed the device's composites, as in the tests); without it, figures a former run recorded are kept.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_error(name):
    import numpy as np
    import torch
    from swem_amd import augment as A
    from tests import synth_ref as S
    _seed, N, out_hw, _sizes = S.CASES[name]
    imgs, masks, clips = S.drawn_case(name)
    syn = A.StaticClipSynthesizer(out_hw, N, S.T, S.SLOT_HW, device='cuda:0')
    out = syn(torch.from_numpy(imgs).to('cuda:0'), torch.from_numpy(masks).to('cuda:0'), clips)
    B = len(clips)
    comp, comp_lab = [t.cpu().numpy() for t in syn.composites(B)]
    ref = S.static_batch(comp, comp_lab, clips, N)
    keep = ~ref['exclude']
    err = np.abs(out[0].cpu().numpy().astype(np.float64) - ref['frames']).max(axis=2)
    cref = S.composite_case(imgs, masks, clips)
    flips = sum(int((comp[b][:, :c['frames'].shape[1], :c['frames'].shape[2]] != c['frames']).any(-1)[~c['exclude']].sum())
                for b, c in enumerate(cref))
    return {'device_vs_fp64_max': float(err[keep].max()), 'composite_bytes_differing_outside_exclusion': flips}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'synth_parity.json'))
    ap.add_argument('--device', action='store_true', help='also measure the device (needs a GPU)')
    args = ap.parse_args()
    from tests import synth_ref as S
    old = {}
    if os.path.exists(args.out):
        old = json.load(open(args.out)).get('cases', {})
    rec = {'what': 'max |static chain in float32 - in float64| (tests/synth_ref.py) over the output frames of each case, outside '
                   'the exclusion set (float64 coordinate within %g px of a threshold); bar = 4 x that; device_vs_fp64_max: the '
                   'device against float64 on its own composites, same set' % S.EDGE,
           'exclusion_cap': S.EXCLUSION_CAP, 'cases': {}}
    for name, (seed, N, out_hw, sizes) in S.CASES.items():
        row = {'seed': seed, 'N': N, 'T': S.T, 'out_hw': list(out_hw), 'sizes': sizes, 'slot_hw': list(S.SLOT_HW)}
        row.update(S.measure_bar(name))
        if args.device:
            row.update(device_error(name))
        else:
            row.update({k: v for k, v in old.get(name, {}).items() if k in ('device_vs_fp64_max',
                                                                             'composite_bytes_differing_outside_exclusion')})
        rec['cases'][name] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
