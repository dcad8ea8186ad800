"""Measures the image tolerance of the device augmentation tests (tests/test_gpu_augment.py) -- it is measured, not chosen:
the numpy restatement (tests/augment_ref.py) in float32 against float64 on each parity case's own inputs, outside the
exclusion set; the bar is 4x that maximum.  CPU only.  Writes profiles/augment_parity.json, which the tests read:

    python tools/augment_parity.py [--out profiles/augment_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment_parity.json'))
    args = ap.parse_args()
    from tests import augment_ref as R
    rec = {'what': 'max |restatement in float32 - restatement in float64| over the output frames of each case, outside the '
                   'exclusion set (float64 coordinate within %g px of a threshold); bar = 4 x that' % R.EDGE,
           'exclusion_cap': R.EXCLUSION_CAP, 'cases': {}}
    for name, (seed, B, T, src_hw, out_hw, cell) in R.CASES.items():
        row = {'seed': seed, 'B': B, 'T': T, 'src_hw': list(src_hw), 'out_hw': list(out_hw)}
        row.update(R.measure_bar(name))
        rec['cases'][name] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
