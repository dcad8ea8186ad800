#!/usr/bin/env python
"""Generates tests/golden/g10_io.npz by RUNNING THE REFERENCE's own host functions on seeded small inputs (the reference is
read-only and imported by file path, cv2 stubbed as make_golden.py stubs its modules; it needs scipy, which the reference's
add_overlay uses):

    python tests/golden/make_golden_io.py        (build container only: the reference never travels)

  utils/visualization.py::add_overlay        on random label maps (with and without a background label, touching objects, image
                                             edges, single pixels) and random images, BGR image + reversed colour as save_overlay
                                             passes them; stored swapped back to RGB, which is what cv2.imwrite puts in the file
  datasets/data_utils.py::to_onehot_tensor   as DAVIS_Test.py:43-48 calls it (with and without single_obj)
  datasets/YTVOS_Test.py::get_suit_size      on 0..2000

NOT run, because they live inside YTVOS_Test.__getitem__ and need a dataset on disk plus cv2: the YouTube-VOS one-hot loop
(:116-132) and its size rule (:75-91).  tests/io_ref.py restates those two by reading; only get_suit_size underneath the size
rule is the reference's own here.  The fixture holds inputs and outputs (data), never reference source; every restatement of
tests/io_ref.py is checked against it while it is written.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
REF = os.environ.get('SWEM_REFERENCE') or os.path.abspath(os.path.join(ROOT, '..', 'reference'))   # a checkout beside this one
sys.path.insert(0, ROOT)

from tests import io_ref  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))            # imported at module level, not used by what runs here
    try:
        import scipy.ndimage.morphology  # noqa: F401
    except ImportError:                                               # newer scipy: the old module path is gone
        import scipy.ndimage
        m = types.ModuleType('scipy.ndimage.morphology')
        m.binary_dilation = scipy.ndimage.binary_dilation
        sys.modules['scipy.ndimage.morphology'] = m
    vis = _load('ref_visualization', os.path.join(REF, 'utils', 'visualization.py'))
    pkg = types.ModuleType('datasets')
    pkg.__path__ = [os.path.join(REF, 'datasets')]
    sys.modules['datasets'] = pkg
    du = _load('datasets.data_utils', os.path.join(REF, 'datasets', 'data_utils.py'))
    dt = types.ModuleType('datasets.data_transform')                  # (YTVOS_Test.py imports ToTensor; never called here)
    dt.ToTensor = object
    sys.modules['datasets.data_transform'] = dt
    if not hasattr(np, 'bool'):
        np.bool = bool                                                # (YTVOS_Test.py:51 predates numpy 1.24; not reached here)
    yt = _load('datasets.YTVOS_Test', os.path.join(REF, 'datasets', 'YTVOS_Test.py'))
    return vis, du, yt


def random_mask(rng, h, w, labels, blobs):
    """Rectangles of random labels over a base label: touching objects, objects on the image edges, single pixels."""
    m = np.full((h, w), labels[0], np.uint8)
    for _ in range(blobs):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        hh, ww = int(rng.integers(1, max(2, h // 2))), int(rng.integers(1, max(2, w // 2)))
        m[y0:y0 + hh, x0:x0 + ww] = labels[int(rng.integers(0, len(labels)))]
    return m


def main():
    vis, du, yt = import_reference()
    from swem_amd.io import default_palette
    rng = np.random.default_rng(1010)
    pal = np.asarray(default_palette(), np.uint8).reshape(256, 3)
    out = {'palette': pal}

    # ---- add_overlay: the label sets include one without 0 (ids[1:] then skips a real object) and non-contiguous ids
    cases = [((9, 13), [0, 1, 2, 3], 6), ((12, 10), [0, 2, 5], 5), ((8, 8), [1, 2, 3], 6), ((1, 9), [0, 1, 4], 3),
             ((7, 1), [0, 3], 2), ((1, 1), [2], 0), ((16, 20), [0, 1, 2, 3, 4, 5, 6, 7, 255], 14), ((10, 12), [3, 7, 200], 7)]
    for k, ((h, w), labels, blobs) in enumerate(cases):
        mask = random_mask(rng, h, w, labels, blobs)
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)                          # RGB, as decoded
        alpha = (0.4, 0.4, 0.4, 0.4, 0.4, 0.4, 0.25, 0.7)[k]
        got_bgr = vis.add_overlay(img[..., ::-1].copy(), mask, pal.reshape(-1), alpha)  # save_overlay: BGR image, palette
        got = got_bgr[..., ::-1]                                                         # cv2.imwrite stores it as RGB again
        assert np.array_equal(io_ref.add_overlay(img, mask, pal, alpha), got), 'io_ref.add_overlay differs (case %d)' % k
        assert np.array_equal(io_ref.overlay_closed(img, mask, pal, alpha), got), 'closed form differs (case %d)' % k
        out['ov%d_img' % k], out['ov%d_mask' % k], out['ov%d_out' % k] = img, mask, np.ascontiguousarray(got)
        out['ov%d_alpha' % k] = np.float64(alpha)
    out['ov_n'] = np.int64(len(cases))
    # the closed form on many more random masks than the fixture stores
    bad = 0
    for _ in range(300):
        h, w = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        labels = sorted(set(int(v) for v in rng.integers(0, 7, int(rng.integers(1, 6)))))
        mask = random_mask(rng, h, w, labels, int(rng.integers(0, 8)))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = vis.add_overlay(img[..., ::-1].copy(), mask, pal.reshape(-1), 0.4)[..., ::-1]
        bad += not np.array_equal(io_ref.overlay_closed(img, mask, pal, 0.4), want)
    print('closed form vs the reference add_overlay on 300 random masks: %d mismatches' % bad)
    assert bad == 0

    # ---- to_onehot_tensor as DAVIS_Test.__getitem__ calls it
    oh_cases = [((3, 5), [0, 1]), ((7, 9), [0, 1, 3]), ((6, 6), [0, 2, 3, 11]), ((5, 4), [1, 2]), ((4, 4), [0])]
    n = 0
    for (h, w), labels in oh_cases:
        mask = random_mask(rng, h, w, labels, 5)
        for single in (False, True):
            m = mask.astype(np.int64)
            if single:
                m[m > 1] = 1
            obj_n = int(m.max()) + 1
            got, _, _ = du.to_onehot_tensor(m, obj_n, shuffle=False, valid_shuffle=False)
            assert np.array_equal(io_ref.onehot_davis(mask, single), got.astype(np.float32)), 'io_ref.onehot_davis differs'
            out['oh%d_mask' % n], out['oh%d_single' % n], out['oh%d_out' % n] = mask, np.int64(single), got.astype(np.uint8)
            n += 1
    out['oh_n'] = np.int64(n)

    # ---- get_suit_size
    sizes = np.arange(0, 2001, dtype=np.int64)
    suit = np.asarray([yt.get_suit_size(int(s)) for s in sizes], np.int64)
    assert all(io_ref.suit_size(int(s)) == int(v) for s, v in zip(sizes, suit))
    out['suit_in'], out['suit_out'] = sizes, suit

    path = os.path.join(HERE, 'g10_io.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
