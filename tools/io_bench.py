"""Evaluation staging from decoded bytes (swem_amd.io.davis_sequence_u8, csrc/stage.hip) beside what it replaces.  One
command, writes profiles/io_device.json:

    python tools/io_bench.py [--out profiles/io_device.json]

  * the workload: a T = 70 frame 480x854 DAVIS-sized sequence with two objects, decoded bytes in host memory;
      today   the loader's float conversion on the host (b / 255, HWC -> CHW, stack: data_utils.py:102 + ToTensor), the host
              one-hot mask, the upload of both and `io.stage_sequence` (4.9 MB per frame over PCIe)
      bytes   `io.davis_sequence_u8`: the bytes uploaded once from pinned memory (1.2 MB per frame), everything else on the device
    alternated in ONE call (today, bytes, today, bytes, ...), each run between two device events with a synchronise behind the
    second: wall time of the host work, the copies and the kernels together; medians of seven runs each and their ratio;
  * the overlay pictures and the id-mapped uint8 index maps of the 69 predicted frames (device-resident inputs, seven regions of
    >= 0.3 s), per frame, beside the model's frame time from `python bench.py` started as a child process BEFORE this process
    opens the GPU;
  * accuracy: the cases of tests/test_gpu_io.py -- the new kernel's and today's path's maximum error against float64, and whether
    the two outputs are bit-equal.
No bar was fixed in advance; the claim the record supports or withdraws: staging from bytes is not slower than today's path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.jf_bench import model_frame_ms, timed_regions  # noqa: E402


def once(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'io_device.json'))
    ap.add_argument('--no-model', action='store_true', help='skip the bench.py child (no model frame time in the record)')
    args = ap.parse_args()
    model = None if args.no_model else model_frame_ms()

    import numpy as np
    import torch
    from swem_amd import _lib, dist as sdist, io, ops
    from tests import test_gpu_io as TG
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit('io_bench.py measures on the GPU: no device found')
    sdist.respect_cpu_quota()
    T, H, W = 70, 480, 854
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    first = np.zeros((H, W), np.uint8)
    first[100:300, 150:400] = 1
    first[250:420, 380:700] = 2

    def today():
        fr = (torch.from_numpy(frames).float() / 255.0).permute(0, 3, 1, 2).contiguous().unsqueeze(0)       # the loader's tensors
        onehot = torch.from_numpy((first[None] == np.arange(3, dtype=np.uint8)[:, None, None]).astype(np.int64))
        return io.stage_sequence(fr.to('cuda'), onehot[None, None].to('cuda'))

    def from_bytes():
        return io.davis_sequence_u8(frames, first)[:2]

    a, b = today(), from_bytes()                                  # warm-up, and the two paths side by side
    torch.cuda.synchronize()
    same_mask = bool(torch.equal(a[1][0], b[1][0]))
    frame_diff = float((a[0] - b[0]).abs().max())
    del a, b
    ms = {'today': [], 'bytes': []}
    for _ in range(7):
        ms['today'].append(once(today))
        ms['bytes'].append(once(from_bytes))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    rec = {'workload': 'T = %d frames %dx%d uint8 RGB + one %dx%d index map with two objects, in host memory' % (T, H, W, H, W),
           'staging': {'timing': 'today / bytes alternated in one call; device events around each run, synchronised; ms per sequence',
                       'today_ms': [round(v, 2) for v in ms['today']], 'bytes_ms': [round(v, 2) for v in ms['bytes']],
                       'today_ms_median': round(med['today'], 2), 'bytes_ms_median': round(med['bytes'], 2),
                       'today_over_bytes': round(med['today'] / med['bytes'], 2),
                       'bytes_ms_per_frame': round(med['bytes'] / T, 4), 'today_ms_per_frame': round(med['today'] / T, 4),
                       'first_frame_masks_equal': same_mask, 'max_abs_frame_difference_between_the_paths': frame_diff,
                       'not_slower_than_today': bool(med['bytes'] <= med['today'])},
           'model': model}

    # results side: 69 predicted frames, device resident
    d_frames = torch.from_numpy(frames).cuda()
    idx = torch.from_numpy(rng.integers(0, 3, (T - 1, H, W)).astype(np.int64)).cuda()
    idx[:, 100:300, 150:400] = 1                                   # (large regions besides the noise: blends, not only contours)
    labels = ops.pack_u8(idx)
    pal = np.asarray(io.default_palette(), np.uint8)
    ids = np.asarray([0, 3, 5], np.uint8)
    rows = {}
    for name, fn in (('overlay_u8', lambda: ops.overlay_u8(d_frames[1:], labels, pal, 0.4)),
                     ('pack_u8_lut', lambda: ops.pack_u8_lut(idx, ids)), ('pack_u8', lambda: ops.pack_u8(idx))):
        reps, t = timed_regions(fn)
        m = t[len(t) // 2]
        rows[name] = {'repeats_per_region': reps, 'ms_per_sequence_median': round(m, 4),
                      'spread_pct': round(100 * (t[-1] - t[0]) / m, 2), 'us_per_frame': round(1e3 * m / (T - 1), 3)}
        if model is not None:
            rows[name]['share_of_model_frame_time_pct'] = round(100 * (m / (T - 1)) / model['ms_per_frame'], 3)
    rec['results_side'] = rows

    acc = [TG.stage_case(*case, seed=case[1] * 100 + case[2]) for case in TG.STAGE_CASES]
    u8 = (np.arange(2 * 6 * 10 * 3) % 256).astype(np.uint8).reshape(2, 6, 10, 3)
    ident = ops.stage_frames_u8(torch.from_numpy(u8).cuda(), (6, 10)).cpu().numpy()
    rec['accuracy'] = {'against': 'tests/io_ref.py::stage_frames64 (float64)', 'cases': acc,
                       'identity_equals_fp32_b_over_255_exactly': bool(np.array_equal(
                           ident, (np.arange(256, dtype=np.float32) / 255)[u8].transpose(0, 3, 1, 2)))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
