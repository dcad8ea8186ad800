"""Result PNGs encoded on the device (io.IndexMapWriter(encode='device'), csrc/png.hip) beside the host path it replaces
(encode='host': the maps cross at full size, PIL writes them on four threads).  One command, writes profiles/png_device.json:

    python tools/png_bench.py [--out profiles/png_device.json] [--no-model]

  * the sequence: the 69 predicted index maps of a 70-frame 480x854 clip with two objects -- the bench model's own predictions
    (bench.py's weights, configuration and shipped plans on a synth.make_clip clip, through evaluator.evaluate_davis_seq), and
    beside them synthetic discs with ragged edges (the bench model has random weights: its maps are not what a trained model
    draws);
  * per content and per path, alternated host / device in ONE process, medians of `--repeats` runs each:
      device time   device events on the submitting stream around `submit` (pack_u8, and the encoder's three launches), per frame
      host CPU      time.process_time across submit .. close (every thread of the process), per frame
      wall          time.perf_counter from before `submit` to after `close`: the files are written and closed
      bytes copied device-to-host, total file bytes, and their ratio to PIL's
    and the device files decoded with PIL against the host files: every map equal;
  * the encoder alone (`ops.png_encode_u8`, seven regions of >= 0.3 s) per frame, beside the model's frame time from
    `python bench.py` started as a child process BEFORE this process opens the GPU.
No speed or size bar was fixed in advance; the record states what was measured."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.jf_bench import model_frame_ms, timed_regions  # noqa: E402

T, H, W, N_OBJ = 70, 480, 854, 2


def synthetic_blobs(seed=7):
    """69 maps: two discs drifting across the frame, every row's two edges moved by up to 3 pixels."""
    import numpy as np
    rng = np.random.default_rng(seed)
    yy = np.arange(H, dtype=np.float64)[:, None]
    xx = np.arange(W, dtype=np.float64)[None, :]
    out = np.zeros((T - 1, H, W), np.uint8)
    for t in range(T - 1):
        for label, (cy, cx, r, vx) in enumerate([(200.0, 250.0, 110.0, 3.0), (300.0, 560.0, 90.0, -2.0)], 1):
            half = np.sqrt(np.maximum(r * r - (yy - cy) ** 2, 0.0))
            left = cx + vx * t - half + rng.integers(-3, 4, (H, 1))
            right = cx + vx * t + half + rng.integers(-3, 4, (H, 1))
            out[t][(half > 0) & (xx >= left) & (xx <= right)] = label
    return out


def model_predictions():
    """The bench model (bench.py: weights, configuration, shipped plans) on a 70-frame synthetic clip -> 69 uint8 maps."""
    from types import SimpleNamespace
    import torch
    import bench
    from swem_amd import evaluator, ops, synth, weights
    from swem_amd.swem import SWEM
    cfg = SimpleNamespace(**dict(dict(KEYDIM=128, VALDIM=512, NUM_BASES=256, NUM_EM_ITERS=4, EM_TAU=0.05, TOPL=64, SINGLE_OBJ=False,
                                      BACKBONE='resnet50'), **bench.CFG))
    model = SWEM(cfg)
    model.load_state_dict(weights.fill_state_dict(model.state_dict(), seed=3, backbone='resnet50'))
    model = model.eval().cuda()
    book = ops.PlanBook(fallback=ops.MODEL_FALLBACK)
    if os.path.exists(ops.shipped_plans()):
        book.load_shipped()
    model.book = book
    frames, m0 = synth.make_clip(t=T, h=bench.H, w=bench.W, n_obj=N_OBJ, out_hw=bench.OUT_HW, seed=123)
    with torch.no_grad():
        torch.manual_seed(123)
        preds, _ = evaluator.evaluate_davis_seq(model, frames.cuda(), [m0.cuda()] + [None] * (T - 1), bench.OUT_HW)
    torch.cuda.synchronize()
    return torch.cat(preds, 0).to(torch.uint8).cpu().numpy()


def run_once(mode, preds, root):
    """One sequence through a writer -> figures of that run and the directory it wrote."""
    import torch
    from swem_amd import io
    d = os.path.join(root, mode)
    shutil.rmtree(d, ignore_errors=True)
    w = io.IndexMapWriter(d, encode=mode)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    c0, t0 = time.process_time(), time.perf_counter()
    a.record()
    w.submit('seq', preds)
    b.record()
    n = w.close()
    t1, c1 = time.perf_counter(), time.process_time()
    b.synchronize()
    assert n == len(preds)
    return {'device_ms': a.elapsed_time(b), 'cpu_s': c1 - c0, 'wall_s': t1 - t0}, os.path.join(d, 'seq')


def compare(content, maps_u8, repeats):
    import numpy as np
    import torch
    from PIL import Image
    from swem_amd import io, ops
    n = maps_u8.shape[0]
    preds = [torch.from_numpy(m[None].astype(np.int64)).cuda() for m in maps_u8]
    root = tempfile.mkdtemp(prefix='png_bench_')
    try:
        runs = {'host': [], 'device': []}
        for mode in ('host', 'device'):
            run_once(mode, preds, root)                                     # warm-up: code objects, pinned pools, threads
        for _ in range(repeats):
            for mode in ('host', 'device'):
                runs[mode].append(run_once(mode, preds, root)[0])
        sizes, equal = {}, 0
        for mode in ('host', 'device'):
            d = os.path.join(root, mode, 'seq')
            sizes[mode] = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        for t in range(n):
            name = '%05d.png' % (t + 1)
            hp, dp = Image.open(os.path.join(root, 'host', 'seq', name)), Image.open(os.path.join(root, 'device', 'seq', name))
            equal += int(dp.mode == hp.mode == 'P' and np.array_equal(np.asarray(dp), maps_u8[t]) and
                         np.array_equal(np.asarray(hp), maps_u8[t]) and dp.getpalette() == hp.getpalette())
    finally:
        shutil.rmtree(root, ignore_errors=True)

    def med(mode, key):
        v = sorted(r[key] for r in runs[mode])
        return v[len(v) // 2]
    rec = {'content': content, 'frames': n, 'repeats': repeats, 'files_decode_equal_to_the_maps_and_to_the_host_files': '%d / %d' % (equal, n)}
    for mode in ('host', 'device'):
        rec[mode] = {'device_us_per_frame': round(1e3 * med(mode, 'device_ms') / n, 2),
                     'host_cpu_ms_per_frame': round(1e3 * med(mode, 'cpu_s') / n, 3),
                     'wall_ms_to_files_on_disk': round(1e3 * med(mode, 'wall_s'), 1),
                     'wall_ms_all_runs': [round(1e3 * r['wall_s'], 1) for r in runs[mode]],
                     'bytes_device_to_host': int(n * H * W if mode == 'host' else sizes['device'] + 8 * (n + 1)),
                     'file_bytes_total': int(sizes[mode]), 'file_bytes_per_frame': int(sizes[mode] // n)}
    rec['device']['file_bytes_over_pil'] = round(sizes['device'] / sizes['host'], 3)
    rec['host_cpu_host_over_device'] = round(med('host', 'cpu_s') / max(med('device', 'cpu_s'), 1e-9), 2)
    rec['wall_host_over_device'] = round(med('host', 'wall_s') / max(med('device', 'wall_s'), 1e-9), 2)
    # the encoder alone
    pal = np.asarray(io.default_palette(), np.uint8)
    dev_maps = torch.from_numpy(maps_u8).cuda()
    reps, t = timed_regions(lambda: ops.png_encode_u8(dev_maps, pal))
    m = t[len(t) // 2]
    rec['png_encode_u8'] = {'repeats_per_region': reps, 'ms_per_sequence_median': round(m, 4),
                            'spread_pct': round(100 * (t[-1] - t[0]) / m, 2), 'us_per_frame': round(1e3 * m / n, 3)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_device.json'))
    ap.add_argument('--no-model', action='store_true', help='skip the bench.py child (no model frame time in the record)')
    ap.add_argument('--synthetic', action='store_true', help='synthetic discs only: do not run the bench model for its predictions')
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    model = None if args.no_model else model_frame_ms()

    import torch
    from swem_amd import _lib, dist as sdist
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit('png_bench.py measures on the GPU: no device found')
    cpus = sdist.respect_cpu_quota()
    prop = torch.cuda.get_device_properties(0)
    rec = {'workload': '%d predicted index maps %dx%d, %d objects, int64 on the device, default palette; IndexMapWriter(workers=4)'
                       % (T - 1, H, W, N_OBJ),
           'box': '%s (%s, %d CUs); CPU threads within the quota: %s' % (prop.name, getattr(prop, 'gcnArchName', '?'),
                                                                        prop.multi_processor_count, cpus),
           'timing': 'host / device alternated in one process after one warm-up run each; medians; device time from events around '
                     'submit on the submitting stream; CPU from time.process_time (all threads) across submit .. close',
           'model': model, 'contents': []}
    contents = [('synthetic discs with ragged edges', synthetic_blobs())]
    if not args.synthetic:
        contents.insert(0, ("the bench model's own predictions (random weights)", model_predictions()))
    for name, maps in contents:
        row = compare(name, maps, args.repeats)
        if model is not None:
            for mode in ('host', 'device'):
                row[mode]['host_cpu_over_model_frame_time'] = round(row[mode]['host_cpu_ms_per_frame'] / model['ms_per_frame'], 3)
            row['png_encode_u8']['share_of_model_frame_time_pct'] = round(
                100 * row['png_encode_u8']['us_per_frame'] / 1e3 / model['ms_per_frame'], 3)
        rec['contents'].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
