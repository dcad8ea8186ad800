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
No speed or size bar was fixed in advance; the record states what was measured.

    python tools/png_bench.py --dynamic [--out profiles/png_dynamic.json] [--no-model] [--synthetic]

writes a second record instead: the same two contents through host / device fixed / device dynamic (`codes='dynamic'`), file
sizes against PIL's, the encoder alone through the first entry point and through the second in both modes; and the overlay
pictures of VAL.VISUALIZE on the frames of the bench clip, `overlay_encode='device'` against `'host'`: wall, host CPU, bytes
copied, file sizes."""
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


def run_leg(kw, preds, root, frames_u8=None):
    """`run_once` for any set of writer switches, with the overlay pictures of `frames_u8` where given."""
    import torch
    from swem_amd import io
    shutil.rmtree(root, ignore_errors=True)
    w = io.IndexMapWriter(root, **kw)
    torch.cuda.synchronize()
    c0, t0 = time.process_time(), time.perf_counter()
    w.submit('seq', preds, overlay_frames_u8=frames_u8)
    n = w.close()
    t1, c1 = time.perf_counter(), time.process_time()
    assert n == len(preds)
    return {'cpu_s': c1 - c0, 'wall_s': t1 - t0}


def dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def median(values):
    v = sorted(values)
    return v[len(v) // 2]


def bench_frames_u8():
    """The decoded frames of the bench clip at the maps' size: synth.make_clip's pictures as uint8 RGB (T,H,W,3)."""
    from swem_amd import synth
    frames, _ = synth.make_clip(t=T, h=H, w=W, n_obj=N_OBJ, seed=123)
    return (frames[0] * 255.0).round().clamp(0, 255).byte().permute(0, 2, 3, 1).contiguous().numpy()


def compare_dynamic(content, maps_u8, repeats, model):
    """Index maps: host / device fixed / device dynamic, alternated in one process; the encoder alone in its three forms."""
    import numpy as np
    import torch
    from PIL import Image
    from swem_amd import io, ops
    n = maps_u8.shape[0]
    preds = [torch.from_numpy(m[None].astype(np.int64)).cuda() for m in maps_u8]
    legs = {'host': dict(encode='host'), 'device_fixed': dict(encode='device'), 'device_dynamic': dict(encode='device', codes='dynamic')}
    root = tempfile.mkdtemp(prefix='png_bench_')
    try:
        runs = {k: [] for k in legs}
        for k, kw in legs.items():
            run_leg(kw, preds, os.path.join(root, k))
        for _ in range(repeats):
            for k, kw in legs.items():
                runs[k].append(run_leg(kw, preds, os.path.join(root, k)))
        sizes = {k: dir_bytes(os.path.join(root, k, 'seq')) for k in legs}
        equal = 0
        for t in range(n):
            dp = Image.open(os.path.join(root, 'device_dynamic', 'seq', '%05d.png' % (t + 1)))
            equal += int(dp.mode == 'P' and np.array_equal(np.asarray(dp), maps_u8[t]))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    rec = {'content': content, 'frames': n, 'repeats': repeats, 'dynamic_files_decode_equal_to_the_maps': '%d / %d' % (equal, n)}
    for k in legs:
        rec[k] = {'host_cpu_ms_per_frame': round(1e3 * median(r['cpu_s'] for r in runs[k]) / n, 3),
                  'wall_ms_to_files_on_disk': round(1e3 * median(r['wall_s'] for r in runs[k]), 1),
                  'file_bytes_total': int(sizes[k]), 'file_bytes_per_frame': int(sizes[k] // n),
                  'file_bytes_over_pil': round(sizes[k] / sizes['host'], 3)}
    rec['dynamic_over_fixed_file_bytes'] = round(sizes['device_dynamic'] / sizes['device_fixed'], 3)
    pal = np.asarray(io.default_palette(), np.uint8)
    dev_maps = torch.from_numpy(maps_u8).cuda()

    def px(codes):
        """swem_png_encode_px_u8 itself: ops.png_encode_u8 sends its default call to the first entry point"""
        from swem_amd import _lib
        nbytes = _lib.query('swem_png_workspace_px', n, H, W, 1)
        ws = ops.workspace(nbytes, dev_maps.device)
        _lib.call('swem_png_encode_px_u8', ops._stream(), dev_maps.data_ptr(), 1, pal.tobytes(), ops.PNG_CODES[codes], blob.data_ptr(),
                  blob.numel(), offsets.data_ptr(), n, H, W, ws.data_ptr(), nbytes)
    blob = torch.empty(n * io.png_capacity(H, W), dtype=torch.uint8, device='cuda')
    offsets = torch.empty(n + 1, dtype=torch.int64, device='cuda')
    forms = {'first_entry_point_fixed': lambda: ops.png_encode_u8(dev_maps, pal, blob=blob),
             'second_entry_point_fixed': lambda: px('fixed'), 'second_entry_point_dynamic': lambda: px('dynamic')}
    times = {k: [] for k in forms}
    for _ in range(3):                                  # the three forms alternated, the median of the regions' medians
        for k, fn in forms.items():
            reps, t = timed_regions(fn, regions=5, min_s=0.15)
            times[k].append(t[len(t) // 2])
    rec['encoder_alone'] = {}
    for k in forms:
        m = median(times[k])
        rec['encoder_alone'][k] = {'us_per_frame': round(1e3 * m / n, 3), 'ms_per_sequence_all': [round(v, 4) for v in times[k]]}
        if model is not None:
            rec['encoder_alone'][k]['share_of_model_frame_time_pct'] = round(100 * m / n / model['ms_per_frame'], 3)
    e = rec['encoder_alone']
    e['dynamic_minus_fixed_us_per_frame'] = round(e['second_entry_point_dynamic']['us_per_frame'] -
                                                  e['second_entry_point_fixed']['us_per_frame'], 3)
    e['note'] = ('dynamic minus fixed = the histogram pass, ranking, the serial table build and header on lane 0, and the fixed count '
                 'riding along: an upper bound of the table build; the fixed form is the two token passes (count, write) plus '
                 'gather, stores and checksums')
    return rec


def compare_overlays(maps_u8, frames_u8, repeats, model):
    """VAL.VISUALIZE: submit .. close with overlay_encode='device' against 'host', the index maps device-encoded in both."""
    import numpy as np
    import torch
    from PIL import Image
    n = maps_u8.shape[0]
    preds = [torch.from_numpy(m[None].astype(np.int64)).cuda() for m in maps_u8]
    frames = torch.from_numpy(frames_u8).cuda()
    legs = {'overlay_host': dict(encode='device', codes='dynamic', overlay_encode='host'),
            'overlay_device': dict(encode='device', codes='dynamic', overlay_encode='device')}
    root = tempfile.mkdtemp(prefix='png_bench_')
    try:
        runs = {k: [] for k in legs}
        for k, kw in legs.items():
            run_leg(kw, preds, os.path.join(root, k), frames)
        for _ in range(repeats):
            for k, kw in legs.items():
                runs[k].append(run_leg(kw, preds, os.path.join(root, k), frames))
        sizes = {k: dir_bytes(os.path.join(root, k, 'overlay', 'seq')) for k in legs}
        maps_bytes = dir_bytes(os.path.join(root, 'overlay_device', 'seq'))
        equal = 0
        for t in range(n):
            name = '%05d.png' % (t + 1)
            hp, dp = (Image.open(os.path.join(root, k, 'overlay', 'seq', name)) for k in ('overlay_host', 'overlay_device'))
            equal += int(dp.mode == hp.mode == 'RGB' and np.array_equal(np.asarray(dp), np.asarray(hp)))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    rec = {'content': 'overlay pictures of the synthetic discs on the frames of the bench clip (synth.make_clip, uint8 RGB %dx%d)' % (H, W),
           'frames': n, 'repeats': repeats, 'device_files_decode_equal_to_the_host_files': '%d / %d' % (equal, n)}
    for k in legs:
        rec[k] = {'host_cpu_ms_per_frame': round(1e3 * median(r['cpu_s'] for r in runs[k]) / n, 3),
                  'wall_ms_to_files_on_disk': round(1e3 * median(r['wall_s'] for r in runs[k]), 1),
                  'wall_ms_all_runs': [round(1e3 * r['wall_s'], 1) for r in runs[k]],
                  'overlay_bytes_device_to_host': int(n * H * W * 3 if k == 'overlay_host' else sizes[k] + 8 * (n + 1)),
                  'overlay_file_bytes_total': int(sizes[k]), 'overlay_file_bytes_per_frame': int(sizes[k] // n)}
        if model is not None:
            rec[k]['host_cpu_over_model_frame_time'] = round(rec[k]['host_cpu_ms_per_frame'] / model['ms_per_frame'], 3)
    rec['index_map_file_bytes_total_either_leg'] = int(maps_bytes)
    rec['overlay_file_bytes_device_over_pil'] = round(sizes['overlay_device'] / sizes['overlay_host'], 3)
    rec['wall_host_over_device'] = round(rec['overlay_host']['wall_ms_to_files_on_disk'] / max(rec['overlay_device']['wall_ms_to_files_on_disk'], 1e-9), 2)
    rec['host_cpu_host_over_device'] = round(rec['overlay_host']['host_cpu_ms_per_frame'] / max(rec['overlay_device']['host_cpu_ms_per_frame'], 1e-9), 2)
    from swem_amd import ops
    reps, t = timed_regions(lambda: ops.png_encode_u8(frames[1:], None, codes='dynamic'), regions=5, min_s=0.2)
    rec['png_encode_u8_truecolour_dynamic'] = {'us_per_frame': round(1e3 * t[len(t) // 2] / n, 2), 'frames': n, 'repeats_per_region': reps}
    return rec


def blobs_against_zlib():
    """The figure tests/test_gpu_png_dyn.py::test_size_against_zlib holds the encoder to (tests/png_dyn_cases.py): the IDAT
    bytes of the dynamic file of the tests' 480x854 `blobs` map over zlib level 6 on the same scanlines."""
    import zlib
    import numpy as np
    import torch
    from swem_amd import io, ops
    from tests.test_gpu_png import make_map
    m = make_map('blobs', H, W, seed=0)
    blob, offsets = ops.png_encode_u8(torch.from_numpy(m[None]).cuda(), np.asarray(io.default_palette(), np.uint8), codes='dynamic')
    data = blob[:int(offsets[-1])].cpu().numpy().tobytes()
    idat, pos = 0, 8
    while pos < len(data):                              # chunks: length, type, payload, CRC
        n = int.from_bytes(data[pos:pos + 4], 'big')
        idat += n if data[pos + 4:pos + 8] == b'IDAT' else 0
        pos += 12 + n
    z = len(zlib.compress(b''.join(b'\0' + m[y].tobytes() for y in range(H)), 6))
    return {'map': "tests.test_gpu_png.make_map('blobs', 480, 854, seed=0)", 'idat_bytes_dynamic': idat, 'zlib_level_6_bytes': z,
            'ratio': round(idat / z, 4)}


def main_dynamic(args):
    """--dynamic: the record profiles/png_dynamic.json -- index maps under dynamic tables, and the overlay pictures."""
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
           'timing': 'the legs alternated in one process after one warm-up run each; medians of %d; CPU from time.process_time (all '
                     'threads) and wall from time.perf_counter across submit .. close; the encoder alone from device events' % args.repeats,
           'model': model, 'contents': []}
    discs = synthetic_blobs()
    contents = [('synthetic discs with ragged edges', discs)]
    if not args.synthetic:
        contents.insert(0, ("the bench model's own predictions (random weights)", model_predictions()))
    for name, maps in contents:
        rec['contents'].append(compare_dynamic(name, maps, args.repeats, model))
    rec['overlays'] = compare_overlays(discs, bench_frames_u8(), args.repeats, model)
    rec['blobs_map_against_zlib'] = blobs_against_zlib()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dynamic', action='store_true',
                    help='the dynamic-table and overlay legs instead: writes profiles/png_dynamic.json (or --out)')
    ap.add_argument('--out', default=None, help='default: profiles/png_device.json, with --dynamic profiles/png_dynamic.json')
    ap.add_argument('--no-model', action='store_true', help='skip the bench.py child (no model frame time in the record)')
    ap.add_argument('--synthetic', action='store_true', help='synthetic discs only: do not run the bench model for its predictions')
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'png_dynamic.json' if args.dynamic else 'png_device.json')
    if args.dynamic:
        return main_dynamic(args)
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
