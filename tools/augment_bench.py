"""Speed of the device augmentation (swem_amd.augment.ClipAugmenter, csrc/augment.hip) beside the training step it feeds and the
CPU chain it replaces.  One command, writes profiles/augment_device.json:

    python tools/augment_bench.py [--out profiles/augment_device.json] [--no-train] [--no-cpu]

  * the workload: B = 4 clips of three decoded 480x854 uint8 frames + label maps resident on the device -> 3 x 384x384, N = 2, drawn
    parameters (`draw_params`); warm-up, then seven timed regions of >= 0.3 s each between device events, eager calls (parameters
    already in the static buffer: memset + two launches per call) and replays of the call captured into a graph; median and
    spread, per clip;
  * beside it: the per-clip time of the AMP training step, from `python tools/train_bench.py --amp` started as a child process
    BEFORE this process opens the GPU;
  * the bytes a clip moves (sources read once, outputs written once, plus the pre-colour planes and the uint8 workspace written by
    the first kernel and read back by the second) over the time: a whole-call rate, to show how far from a copy it is;
  * for context only, on ONE CPU core: a PIL / torch restatement of the reference's per-frame chain with its three resamples
    (bicubic resized crop, colour jitter, bicubic affine with fill, colour jitter, thin-plate-spline grid_sample), in frames/s.
The record's condition: device time per clip <= 5 % of the AMP step's per-clip time of the same call."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.3e12      # bytes/s, README
B, T, SRC_HW, OUT_HW, NOBJ = 4, 3, (480, 854), (384, 384), 2


def train_step_ms(steps=20, warmup=2):
    """`python tools/train_bench.py --amp` in a fresh child process: ms per clip of the AMP training step."""
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'train_bench.py'), '--amp', '--clips', str(B), '--steps', str(steps),
           '--warmup', str(warmup), '--no-roofline']
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    if res.returncode != 0:
        raise RuntimeError('train_bench.py failed (%d): %s' % (res.returncode, res.stderr[-2000:]))
    rec = [json.loads(ln) for ln in res.stdout.splitlines() if ln.startswith('{')][-1]
    return {'command': 'python tools/train_bench.py --amp --clips %d --steps %d --warmup %d --no-roofline' % (B, steps, warmup),
            'clips_per_s': rec['value'], 'ms_per_step': rec['ms_per_step'], 'clips_per_step': rec['clips_per_step'],
            'ms_per_clip': rec['ms_per_step'] / rec['clips_per_step']}


def timed_regions(fn, regions=7, min_s=0.3):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = max(3, int(min_s / max((time.perf_counter() - t0) / 3, 1e-6)) + 1)
    out = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return reps, sorted(out)


def cpu_chain_frames_per_s(frames=6, seed=0):
    """The reference's per-frame work (video_dataset.py:269-299) restated with PIL and torch on one core: three resamples with
    8-bit rounding between them.  Context for the device time, not a parity yardstick."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from PIL import Image, ImageEnhance
    from swem_amd import augment as A
    torch.set_num_threads(1)
    rng = np.random.default_rng(seed)
    Ho, Wo = OUT_HW
    low = rng.integers(0, 256, size=(SRC_HW[0] // 8 + 1, SRC_HW[1] // 8 + 1, 3), dtype=np.uint8)
    im0 = Image.fromarray(low).resize((SRC_HW[1], SRC_HW[0]), Image.BICUBIC)
    gt0 = Image.fromarray((rng.integers(0, 3, size=(SRC_HW[0] // 24, SRC_HW[1] // 24)) * 3).astype(np.uint8)).resize(
        (SRC_HW[1], SRC_HW[0]), Image.NEAREST)
    enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
    yy, xx = torch.linspace(-1, 1, Ho, dtype=torch.float32), torch.linspace(-1, 1, Wo, dtype=torch.float32)
    t0 = time.perf_counter()
    for _ in range(frames):
        p = A.draw_params(rng, 1, SRC_HW, OUT_HW)
        fr = p['frames'][0]
        top, left, ch, cw = p['crop']
        im, gt = im0, gt0
        if p['flip']:
            im, gt = im.transpose(Image.FLIP_LEFT_RIGHT), gt.transpose(Image.FLIP_LEFT_RIGHT)
        im = im.resize((Wo, Ho), Image.BICUBIC, box=(left, top, left + cw, top + ch))
        gt = gt.resize((Wo, Ho), Image.NEAREST, box=(left, top, left + cw, top + ch))
        for op in p['order']:
            im = enh[op](im).enhance(p['factors'][op])
        coeffs = tuple(A.inverse_affine(fr['angle'], fr['shear'], OUT_HW).reshape(-1))
        im = im.transform((Wo, Ho), Image.AFFINE, coeffs, resample=Image.BICUBIC, fillcolor=A.IM_MEAN)
        gt = gt.transform((Wo, Ho), Image.AFFINE, coeffs, resample=Image.NEAREST, fillcolor=0)
        for op in fr['order']:
            im = enh[op](im).enhance(fr['factors'][op])
        x = torch.from_numpy(np.array(im)).permute(2, 0, 1).float().div_(255)[None]
        g = torch.from_numpy(np.array(gt)).float()[None, None]
        Aff, W = A.tps_coefficients(fr['tps_Y'])
        pts = torch.stack([xx[None, :].expand(Ho, Wo), yy[:, None].expand(Ho, Wo)], -1).reshape(-1, 2)
        X = torch.from_numpy(A.TPS_ANCHORS).float()
        d2 = ((pts[:, None, :] - X[None, :, :]) ** 2).sum(-1)
        grid = (torch.from_numpy(Aff[0]).float() + pts @ torch.from_numpy(Aff[1:]).float() +
                (d2 * torch.log(d2 + 1e-9)) @ torch.from_numpy(W).float()).view(1, Ho, Wo, 2)
        x = F.grid_sample(x, grid, mode='bilinear', align_corners=False)
        g = F.grid_sample(g, grid, mode='nearest', align_corners=False)
    dt = time.perf_counter() - t0
    return {'frames': frames, 'frames_per_s_one_core': round(frames / dt, 2), 'ms_per_frame': round(1e3 * dt / frames, 2),
            'what': 'PIL bicubic resized crop + ColorJitter + PIL bicubic affine (fill) + ColorJitter + TPS grid_sample on 480x854 '
                    '-> 384x384, image and label, one torch thread; without JPEG decoding and label picking'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment_device.json'))
    ap.add_argument('--no-train', action='store_true', help='skip the train_bench.py child (no share of the step is recorded)')
    ap.add_argument('--no-cpu', action='store_true', help='skip the one-core PIL chain')
    args = ap.parse_args()

    train = None if args.no_train else train_step_ms()
    cpu = None if args.no_cpu else cpu_chain_frames_per_s()

    import numpy as np
    import torch
    from swem_amd import _lib, augment as A
    from tests import augment_ref as R
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit('augment_bench.py measures on the GPU: no device found')
    src, lab = R.make_inputs(21, B, T, SRC_HW, cell=24)
    rng = np.random.default_rng(22)
    clips = [A.draw_params(rng, T, SRC_HW, OUT_HW) for _ in range(B)]
    s, l = torch.from_numpy(src).cuda(), torch.from_numpy(lab).cuda()
    aug = A.ClipAugmenter(OUT_HW, NOBJ, T)
    out = aug.empty_out(B)
    aug(s, l, clips, out=out)
    torch.cuda.synchronize()

    def eager():
        aug(s, l, None, out=out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eager()
    Ho, Wo = OUT_HW
    px = T * Ho * Wo
    algorithmic = T * SRC_HW[0] * SRC_HW[1] * 4 + px * (3 * 4 + (NOBJ + 1) * 4 + 8) + (NOBJ + 1) * 4 + 4
    moved = algorithmic + px * (2 * 3 * 4 + 2 * 2)
    rec = {'workload': 'B = %d clips of T = %d decoded %dx%d uint8 frames + label maps on the device -> %dx%d, N = %d, drawn '
                       'parameters' % (B, T, SRC_HW[0], SRC_HW[1], Ho, Wo, NOBJ),
           'timing': 'device events around repeated calls; 7 regions of >= 0.3 s; us per clip = per call / %d' % B,
           'train_step_amp': train, 'cpu_chain': cpu,
           'bytes_per_clip': {'algorithmic': algorithmic, 'moved_with_intermediates': moved,
                              'workspace_bytes_per_call': int(_lib.query('swem_augment_workspace', B, T, Ho, Wo))}}
    for name, fn in (('eager', eager), ('graph_replay', graph.replay)):
        reps, ms = timed_regions(fn)
        med = ms[len(ms) // 2]
        row = {'repeats_per_region': reps, 'ms_per_call_regions': [round(v, 4) for v in ms], 'ms_per_call_median': round(med, 4),
               'spread_pct': round(100 * (ms[-1] - ms[0]) / med, 2), 'us_per_clip': round(1e3 * med / B, 2),
               'us_per_frame': round(1e3 * med / (B * T), 2),
               'moved_GB_per_s': round(moved * B / (med * 1e-3) / 1e9, 1),
               'moved_share_of_6.3TBps_pct': round(100 * moved * B / (med * 1e-3) / HBM_ACHIEVABLE, 2)}
        if train is not None:
            row['share_of_amp_step_per_clip_pct'] = round(100 * (med / B) / train['ms_per_clip'], 3)
        if cpu is not None:
            row['device_frames_per_s'] = round(B * T / (med * 1e-3), 0)
        rec[name] = row
    if train is not None:
        share = rec['graph_replay']['share_of_amp_step_per_clip_pct']
        rec['condition'] = {'text': 'device time per clip (graph replay) <= 5 % of the AMP training step per clip of the same call',
                            'share_pct': share, 'met': bool(share <= 5.0),
                            'eager_share_pct': rec['eager']['share_of_amp_step_per_clip_pct']}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
