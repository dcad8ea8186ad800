"""Speed of J&F scoring on the device (swem_amd.metrics.jf_counts_device, csrc/metrics.hip) beside what it replaces and what
it must not slow down.  One command, writes profiles/jf_device.json:

    python tools/jf_bench.py [--out profiles/jf_device.json]

  * the workload a user runs: a T = 70 frame 480x854 sequence, N = 2 (and N = 5) objects, uint8 index maps resident on the
    device (the seeded generator of tests/test_gpu_metrics.py); warm-up, then seven timed regions of enough repeats to last
    >= 0.3 s each, device events around `jf_counts_device` + the copy of the counts to the host; median and spread;
  * in the same call: the CPU `evaluate_semisupervised` on 8 of those frames (ms per frame and object), and the model's frame
    time from `python bench.py` started as a child process BEFORE this process opens the GPU (ms_per_step / frames_per_step);
  * algorithmic bytes (every map read once + the counts written) over the time: a WHOLE-CALL rate (memset, two kernels, the
    copy and the host's wait), not a kernel's; per-kernel times come from a profiler run of their own:
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/jf_bench.py --profile-only
    (profiles/jf_device_kernel_stats.csv).
The record's condition: device scoring time per frame (all N = 2 objects) <= 10 % of the model's frame time of the same call."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.3e12      # bytes/s, README


def model_frame_ms(steps=100, warmup=5):
    """`python bench.py` in a fresh child process; ms per frame of the headline workload = ms_per_step / frames per step."""
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if res.returncode != 0:
        raise RuntimeError('bench.py failed (%d): %s' % (res.returncode, res.stderr[-2000:]))
    rec = [json.loads(ln) for ln in res.stdout.splitlines() if ln.startswith('{')][-1]
    fps_step = int(rec['config']['frames_per_step'])
    return {'command': 'python bench.py --gpus 1 --steps %d --warmup %d' % (steps, warmup), 'ms_per_step': rec['ms_per_step'],
            'frames_per_step': fps_step, 'ms_per_frame': rec['ms_per_step'] / fps_step, 'frames_per_s': rec['value']}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jf_device.json'))
    ap.add_argument('--profile-only', action='store_true', help='a few calls of the N = 2 workload and nothing else (for rocprofv3)')
    args = ap.parse_args()

    model = None if args.profile_only else model_frame_ms()

    import torch
    from swem_amd import _lib, metrics as M
    from tests.test_gpu_metrics import make_maps
    _lib.load()          # (built by `python -m swem_amd.build` / the bench.py child above; never a fallback)
    if not torch.cuda.is_available():
        raise SystemExit('jf_bench.py measures on the GPU: no device found')
    T, H, W = 70, 480, 854
    rec = {'workload': 'T = %d frames %dx%d, uint8 index maps resident on the device, disk radius %d' % (T, H, W, M.bound_pixels((H, W))),
           'timing': 'device events around jf_counts_device + counts.cpu(); 7 regions of >= 0.3 s; ms per call = per sequence',
           'model': model, 'objects': {}}
    for N in ((2,) if args.profile_only else (2, 5)):
        gt, pred = make_maps(T, H, W, N, seed=11)
        g, p = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()

        def call():
            return M.jf_counts_device(g, p, N).cpu()
        if args.profile_only:
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            return
        reps, ms = timed_regions(call)
        med = ms[len(ms) // 2]
        nbytes = 2 * T * H * W + T * N * 6 * 4
        row = {'repeats_per_region': reps, 'ms_per_sequence_regions': [round(v, 4) for v in ms], 'ms_per_sequence_median': round(med, 4),
               'spread_pct': round(100 * (ms[-1] - ms[0]) / med, 2), 'us_per_frame_all_objects': round(1e3 * med / T, 3),
               'algorithmic_bytes': nbytes, 'whole_call_GB_per_s': round(nbytes / (med * 1e-3) / 1e9, 2),
               'whole_call_share_of_6.3TBps_pct': round(100 * nbytes / (med * 1e-3) / HBM_ACHIEVABLE, 3),
               'workspace_bytes': int(_lib.query('swem_jf_workspace', T, N, H, W))}
        # the CPU metric on 8 of the frames (the protocol drops the first and the last: 6 scored), on this box
        t0 = time.perf_counter()
        cpu = M.evaluate_semisupervised(gt[:8], pred[:8], N)
        cpu_s = time.perf_counter() - t0
        dev = M.evaluate_semisupervised_device(g[:8], p[:8], N)
        row['cpu_ms_per_frame_and_object'] = round(1e3 * cpu_s / (6 * N), 2)
        row['device_equals_cpu_on_those_frames'] = bool(dev['J&F-Mean'] == cpu['J&F-Mean'] and all(
            tuple(a) == tuple(b) for k in 'JF' for a, b in zip(dev[k], cpu[k])))
        row['speedup_vs_cpu_per_frame_and_object'] = round(row['cpu_ms_per_frame_and_object'] / (med / (T * N)), 1)
        row['share_of_model_frame_time_pct'] = round(100 * (med / T) / model['ms_per_frame'], 3)
        rec['objects']['N=%d' % N] = row
    share = rec['objects']['N=2']['share_of_model_frame_time_pct']
    rec['condition'] = {'text': 'device scoring time per frame (N = 2) <= 10 % of the model frame time of the same call',
                        'share_pct': share, 'met': bool(share <= 10.0), 'aim_below_2_pct_met': bool(share < 2.0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
