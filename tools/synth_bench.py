"""Speed of the stage-0 path on the device (swem_amd.augment.StaticClipSynthesizer; csrc/synth.hip and the static form of
csrc/augment.hip) beside the training step it feeds and its one-core CPU restatement.  One command, writes
profiles/synth_device.json:

    python tools/synth_bench.py [--out profiles/synth_device.json] [--no-train] [--no-cpu]

  * the workload: B = 4 clips of N = 2 decoded uint8 images + masks in 480x640 slots resident on the device -> T = 3 frames of
    384x384, drawn parameters (`draw_static_params`); warm-up, then seven timed regions of >= 0.3 s each between device events,
    eager calls (parameters already in the static buffers: seven launches per call) and replays of the call captured
    into a graph; median and spread, per clip;
  * the two stages apart (compositing: four launches; static chain: three), same timing;
  * beside it: the per-clip time of the AMP training step, from `python tools/train_bench.py --amp` started as a child process
    BEFORE this process opens the GPU;
  * the bytes a clip moves (inputs read by the statistics pass and again by the composite, composites written and read back, outputs
    written once, plus the pre-colour planes and the uint8 workspace) over the time: a whole-call rate;
  * for context only, on ONE CPU core: the float64 numpy restatement (tests/synth_ref.py) of one clip.
No bar was fixed in advance; above 5 % of the AMP step per clip the stage times say where the time goes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
HBM_ACHIEVABLE = 6.3e12      # bytes/s, README
B, N, T, SLOT_HW, OUT_HW = 4, 2, 3, (480, 640), (384, 384)
SIZES = [[(480, 640), (375, 500)], [(333, 500), (480, 640)], [(480, 640), (480, 640)], [(400, 600), (480, 360)]]


def cpu_restatement_s(imgs, masks, clips):
    """tests/synth_ref.py in float64 on one thread: compositing and the static chain of clip 0."""
    import numpy as np
    import torch
    from tests import synth_ref as S
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    c = S.composite(*S.unslot(imgs, masks, 0, clips[0]['sizes']), clips[0])
    t1 = time.perf_counter()
    S.static_chain(c['frames'], c['labels'], clips[0], N, np.float64)
    t2 = time.perf_counter()
    return {'what': 'the float64 numpy restatement of one clip (tests/synth_ref.py), one core; without decoding',
            'composite_s': round(t1 - t0, 3), 'static_chain_s': round(t2 - t1, 3), 's_per_clip': round(t2 - t0, 3),
            'frames_per_s_one_core': round(T / (t2 - t0), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'synth_device.json'))
    ap.add_argument('--no-train', action='store_true', help='skip the train_bench.py child (no share of the step is recorded)')
    ap.add_argument('--no-cpu', action='store_true', help='skip the one-core restatement')
    args = ap.parse_args()
    import augment_bench as AB
    AB.B = B
    train = None if args.no_train else AB.train_step_ms()

    import numpy as np
    import torch
    from swem_amd import _lib, augment as A, ops
    from tests import synth_ref as S
    _lib.load()
    imgs, masks = S.make_slots(31, SIZES, N, slot_hw=SLOT_HW, cell=24, values=(0, 1))
    rng = np.random.default_rng(32)
    clips = [A.draw_static_params(rng, T, s, OUT_HW) for s in SIZES]
    cpu = None if args.no_cpu else cpu_restatement_s(imgs, masks, clips)
    if not torch.cuda.is_available():
        raise SystemExit('synth_bench.py measures on the GPU: no device found')
    i, m = torch.from_numpy(imgs).cuda(), torch.from_numpy(masks).cuda()
    syn = A.StaticClipSynthesizer(OUT_HW, N, T, SLOT_HW)
    out = syn.empty_out(B)
    syn(i, m, clips, out=out)
    torch.cuda.synchronize()
    comp, comp_lab = syn.composites(B)
    first = [t.clone() for t in out] + [comp.clone(), comp_lab.clone()]
    ws, dev = syn._buffers(B).ws, syn._buffers(B).params.dev
    sws, sdev = syn._synth_buffers(B).ws, syn._synth_buffers(B).params.dev

    def eager():
        syn(i, m, None, out=out)

    def stage_synth():
        ops.synth_frames(i, m, sdev, comp, comp_lab, sws)

    def stage_chain():
        ops.augment_static(comp, comp_lab, dev, out[0], out[1], out[2], out[3], out[4], ws)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eager()
    Ho, Wo = OUT_HW
    px = T * Ho * Wo
    slot = SLOT_HW[0] * SLOT_HW[1]
    real = [sum(h * w for h, w in s) for s in SIZES]
    img0 = [s[0][0] * s[0][1] for s in SIZES]
    inputs = float(np.mean(real)) * 4                              # image + mask bytes of a clip's real sizes
    comps = float(np.mean(img0)) * 4 * T
    outputs = px * (3 * 4 + (N + 1) * 4 + 8) + (N + 1) * 4 + 4
    algorithmic = inputs + outputs
    moved = 2 * inputs + 2 * comps + outputs + px * (2 * 3 * 4 + 2 * 2)
    rec = {'workload': 'B = %d clips of N = %d decoded uint8 images + masks in %dx%d slots on the device (sizes %s) -> T = %d frames '
                       'of %dx%d, drawn parameters' % (B, N, SLOT_HW[0], SLOT_HW[1], SIZES, T, Ho, Wo),
           'timing': 'device events around repeated calls; 7 regions of >= 0.3 s; us per clip = per call / %d' % B,
           'train_step_amp': train, 'cpu_restatement': cpu,
           'bytes_per_clip': {'algorithmic': int(algorithmic), 'moved_with_intermediates': int(moved), 'slot_bytes': slot * 4 * N,
                              'workspace_bytes_per_call': int(_lib.query('swem_augment_workspace', B, T, Ho, Wo)) +
                              int(_lib.query('swem_synth_workspace', B, T, N))}}
    for name, fn in (('eager', eager), ('graph_replay', graph.replay), ('stage_compositing', stage_synth),
                     ('stage_static_chain', stage_chain)):
        reps, ms = AB.timed_regions(fn)
        med = ms[len(ms) // 2]
        row = {'repeats_per_region': reps, 'ms_per_call_regions': [round(v, 4) for v in ms], 'ms_per_call_median': round(med, 4),
               'spread_pct': round(100 * (ms[-1] - ms[0]) / med, 2), 'us_per_clip': round(1e3 * med / B, 2),
               'us_per_frame': round(1e3 * med / (B * T), 2)}
        if not name.startswith('stage'):
            row['moved_GB_per_s'] = round(moved * B / (med * 1e-3) / 1e9, 1)
            row['moved_share_of_6.3TBps_pct'] = round(100 * moved * B / (med * 1e-3) / HBM_ACHIEVABLE, 2)
            row['device_frames_per_s'] = round(B * T / (med * 1e-3), 0)
        if train is not None:
            row['share_of_amp_step_per_clip_pct'] = round(100 * (med / B) / train['ms_per_clip'], 3)
        # thousands of calls issued back to back: what the last one left equals what the first, synchronised call gave
        torch.cuda.synchronize()
        row['outputs_equal_first_call'] = all(torch.equal(a, b) for a, b in zip(list(out) + [comp, comp_lab], first))
        rec[name] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
