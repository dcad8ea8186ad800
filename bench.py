#!/usr/bin/env python
"""bench.py -- SWEM 480p multi-object inference throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run measures the headline alone: set-up, warm-up, the K timed steps, --dump-outputs, the JSON line.  --full adds
everything else the line can carry (the objects listed below), each a run of its own after the timed steps.

Workload (BASELINE.json configs[1]): synthetic structured 480x864 clip, ResNet-50 key encoder, ResNet-18 value
encoder, K=256 bases, 5 EM iterations, 2 objects, output 480x854, random weights of the reference architecture.
A "step" is one steady-state frame of the reference's per-sequence loop (swem_evaluator.py:72-97):
encode_key -> match -> segment -> argmax/one-hot -> bilinear -> encode_value -> memorize, for each of the --seqs
independent sequences a GPU works on concurrently.  Default since round 6: 8 sequences as two LOCK-STEP lanes of four
(--lockstep 4, evaluator.LockstepGraph: a lane encodes the keys of 4 x 10 frames in one pass, runs match and memorize per sequence
and the decoder and value encoder once for the objects of its four sequences; the second lane's kernels fill what the first leaves
idle).  --lockstep 0: every sequence its own pipeline, one HIP stream + one HIP graph each (round 5's default with --seqs 4);
--seqs 1 = strictly one at a time.  Frames are resident in
HBM before the timed region (the reference also excludes the H2D copy, basic_evaluator.py:157-176).
Every rank runs its own clip (sequences are independent: weak scaling, no data-path collective);
value = frames of all ranks / max-over-ranks time.

Arithmetic of the line (`dtype`, `plans`): the shipped plans run the convolutions in f16x3 -- operands as fp16 hi + mid pairs
(22-23 significant bits), three MFMA products, fp32 accumulation: the error of the exact fp32 kernels.

Extra objects in the JSON line (--full; the --no-* options below leave some of them out):
  roofline     -- dominant conv kernel of the timed leg: useful conv FLOPs / summed launch durations (HIP events on the launch
                  stream) against ITS pipe's ceiling (dense f16 / bf16 MFMA peak / products per fp32 product); mfma_busy and
                  traffic from the committed rocprofv3 --pmc passes (profiles/r06_conv_pmc*.json, r06_conv_traffic_by_kernel*.json);
                  `pipes` has the fp32-MFMA layers against 157.3 TFLOP/s; `whole_frame` prices the timed configuration.
  fp32_level   -- the same workload in the exact-split arithmetic (fp32 MFMA / bf16x6: all 24 operand bits), with its own
                  `roofline` and single-sequence figure; `value_by_arithmetic` puts both legs side by side at top level.
  single_sequence, objects -- one sequence at a time (the reference's FPS semantics); 1 and 3 objects, both arithmetics.
  em_matching  -- the EM / matching kernels against the fp32 matrix peak (algorithmic and executed FLOPs).
  cpu_baseline -- the CPU oracle (oracle/, a port of the reference's PyTorch path) on the same clip, bounded sample.
  whole_frame, conv_frac_time_weighted -- from the roofline leg; training -- BASELINE configs C / D (training_leg).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

H, W, OUT_HW, N_OBJ = 480, 864, (480, 854), 2
CFG = dict(BACKBONE='resnet50', NUM_BASES=256, NUM_EM_ITERS=5, SINGLE_OBJ=False, KEYDIM=128, VALDIM=512,
           EM_TAU=0.05, TOPL=64)
FP32_MATRIX_PEAK_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CUs @ 2.4 GHz
BF16X6_PEAK_TFLOPS = round(2500.0 / 6, 1)  # dense bf16 MFMA peak / six products per fp32 product (bf16x6 conv mode)
BF16X3_PEAK_TFLOPS = round(2500.0 / 3, 1)  # ... / three products (bf16x3 and f16x3 modes: hi + mid planes; the dense f16 MFMA peak
                                           # equals the bf16 one, MI355X_MICROARCH.md)


def algorithmic_flops_per_frame(n):
    """SURVEY.md section 8d / BASELINE.md section 3."""
    return (73.3 + n * 301.9) * 1e9


def em_flops_per_frame(n, P=1620, L=256, C=128, V=512, T=5, Lm=512):
    return n * (4.0 * P * L * (C * (3 * T - 1) + V) + 4.0 * Lm * P * (C + V))


def em_flops_executed_per_frame(n, P=1620, L=256, C=128, V=512, T=5, Lm=512):
    """What the kernels really issue: the W step of iteration i-1 and the E step of iteration i share ONE affinity GEMM
    (em_ew16_kernel), so a memorize runs T affinity GEMMs + T M-step GEMMs, not the reference's 3T - 1."""
    return n * (4.0 * P * L * (C * 2 * T + V) + 4.0 * Lm * P * (C + V))


def em_ideal_seconds_executed(n, P=1620, L=256, C=128, V=512, T=5, Lm=512, readout_f16=True):
    """Time of the EXECUTED EM + matching FLOPs of one frame at the peak of the pipe each GEMM runs on: the value readout
    (4 Lm P V per object, 3.4 GFLOP at N = 2) runs as an f16x3 GEMM on the pre-split conv kernel -- ceiling 2500 / 3 TFLOP/s --
    everything else on the fp32 matrix pipe (157.3).  VERDICT r04 item 3c: dividing the readout by the fp32 peak flattered it."""
    readout = n * 4.0 * Lm * P * V
    rest = em_flops_executed_per_frame(n, P, L, C, V, T, Lm) - readout
    return rest / (FP32_MATRIX_PEAK_TFLOPS * 1e12) + readout / ((BF16X3_PEAK_TFLOPS if readout_f16 else FP32_MATRIX_PEAK_TFLOPS) * 1e12)


class FrameRunner:
    """Steady-state frame loop over a pre-staged clip (frames cycle; the memory keeps evolving)."""

    def __init__(self, model, frames, m0):
        from swem_amd import ops
        self.model, self.frames, self.ops = model, frames, ops
        self.t = frames.shape[1]
        self.i = 0
        h, w = frames.shape[-2:]
        with torch.no_grad():
            mk16, _, s16, _, _ = model('encode_key', frames[:, 0])
            init_mask = ops.resize_planes(m0, (h, w), 'nearest')
            mv16 = model('encode_value', frames[:, 0], init_mask, s16)
            model('init', mk16, mv16, m0)

        self.graph = None
        self.look = None            # evaluator.LookaheadGraph: k frames per replay, the key encoder batched over them

    def next_frame(self):
        self.i = self.i % (self.t - 1) + 1
        return self.frames[:, self.i]

    def step(self):
        from swem_amd import evaluator
        if self.look is not None:
            # one frame per call, as the reference's loop; every k-th call replays the group graph (the k frame chains of the
            # group whose keys are ready + the batched key encoder of the next k frames).  With --steps a multiple of k the
            # timed region holds exactly steps frames of work (otherwise up to k-1 more, never fewer).
            if self.left == 0:
                self.grp = (self.grp + 1) % len(self.groups)       # the group after the one whose keys are ready
                self.preds = self.look.run(self.groups[self.grp])
                self.left = self.look.k
            self.left -= 1
            return self.preds[self.look.k - 1 - self.left]
        f = self.next_frame()
        if self.graph is not None:
            return self.graph.run(f)
        with torch.no_grad():
            return evaluator.frame_step(self.model, f, OUT_HW)

    def eager_group(self, k):
        """k frames the way the look-ahead graphs run them, but eagerly (per-launch event timing): one batched key-encoder
        pass, then the k frame chains."""
        from swem_amd import evaluator
        with torch.no_grad():
            grp = torch.cat([self.next_frame() for _ in range(k)])
            keys = self.model('encode_key', grp)
            for j in range(k):
                evaluator.frame_chain(self.model, evaluator.key_item(keys, j), grp[j:j + 1], OUT_HW)

    def enable_graph(self, pipelined=False, lookahead=0):
        """Capture the steady state into HIP graphs (both banks must exist: call after >= 2 eager steps).
        lookahead = k > 0: evaluator.LookaheadGraph (k frames per replay, one batched key-encoder pass for the next k;
        pipelined: that pass on a side stream next to the current group's frame chains).  lookahead = 0: one frame per
        replay; pipelined: evaluator.PipelinedFrameGraph (the previous frame's memorize under this frame's key encoder)."""
        from swem_amd import evaluator
        if lookahead > 0:
            k = lookahead
            # the clip's frames 1..t-1 cycle; the groups of k consecutive frames of that cycle, staged once
            cyc = [1 + (self.i + j) % (self.t - 1) for j in range(k * (self.t - 1))]
            self.groups = [torch.cat([self.frames[:, c] for c in cyc[g * k:(g + 1) * k]]).contiguous()
                           for g in range(self.t - 1)]
            self.look = evaluator.LookaheadGraph(self.model, self.frames[:, 1].shape, OUT_HW, k,
                                                 overlap=pipelined).capture(self.groups[0])
            self.look.prime(self.groups[0])
            self.grp, self.left, self.preds = 0, 0, None
            return
        cls = evaluator.PipelinedFrameGraph if pipelined else evaluator.FrameGraph
        self.graph = cls(self.model, self.frames[:, 1].shape, OUT_HW).capture(self.frames[:, 1])


class LockstepRunner:
    """S sequences in lock step on one stream (evaluator.LockstepGraph): a step = one frame of EACH of them.  Built from S warmed-up
    FrameRunners (their models hold the sequences' memories; their staged clips give the frame groups).  graph=False (or `look` set
    to None later): the same groups eagerly (per-launch timing, profiler runs)."""

    def __init__(self, runners, k, graph=True):
        from swem_amd import evaluator
        self.rs, self.nseq, self.k = list(runners), len(runners), k
        self.model = self.rs[0].model
        per_seq = []
        for rn in self.rs:
            cyc = [1 + (rn.i + j) % (rn.t - 1) for j in range(k * (rn.t - 1))]
            per_seq.append([torch.cat([rn.frames[:, c] for c in cyc[g * k:(g + 1) * k]]) for g in range(rn.t - 1)])
        self.groups = [torch.stack([per_seq[s][g] for s in range(self.nseq)], dim=1).contiguous() for g in range(len(per_seq[0]))]
        self.look = self.graph = self.lane = None
        self.grp, self.left, self.preds = 0, 0, None
        if not graph:      # (eager only: the lane object without captured graphs -- its lane-wide banks and packs serve the eager groups)
            self.lane = evaluator.LockstepGraph([rn.model for rn in self.rs], self.rs[0].frames[:, 1].shape, OUT_HW, k, overlap=False,
                                                forks='none', batched_em=True)
        if graph:
            self.look = evaluator.LockstepGraph([rn.model for rn in self.rs], self.rs[0].frames[:, 1].shape, OUT_HW, k,
                                                overlap=False, forks='none', batched_em=True).capture(self.groups[0])
            self.look.prime(self.groups[0])
            self.lane = self.look

    def eager_group(self, k):
        """The next group of k lock-step frames eagerly -- the launches the captured graphs replay: one key-encoder pass over the
        k x S frames, then the k lock-step chains (EM and matching batched over the lane's sequences)."""
        from swem_amd import evaluator
        assert k == self.k
        self.grp = (self.grp + 1) % len(self.groups)
        grp = self.groups[self.grp]
        lane, S = self.lane, self.nseq
        sets = (lane.state, lane.state2)
        preds = []
        with torch.no_grad():
            keys = self.model('encode_key', grp.view((k * S,) + tuple(grp.shape[2:])))
            for j in range(k):
                preds.append(evaluator.lockstep_chain_batched(lane, evaluator.key_items(keys, j * S, S), grp[j], OUT_HW,
                                                              sets[1 - lane.cur]))
        return preds

    def step(self):
        if self.left == 0:
            if self.look is not None:
                self.grp = (self.grp + 1) % len(self.groups)
                self.preds = self.look.run(self.groups[self.grp])
            else:
                self.preds = self.eager_group(self.k)
            self.left = self.k
        self.left -= 1
        return self.preds[self.k - 1 - self.left]


def host_cpu():
    """CPU model and core counts of this host (lscpu / /proc/cpuinfo; the affinity mask bounds what this process may use)."""
    import re
    import subprocess
    info = {'model': None, 'sockets': None, 'logical_cpus': os.cpu_count(), 'physical_cores': None,
            'logical_cpus_available': len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else os.cpu_count()}
    try:
        txt = subprocess.run(['lscpu'], capture_output=True, text=True, timeout=10).stdout
        get = lambda k: (re.search(r'^%s:\s*(.+)$' % re.escape(k), txt, re.M) or [None, None])[1]
        info['model'] = get('Model name')
        so, cps, tpc = get('Socket(s)'), get('Core(s) per socket'), get('Thread(s) per core')
        if so and cps:
            info['sockets'] = int(so)
            info['physical_cores'] = int(so) * int(cps)
        info['threads_per_core'] = int(tpc) if tpc else None
    except (OSError, ValueError, subprocess.SubprocessError):
        pass
    tpc = info.get('threads_per_core') or 1
    avail = info['logical_cpus_available']
    try:                                   # a cgroup CPU quota (cpu.max: "<quota> <period>") bounds it further
        with open('/sys/fs/cgroup/cpu.max') as f:
            q, per = f.read().split()[:2]
        if q != 'max':
            info['cgroup_cpu_quota'] = round(int(q) / int(per), 2)
            avail = max(1, min(avail, int(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    # physical cores this process can use: the affinity mask / cgroup may expose fewer CPUs than the machine has
    info['physical_cores_available'] = max(1, min(info['physical_cores'] or avail, avail // tpc if avail >= tpc else avail))
    return info


def cpu_baseline(frames, m0, sd, n_frames=20, warm=2):
    """The CPU oracle (a port of the reference's PyTorch path) on the same clip: frame 0 and `warm` frames untimed, then
    the mean over `n_frames` steady-state frames, every host thread torch finds."""
    from oracle import swem_oracle as O
    import torch.nn.functional as F
    cfg = O.make_cfg(**CFG)
    cpu = host_cpu()
    # one torch thread per PHYSICAL core: on an SMT host torch's default of one thread per logical CPU
    # oversubscribes the FP units (round 2: 0.39 frames/s on 128 threads against 0.9 on 8 cores)
    threads = max(1, min(cpu['physical_cores_available'] or torch.get_num_threads(), torch.get_num_threads()))
    torch.set_num_threads(threads)
    fr, m0 = frames.cpu(), m0.cpu()
    t_clip, (h, w) = fr.shape[1], fr.shape[-2:]
    model = O.Model(sd, cfg)
    with torch.no_grad():
        torch.manual_seed(0)
        mk16, _, s16, _, _ = model('encode_key', fr[:, 0])
        model('init', mk16, model('encode_value', fr[:, 0], F.interpolate(m0, size=(h, w), mode='nearest').float(), s16), m0)

        def frame(i):                     # swem_evaluator.py:72-97, every frame memorised
            f = fr[:, 1 + i % (t_clip - 1)]
            qk16, qv16, s16, s8, s4 = model('encode_key', f)
            context, n = model('match', qk16, qv16)
            logits, pred_mask = model('segment', n, context, s8, s4, None, OUT_HW)
            pred = torch.argmax(pred_mask, dim=1, keepdim=True)
            hard = (pred.expand(-1, n + 1, -1, -1) == torch.arange(n + 1).view(1, -1, 1, 1)).type_as(pred)
            pm = F.interpolate(pred_mask, size=(h, w), mode='bilinear', align_corners=False)
            model('memorize', qk16, model('encode_value', f, pm, s16), hard, pm)
        for i in range(warm):
            frame(i)
        t0 = time.time()
        for i in range(n_frames):
            frame(warm + i)
        dt = time.time() - t0
    return {'value': round(n_frames / dt, 4), 'unit': 'frames/s', 'cores': threads, 'kind': 'port', 'cpu': cpu,
            'sample': 'oracle/swem_oracle.py, the same 480x864 clip: frame 0 + %d warm-up frames untimed, then %d steady-state '
                      'frames (encode_key, match, segment, encode_value, memorize) in %.1f s on %d torch CPU threads '
                      '(one per physical core available; %s)' % (warm, n_frames, dt, threads, cpu['model'])}


def dump_outputs(path, outs, limit=64 * 10 ** 6 - 4096):
    """--dump-outputs: the int64 index maps one timed step returned (one (H, W) map per sequence, in sequence order) as
    path/index_maps.npy, float32 of shape (sequences, H, W); above `limit` bytes a fixed seeded sample of its values (flat).
    (The limit leaves room for the .npy header: the file stays within 64 MB.)"""
    import numpy as np
    maps = torch.cat([o.reshape((-1,) + tuple(o.shape[-2:])) for o in outs]).cpu().numpy().astype(np.float32)
    if maps.nbytes > limit:
        keep = np.sort(np.random.default_rng(0).choice(maps.size, limit // maps.itemsize, replace=False))
        maps = maps.reshape(-1)[keep]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, 'index_maps.npy'), maps)


def training_leg(cpu=True, steps=10):
    """BASELINE configs C / D (the training step, reference swem_trainer.py:59-108): a short leg of tools/train_bench.py -- 4 clips of
    3 x 384x384, 2 objects, ResNet-50, K = 256, graph replay, the shipped training plans -- in a CHILD process (its own trainer,
    plan book and HIP graphs; this process keeps its inference models), once per arithmetic: fp32-level (fp32 MFMA / bf16x6 / f16x3
    per layer) and config.AMP (bf16 operands).  Each record carries clips/s, `roofline` (useful FLOPs of the step's convolutions and
    EM / matching GEMMs / time, against the dense matrix peak of its arithmetic) and, for the fp32-level one, `cpu_baseline` (the
    oracle's training step on one clip)."""
    import subprocess
    tool = os.path.join(ROOT, 'tools', 'train_bench.py')
    out = {}
    for key, extra in (('fp32_level', []), ('amp', ['--amp'])):
        plans = os.path.join(ROOT, 'swem_amd', 'plans', 'mi355x_train_384_k256_%s.json' % key)
        cmd = [sys.executable, tool, '--clips', '4', '--steps', str(steps), '--warmup', '1'] + extra
        if os.path.exists(plans):
            cmd += ['--load-plans', plans]
        if cpu and key == 'fp32_level':
            cmd += ['--cpu-baseline']
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
            if r.returncode != 0 or not line:
                out[key] = {'error': (r.stderr or r.stdout)[-600:]}
                continue
            d = json.loads(line[-1])
            d['plans'] = os.path.relpath(plans, ROOT) if os.path.exists(plans) else 'tuned on the device in this run'
            out[key] = d
        except (subprocess.SubprocessError, OSError, ValueError) as e:
            out[key] = {'error': repr(e)[:600]}
    out['note'] = ('tools/train_bench.py in a child process per arithmetic, %d timed steps of 4 clips after the warm-up / capture steps; '
                   'value = clips/s of the replayed step (forward, loss, backward, gradient sum over the lanes, gated AdamW)' % steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--regions', type=int, default=7,
                    help='into how many back-to-back regions the --steps timed steps are split (each a whole number of graph '
                         'replays, bracketed by barrier + synchronize, max over ranks; fewer when --steps holds fewer replays): '
                         '`value` is the MEDIAN region, value_min / value_max the spread (one region of 20 steps is 0.17 s: '
                         'box-to-box and run-to-run noise of +-4 %% otherwise decides the line)')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='after the timed steps, write what the last one returned -- the index map of every sequence of rank 0, '
                         'in sequence order -- to DIR/index_maps.npy (float32; above 64 MB a fixed seeded sample of its pixels).  '
                         'Two runs compute with the same plans where the line\'s plans.digest agrees: shapes missing from the '
                         'shipped plan file are tuned by timing during warm-up, --load-plans FILE fixes them all')
    ap.add_argument('--full', action='store_true',
                    help='after the timed steps, also run every other leg of the line (single sequence, fp32_level, objects, '
                         'roofline, whole_frame, em_matching, cpu_baseline, training); the --no-* options below leave some out.  '
                         'Without it the run stops at the headline: set-up, warm-up, timed steps, --dump-outputs, the JSON line')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--objects', type=int, default=N_OBJ)
    ap.add_argument('--no-autotune', action='store_true')
    ap.add_argument('--save-plans', default=None, help='write the tuned per-layer plans to this JSON file')
    ap.add_argument('--load-plans', default=None, help='reuse plans from this file (no tuning; for profiler runs)')
    ap.add_argument('--no-graph', action='store_true', help='eager launches instead of HIP-graph replay')
    ap.add_argument('--pipeline', choices=('auto', 'on', 'off'), default='auto',
                    help='software-pipelined frame graph (evaluator.PipelinedFrameGraph): +12 %% with one sequence, -10 %% with several '
                         '(their streams already fill the hardware queues); auto = on for --seqs 1 only')
    ap.add_argument('--lookahead', type=int, default=-1,
                    help='frames per graph replay with the key encoder batched over them (evaluator.LookaheadGraph); 0 = one frame '
                         'per replay; default: the divisor of --steps nearest to 8 (the timed region then holds exactly --steps '
                         'frames per sequence: 10 for 20 or 100 steps, 8 for 24 / 40 / 48), else 4 (then the last region also runs '
                         'the rest of a replay it does not count); a value given here must divide --steps')
    ap.add_argument('--seqs', type=int, default=8,
                    help='sequences in flight per GPU (default 8 = two lock-step lanes of four; round 5: --seqs 4 --lockstep 0)')
    ap.add_argument('--lockstep', type=int, default=4,
                    help='S > 1: the sequences run in lanes of S sequences in LOCK STEP (evaluator.LockstepGraph: decoder and value '
                         'encoder batched over the objects of the S sequences, ONE key-encoder pass over S x lookahead frames), '
                         '--seqs / S lanes side by side, each on its own stream; 0: every sequence its own pipeline')
    ap.add_argument('--conv-report', action='store_true', help='per-shape conv timing table on stderr')
    ap.add_argument('--no-em', action='store_true', help='skip the EM/matching timing legs (profiler runs)')
    ap.add_argument('--tune', action='store_true', help='ignore the shipped plan file: tune every layer shape on the device')
    ap.add_argument('--no-roofline', action='store_true', help='skip the per-launch roofline / EM legs (plan search tools)')
    ap.add_argument('--round3-forms', action='store_true', help='tuner also offers the prefetched-fragment / stream-K kernel forms')
    ap.add_argument('--no-legs', action='store_true', help='skip the single-sequence and fp32-level legs (profiler runs)')
    ap.add_argument('--no-training', action='store_true', help='skip the `training` sub-record (BASELINE configs C / D: a short leg '
                                                              'of tools/train_bench.py in a child process, both arithmetics)')
    ap.add_argument('--trace-layers', default=None, help='write the per-launch conv list of the eager roofline frames (JSON)')
    ap.add_argument('--cpu-frames', type=int, default=20, help='timed frames of the CPU baseline (after 2 warm-up frames)')
    ap.add_argument('--max-split', type=int, default=0, help='cap the K-split factors the conv tuner may choose (0 = all)')
    ap.add_argument('--math-modes', type=int, nargs='*', default=None,
                    help='run the WHOLE bench (main timed region, roofline) under ops.conv_math(modes), e.g. 0 1 = the exact-split '
                         'arithmetic as the main leg (profiler runs of that leg); implies --no-legs')
    ap.add_argument('--object-legs', type=int, nargs='*', default=[1, 3],
                    help='extra single-sequence legs at these object counts, both arithmetics (default 1 3; empty: none)')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    if not args.full and (args.conv_report or args.trace_layers):
        ap.error('--conv-report and --trace-layers report on the roofline leg: add --full')
    if args.lookahead > 0 and args.steps % args.lookahead:
        ap.error('--lookahead %d does not divide --steps %d: a timed region would replay frames it does not count'
                 % (args.lookahead, args.steps))
    if args.lookahead < 0:
        # a longer look-ahead batches the key encoder further (8-10 frames: + 2-3 % over 4, profiles/r04_lookahead_sweep.txt); the
        # replay granularity must divide the timed steps, or the region would hold up to k - 1 frames of work it does not count
        args.lookahead = next((k for k in (8, 10, 6, 12, 5, 4) if args.steps % k == 0), 4)

    from swem_amd import dist as sdist
    rank, local_rank, world = sdist.env_world()
    if world != args.gpus and world > 1:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d' % (args.gpus, world))
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (the reference is launched through
        # torch.distributed.launch, train.py:22-41).  Nothing in this process has touched the GPU yet; the ranks are
        # fresh child interpreters, this parent relays rank 0's JSON line and the exit code.
        rc, text = sdist.launch_ranks(args.gpus, [os.path.abspath(__file__)] + sys.argv[1:])
        sys.stdout.write(text)
        sys.stdout.flush()
        raise SystemExit(rc)
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU: swem_amd has no CPU path')
    # one rank per GPU; (ranks wrap around only when a multi-rank run is rehearsed on a smaller box, SWEM_DIST_BACKEND=gloo)
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)        # before the RCCL communicator is created
    dev = torch.device('cuda', local_rank)
    sdist.init()
    # the ranks of a node share one container's CPU quota (16 CPUs per 100 ms on this pool): a rank's torch CPU ops (clip
    # synthesis, weight fill) must not wake a 128-thread pool each -- a burnt quota stalls every thread of every rank
    cpu_threads = sdist.respect_cpu_quota(world)
    ranks = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    if ranks != args.gpus:
        raise SystemExit('--gpus %d but the process group has %d ranks' % (args.gpus, ranks))

    import __graft_entry__
    if rank == 0:
        __graft_entry__.build()
    sdist.barrier()
    from types import SimpleNamespace
    from swem_amd import ops, synth, weights
    from swem_amd.swem import SWEM

    # (the oracle is imported by the cpu_baseline leg only: it is the checker, never part of what is measured)
    cfg = SimpleNamespace(**dict(dict(KEYDIM=128, VALDIM=512, NUM_BASES=256, NUM_EM_ITERS=4, EM_TAU=0.05, TOPL=64,
                                      SINGLE_OBJ=False, BACKBONE='resnet50'), **CFG))
    n_obj = args.objects
    nseq = max(1, args.seqs)
    from swem_amd import evaluator
    # ONE book for every model of this process: tuned on the first sequence, read by all (untuned shapes: a model's default)
    book = ops.PlanBook(fallback=ops.MODEL_FALLBACK)
    plans_src = None
    if args.load_plans:
        book.load(args.load_plans)
        plans_src = args.load_plans
    elif not args.tune and not args.no_autotune and os.path.exists(ops.shipped_plans()):
        # default: the plan file that ships with the library for this workload (per-layer tuner + whole-frame check of the near
        # ties, tools/tune_in_context.py: the tuner times a layer ALONE, which loses 2-4 % of the frame rate to ties that go
        # the other way when four sequences share the chip); shapes it does not hold are tuned on the device
        book.load_shipped()
        plans_src = 'swem_amd/plans/mi355x_480p_k256.json (shipped; shapes it does not hold are tuned during warm-up; --tune re-tunes all)'
    if args.round3_forms:
        ops.TUNE_ROUND3_FORMS = True
    if args.max_split:
        ops._TUNE_SPLITS = tuple(v for v in ops._TUNE_SPLITS if v <= args.max_split)
    tune = not args.no_autotune and not args.load_plans   # per-layer plan chosen by timing, during warm-up only (missing shapes)
    sd_box, clip_box = [None], {}

    def make_runners(n, pipelined, seed_base, tune=tune, n_obj=n_obj):
        """n independent sequences, each its own model (memory banks) on its own probed stream, warmed up (the first one
        tunes the plans of the current conv_math mode into `book`) and captured into its frame graph."""
        rs, sts, pending = [], [], []
        # lock-step lanes (--lockstep S): n / S lanes of S sequences each; a lane is ONE pipeline on one stream
        S_ = args.lockstep if (args.lockstep > 1 and n >= args.lockstep and n % args.lockstep == 0 and args.lookahead > 0) else 0
        nstreams = n // S_ if S_ else n
        # streams that really overlap (two HIP streams can share a hardware queue and then serialise: evaluator.overlapping_streams)
        seq_streams = evaluator.overlapping_streams(nstreams) if nstreams > 1 else [torch.cuda.current_stream()]
        for si in range(n):
            model = SWEM(cfg)
            if sd_box[0] is None:
                sd_box[0] = weights.fill_state_dict(model.state_dict(), seed=3, backbone='resnet50')
            model.load_state_dict(sd_box[0])
            model = model.eval().to(dev)
            model.book = book
            seed = 123 + rank * 16 + si
            if (seed, n_obj) not in clip_box:
                clip_box[(seed, n_obj)] = synth.make_clip(t=8, h=H, w=W, n_obj=n_obj, out_hw=OUT_HW, seed=seed)
            frames_cpu, m0_cpu = clip_box[(seed, n_obj)]
            st = seq_streams[si // S_ if S_ else si]
            with torch.cuda.stream(st):
                torch.manual_seed(seed_base + rank * 16 + si)
                rn = FrameRunner(model, frames_cpu.to(dev), m0_cpu.to(dev))
                ops.AUTOTUNE = tune and si == 0
                for _ in range(max(args.warmup, 2)):
                    rn.step()
                if S_:
                    ops.AUTOTUNE = False
                    pending.append(rn)
                    if len(pending) == S_:       # the lane is complete: capture its lock-step graphs (the first lane tunes the batched shapes)
                        ops.AUTOTUNE = tune and si == S_ - 1
                        lane = LockstepRunner(pending, args.lookahead, graph=not args.no_graph)
                        for _ in range(2 * args.lookahead):
                            lane.step()
                        ops.AUTOTUNE = False
                        rs.append(lane)
                        sts.append(st)
                        pending = []
                    torch.cuda.synchronize()
                    continue
                if not args.no_graph:
                    # (the look-ahead capture's eager passes tune the batched key-encoder shapes while the tuner is on)
                    rn.enable_graph(pipelined=pipelined, lookahead=args.lookahead)
                    ops.AUTOTUNE = False
                    for _ in range(2 * max(args.lookahead, 1)):
                        rn.step()   # (the pipelined one-frame graph's first step runs eagerly: nothing is pending yet)
                ops.AUTOTUNE = False
            torch.cuda.synchronize()
            rs.append(rn)
            sts.append(st)
        return rs, sts

    last_outs = []

    def timed(rs, sts, steps):
        """EXACTLY `steps` steps (one frame of every sequence each) between barrier + synchronize; (frames, seconds) over
        all ranks: total frames, max-over-ranks time.  What the last step returned is left in `last_outs`."""
        sdist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if len(rs) == 1:
                outs = [rs[0].step()]
            else:
                outs = []
                for rn, st in zip(rs, sts):
                    with torch.cuda.stream(st):
                        outs.append(rn.step())
        # (the blocking synchronize sleeps on an interrupt; on hosts that deliver it late -- wake-ups quantised to 100 ms were
        # measured here -- the clock would include up to a tick of idle time: poll the streams' events first)
        ops.spin_sync(sts)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        ops.check_faults()       # (outside the clock) a K-split / stream-K wait that expired inside the region raises here
        sdist.barrier()
        last_outs[:] = outs
        return sdist.reduce_counters(steps * sum(getattr(rn, 'nseq', 1) for rn in rs), elapsed, device=dev)

    def timed_median(rs, sts, steps):
        """EXACTLY `steps` timed steps, split into up to --regions regions back to back -> (frames of the `steps` steps, `steps`
        x the MEDIAN region's seconds per step, frames/s of every region in run order).  Every region is the contract's: a whole
        number of graph replays (k steps of a look-ahead / lock-step runner; the last region also takes the steps that do not
        fill one) between barrier + synchronize, max over ranks; the median is taken over the regions' max-over-ranks times per
        step (every rank computes the same list)."""
        r0 = rs[0]
        k = r0.k if isinstance(r0, LockstepRunner) else (r0.look.k if r0.look is not None else 1)
        groups = steps // k
        n = max(1, min(args.regions, groups))
        sizes = [k * (groups // n + (i < groups % n)) for i in range(n)]
        sizes[-1] += steps - sum(sizes)
        regs = [timed(rs, sts, s) for s in sizes]
        ts = sorted(t / s for (_, t), s in zip(regs, sizes))
        med = ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])
        return regs[0][0] // sizes[0] * steps, med * steps, [round(f / t, 3) for f, t in regs]

    pipelined = args.pipeline == 'on' or (args.pipeline == 'auto' and nseq == 1)
    main_tag, pmc_tag = (), ''
    if args.math_modes:
        mm_ctx = ops.conv_math(tuple(args.math_modes))
        mm_ctx.__enter__()                   # (for the rest of the process)
        args.no_legs = True
        main_tag, pmc_tag = ('math',) + tuple(args.math_modes), '_exact' if tuple(args.math_modes) == (0, 1) else ''
        tune = tune or (not args.no_autotune and not any(k_[10:] == main_tag for k_ in book.conv))
    runners, streams = make_runners(nseq, pipelined, 1234, tune=tune)
    lockstep = isinstance(runners[0], LockstepRunner)
    runner = runners[0].rs[0] if lockstep else runners[0]      # (the per-launch roofline leg traces eager frames of ONE sequence)
    frames_cpu, m0_cpu = clip_box[(123 + rank * 16, n_obj)]
    sd = sd_box[0]
    if args.save_plans and rank == 0:
        book.save(args.save_plans)
    hist = book.math_histogram(main_tag)

    # ---------------- timed region: exactly K steps in all, as up to --regions regions between barrier + synchronize; the median region counts
    total_frames, max_t, region_fps = timed_median(runners, streams, args.steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_outs)

    def launch_text(pipe_, lock_=False):
        if args.no_graph:
            return 'eager'
        if lock_:
            return ('hipGraph replay, %d lane(s) of %d sequences in lock step, %d frames of every sequence per replay: ONE key-encoder pass '
                    'over the %d x %d frames of the next group + %d lock-step frames of the current one (match and memorize per sequence; '
                    'decoder and value encoder batched over the objects of the %d sequences)'
                    % (nseq // args.lockstep, args.lockstep, args.lookahead, args.lockstep, args.lookahead, args.lookahead, args.lockstep))
        if args.lookahead > 0:
            return ('hipGraph replay, %d frames per replay: one batched key-encoder pass for the next %d frames%s + the %d frame '
                    'chains (match, segment, encode_value, memorize) of the current ones'
                    % (args.lookahead, args.lookahead, ' on a side stream' if pipe_ else '', args.lookahead))
        return 'hipGraph replay of the steady-state frame' + (
            ', software-pipelined (previous frame\'s memorize under this frame\'s key encoder)' if pipe_ else '')

    out = None
    # the key says which collective library the process group really runs on: 'rccl_ranks' only when torch's backend is nccl
    # (= RCCL on ROCm); a gloo rehearsal on a smaller box reports 'gloo_ranks' (the old line said rccl_ranks = 2
    # over gloo); a single process has no communicator at all
    backend = torch.distributed.get_backend() if torch.distributed.is_initialized() else None
    ranks_key = 'rccl_ranks' if backend == 'nccl' else ('%s_ranks' % backend if backend else 'ranks')
    if rank == 0:
        fps = total_frames / max_t
        out = {
            'metric': 'frames/sec (480p, K=256 bases, multi-object SWEM inference)', 'value': round(fps, 3),
            'unit': 'frames/s', 'n_gpus': world, ranks_key: ranks, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(1e3 * max_t / args.steps, 3), 'ms_per_frame': round(1e3 * max_t / total_frames * world, 3),
            'timed_regions': len(region_fps), 'value_min': min(region_fps), 'value_max': max(region_fps),
            'value_regions': region_fps,
            'value_note': 'the --steps timed steps run as up to --regions back-to-back regions (each: barrier + synchronize on both '
                          'sides, max over ranks); ms_per_step = the MEDIAN region time per step, value = frames per step / that time',
            'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None,
            # what the arithmetic IS (not a precision claim): storage and accumulation are fp32 everywhere, the convolutions'
            # operands are what the plans say -- the mode that holds most layer shapes names the line, `dtype_detail` has all
            'dtype': ('f32 storage + accumulate; conv operands f16x3 (fp16 hi+mid planes = 22-23 significant bits, 3 MFMA products: '
                      'fp32-level error)' if hist['f16x3'] >= max(hist['bf16x6'], hist['bf16x3'], 1) else
                      'f32 storage + accumulate; conv operands bf16x3 (hi+mid bf16 planes = 16 significant bits, 3 MFMA products)'
                      if hist['bf16x3'] >= max(hist['bf16x6'], 1) else
                      'f32 storage + accumulate; conv operands bf16x6 (exact 3-way bf16 split = 24 significant bits, 6 MFMA products)'
                      if hist['bf16x6'] else 'f32 (fp32 MFMA)'),
            'dtype_detail': {'conv_layer_shapes_by_math': hist, 'em_and_affinity': 'fp32 MFMA',
                             'matching_readout': ('f16x3 (probabilities x 2^14 and value bases as fp16 pairs)'
                                                  if any((v >> 16) & 3 == 3 for v in book.match.values()) else 'fp32 MFMA'),
                             'fp32_level_leg': 'fp32_level = the exact-split arithmetic (conv tuner restricted to fp32 MFMA / bf16x6)'},
            'data': 'synthetic',
            'config': {'workload': 'DAVIS17-val-shaped synthetic 480x864 clip (out 480x854), ResNet-50 key encoder, '
                                   'K=256, 5 EM iters, %d objects, memorise every frame, %d sequence(s) per GPU' % (n_obj, nseq),
                       'objects': n_obj, 'frames_per_step': nseq, 'sequences_per_gpu': nseq, 'parallelism': 'seq-sharded x%d (no collective)' % world,
                       'weights': 'random init of the reference architecture (seeded)',
                       'torch_cpu_threads_per_rank': cpu_threads,
                       'launch': launch_text(pipelined, lockstep), 'lockstep_lanes': (nseq // args.lockstep) if lockstep else 0},
            'fps_per_gpu': round(fps / world, 3),
            'frame_algorithmic_tflops': round(algorithmic_flops_per_frame(n_obj) * fps / world / 1e12, 2),
            'plans': {'conv_layer_shapes_by_math': hist, 'digest': book.digest(),
                      'source': plans_src or ('on-device tuner during warm-up' if tune else 'built-in heuristic (fp32 MFMA)'),
                      'math_modes_allowed': list(ops.CONV_MATH_MODES)},
        }

    def leg_roofline(runner, hist, pmc_tag):
        """Roofline of one leg's dominant conv kernel: per-launch HIP-event timing of eager frames of ONE sequence (runner) in the
        conv_math mode the caller has entered; pmc_tag names the committed counter files (profiles/r05_conv_*<tag>.json)."""
        # ---------------- roofline of the dominant kernel: per-launch HIP-event timing on the launch stream
        per = getattr(runner, 'nseq', 1)        # (a lock-step lane: every eager group holds kla frames of EACH of its sequences)
        kla = args.lookahead if (args.lookahead > 0 and (not args.no_graph or per > 1)) else 0      # (a lane runs whole groups, eagerly too)
        nprof = min(args.steps, 5) if not kla else kla * max(1, 4 // kla) * per       # frames traced eagerly
        runner.graph = runner.look = None       # per-launch timing needs eager launches (same kernels, same plans)

        def eager_frames(n):
            # (per-launch durations are taken on ONE stream: the eager calls' side-stream key encoder, ops.ASYNC_KEY_ENCODER, would
            # run some launches beside others and stretch both)
            # (set directly: ops.flags() starts a new plan / hint epoch, after which producers write their fp32 maps again for a frame)
            saved, ops.ASYNC_KEY_ENCODER = ops.ASYNC_KEY_ENCODER, False
            try:
                if kla:
                    for _ in range(n // (kla * per)):
                        runner.eager_group(kla)
                else:
                    for _ in range(n):
                        runner.step()
            finally:
                ops.ASYNC_KEY_ENCODER = saved
        ops.CONV_TRACE = []
        # (matching's readout GEMM also runs on a conv kernel, launched by the library itself: a marker keeps the launch list
        # aligned with a rocprofv3 kernel trace, tools/conv_by_layer.py; it is priced in `em_matching`, not here)
        real_mp = ops.match_packed

        def marked(qk_, pack_, L_, topl_, tau_, **kw_):
            ops.CONV_TRACE.append((None, None, 2.0 * pack_[1].shape[0] * qk_.shape[-2] * pack_[1].shape[1] * pack_[1].shape[2],      # (N objects x P pixels x V x 4L)
                                   'matching readout GEMM', 0.0, 0, 'readout'))
            return real_mp(qk_, pack_, L_, topl_, tau_, **kw_)
        ops.match_packed = marked
        # The launch stream must never run dry while the frames are traced: with an empty queue a launch's event interval is
        # the HOST's enqueue time (~10 us per Python call), not the kernel's.  A spin kernel holds the GPU back until the host
        # has enqueued all traced frames; the intervals then lie between back-to-back packets of one in-order queue.
        eager_frames(max(kla, 1) * per)             # (the eager batched shapes: workspaces sized, planes hinted)
        torch.cuda.synchronize()
        t_host = time.perf_counter()
        eager_frames(max(kla, 1) * per)
        t_host = (time.perf_counter() - t_host) / (max(kla, 1) * per)      # host time to enqueue one eager frame
        torch.cuda.synchronize()
        ops.CONV_TRACE = []
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        torch.cuda._sleep(10_000_000)
        c1.record()
        torch.cuda.synchronize()
        cyc_per_ms = 10_000_000 / c0.elapsed_time(c1)
        torch.cuda._sleep(int(cyc_per_ms * 1e3 * t_host * nprof * 1.2))
        eager_frames(nprof)
        torch.cuda.synchronize()
        ops.match_packed = real_mp
        tr_all, ops.CONV_TRACE = ops.CONV_TRACE, None
        tr = [t_ for t_ in tr_all if t_[0] is not None]
        if args.trace_layers:                   # per-launch list for tools/conv_by_layer.py (joined with rocprofv3 durations)
            with open(args.trace_layers + pmc_tag, 'w') as f:
                json.dump({'frames': nprof, 'launches': [{'layer': t_[3], 'flops': t_[2], 'bytes': t_[4], 'plan': t_[5],
                                                          'pipe': t_[6], 'event_us': None if t_[0] is None else
                                                          1e3 * t_[0].elapsed_time(t_[1])} for t_ in tr_all]}, f)
        if args.conv_report:
            agg = {}
            for t_ in tr:
                a_ = agg.setdefault((t_[3], t_[6]), [0, 0.0, 0.0])
                a_[0] += 1
                a_[1] += t_[0].elapsed_time(t_[1])
                a_[2] += t_[2]
            print('%-34s %5s %5s %9s %9s %8s' % ('conv shape (BxHxW k s cin->ncols)', 'pipe', 'n/frm', 'us/call', 'ms/frame',
                                                 'TFLOP/s'), file=sys.stderr)
            for (d, pipe), (c, t, f) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
                print('%-34s %5s %5.1f %9.1f %9.3f %8.1f' % (d, pipe, c / nprof, 1e3 * t / c, t / nprof, f / (t * 1e-3) / 1e12),
                      file=sys.stderr)
        # The conv family runs on TWO matrix pipes with different ceilings: layers in bf16x6 mode issue six bf16 MFMA
        # products per fp32 product (ceiling: dense bf16 peak / 6), the rest run v_mfma_f32_32x32x2_f32.  Each pipe's useful
        # FLOPs are priced against its own ceiling; `roofline` is the pipe that holds most of the time.
        pipes = {}
        for t_ in tr:
            d = pipes.setdefault(t_[6], {'ms': 0.0, 'flops': 0.0, 'bytes': 0.0, 'n': 0})
            d['ms'] += t_[0].elapsed_time(t_[1])
            d['flops'] += t_[2]
            d['bytes'] += t_[4]
            d['n'] += 1
        peaks = {'bf16': BF16X6_PEAK_TFLOPS, 'bf16x3': BF16X3_PEAK_TFLOPS, 'f16x3': BF16X3_PEAK_TFLOPS, 'fp32': FP32_MATRIX_PEAK_TFLOPS}
        per_pipe = {}
        for k, d in pipes.items():
            ach = d['flops'] / (d['ms'] * 1e-3) / 1e12
            per_pipe[k] = {'achieved': round(ach, 2), 'peak': peaks[k], 'frac': round(ach / peaks[k], 4),
                           'launches_per_frame': d['n'] // nprof, 'avg_launch_us': round(1e3 * d['ms'] / d['n'], 2),
                           'ms_per_frame': round(d['ms'] / nprof, 3), 'gflop_per_launch': round(d['flops'] / d['n'] / 1e9, 3),
                           'algorithmic_bytes_per_launch': int(d['bytes'] / d['n'])}
        dom = max(pipes, key=lambda k: pipes[k]['ms'])
        # the dominant KERNEL: launches grouped by the template instantiation their plan selects (math mode, block tile,
        # variant = plan bits 20-23: conv.hip); `roofline` prices the one that holds most of the conv time against its pipe
        def kernel_of(t_):
            plan_, pipe_ = t_[5], t_[6]
            if pipe_ == 'fp32':
                return ('fp32', plan_ & 15, (plan_ >> 4) & 15, 0)
            return (pipe_, plan_ & 15, (plan_ >> 4) & 15, (plan_ >> 20) & 15)
        kern = {}
        for t_ in tr:
            d = kern.setdefault(kernel_of(t_), {'ms': 0.0, 'flops': 0.0, 'bytes': 0.0, 'n': 0})
            d['ms'] += t_[0].elapsed_time(t_[1])
            d['flops'] += t_[2]
            d['bytes'] += t_[4]
            d['n'] += 1
        dk = max(kern, key=lambda k: kern[k]['ms'])
        dkd = kern[dk]
        dk_ach = dkd['flops'] / (dkd['ms'] * 1e-3) / 1e12
        # rocprofv3's name of that instantiation (conv.hip: variant -> stages / waves / MFMA shape), for the committed stats
        def bf3s_name(pipe_, wm_, wn_, var_):
            if wm_ == 4:                               # the 256-column tiles (conv_t256_kernel: height = 32 * variant rows, 0 = 256)
                return 'conv_t256_kernel<%s, %d>' % ('true' if pipe_ == 'f16x3' else 'false', 2 * var_)
            one = (wm_, wn_) == (1, 1)
            big = (wm_, wn_) == (2, 2)
            nst, nw, m16, kg = (3 if one != (var_ == 1) else 2), 4, False, 4          # launch_bf3s (conv.hip), default / 1
            if var_ in (12, 13) and big:
                nst, nw, m16 = 4, 8, var_ == 13
            elif var_ in (10, 11):
                nst, m16 = 4, var_ == 11
            elif big and var_ in (14, 2, 3, 6, 8, 9):
                nst, nw, m16, kg = {14: (3, 8, True, 4), 2: (2, 8, False, 4), 3: (3, 8, False, 4), 6: (2, 8, True, 4),
                                    8: (2, 4, False, 2), 9: (3, 4, False, 2)}[var_]
            elif var_ == 4:
                nst, m16 = (3 if one else 2), True
            pf, sk = var_ in (5, 7, 15), False
            if var_ == 5:
                nst, nw, m16, kg = 2, 4, True, 4
            elif var_ == 15:
                nst, nw, m16, kg = 3, 4, True, 4
            elif var_ == 7:
                nst, nw, m16, kg = 4, 8, True, 4
            return 'conv_igemm_bf3s_kernel<%d, %d, %d, %d, %s, %d, %d, %s, %s, %s>' % (
                wm_, wn_, nst, nw, 'true' if m16 else 'false', 2 if pipe_ in ('bf16x3', 'f16x3') else 3, kg, 'true' if pf else 'false',
                'true' if sk else 'false', 'true' if pipe_ == 'f16x3' else 'false')
        dk_name = bf3s_name(*dk) if dk[0] != 'fp32' else 'conv_igemm_pipe_kernel<%d, %d>' % (dk[1], dk[2])
        traffic, tsrc = None, None
        for name in ('r06_conv_traffic_by_kernel%s.json' % pmc_tag, 'r05_conv_traffic_by_kernel%s.json' % pmc_tag, 'r04_conv_traffic_by_kernel%s.json' % pmc_tag,
                     'r03_conv_traffic_by_kernel.json', 'r02_conv_traffic_by_kernel.json'):
            if traffic is not None:
                break
            try:
                with open(os.path.join(ROOT, 'profiles', name)) as f:
                    byk = json.load(f)
                hit = [v for k, v in byk.items() if k.replace('void ', '').replace(' ', '') == dk_name.replace(' ', '')]
                if hit:
                    traffic, tsrc = hit[0]['bytes_per_launch'], 'profiles/' + name
            except (OSError, KeyError, ValueError):
                pass
        if traffic is None:
            for name in ('r03_conv_traffic.json', 'r02_conv_traffic.json', 'r01_conv_traffic.json'):
                try:
                    with open(os.path.join(ROOT, 'profiles', name)) as f:
                        traffic, tsrc = json.load(f)['hbm_bytes_per_launch'], 'profiles/' + name + ' (average over ALL conv launches)'
                    break
                except (OSError, KeyError, ValueError):
                    pass
        mfma_busy, mfma_src = None, None
        try:       # counter evidence of the same kernel from the committed rocprofv3 --pmc passes (tools/pmc_kernels.sh)
            pmc_file = next((f_ for f_ in ('r06_conv_pmc%s.json' % pmc_tag, 'r05_conv_pmc%s.json' % pmc_tag, 'r04_conv_pmc%s.json' % pmc_tag, 'r03_conv_pmc.json')
                             if os.path.exists(os.path.join(ROOT, 'profiles', f_))), 'r03_conv_pmc.json')
            with open(os.path.join(ROOT, 'profiles', pmc_file)) as f:
                pm = json.load(f)
            hit = [v for k, v in pm.items() if k.replace(' ', '') == dk_name.replace(' ', '') and 'mfma_busy' in v]
            if hit:
                mfma_busy, mfma_src = round(hit[0]['mfma_busy'], 4), 'profiles/' + pmc_file
        except (OSError, KeyError, ValueError):
            pass
        # counters copied from committed profile files are only as fresh as those files: older than the conv objects of the
        # library this run loaded = measured on other code
        def stale(src):
            """True when the profile file `src` was measured on other convolution sources than this run's (the round's profile
            set carries the hash of the sources it was taken on: tools/profile_stamp.py -> profiles/rNN_profile_stamp.json);
            a profile of an earlier round, or one without a stamp, is stale by definition."""
            if not src:
                return None
            try:
                name = os.path.basename(src.split(' ')[0])
                with open(os.path.join(ROOT, 'profiles', name[:3] + '_profile_stamp.json')) as f_:
                    stamp = json.load(f_)['conv_sources_sha1']
                sys.path.insert(0, os.path.join(ROOT, 'tools'))
                import profile_stamp
                return bool(stamp != profile_stamp.conv_sources_sha1())
            except (OSError, KeyError, ValueError, ImportError):
                return True
        tot_ms = sum(d_['ms'] for d_ in kern.values())
        roof = {
            'bound': 'mfma', 'mfma_busy': mfma_busy, 'mfma_busy_source': mfma_src, 'mfma_busy_stale': stale(mfma_src),
            'traffic_stale': stale(tsrc),
            # every conv launch of the traced frames, each kernel weighted by the time it holds (what `frac` would be if the conv
            # family were one kernel): the dominant kernel alone no longer speaks for the family -- its share is in dominant_kernel
            'frac_time_weighted_all_conv_kernels': round(sum(d_['flops'] / 1e12 / peaks[k_[0]] for k_, d_ in kern.items()) / (tot_ms * 1e-3), 4),
            'mfma_busy_note': 'SQ_VALU_MFMA_BUSY_CYCLES / SIMD cycles of the dominant kernel on its largest layer, from separate '
                              'rocprofv3 --pmc passes (NOT re-measured by this run): the share of cycles the matrix pipe is busy AT '
                              'THE CLOCK THE CHIP HOLDS (1.7-2.0 GHz under this load), where frac divides by the 2.4 GHz peak',
            'kernel': (dk_name + ' -- implicit-GEMM conv on pre-split bf16 planes moved by LDS-DMA, %s, fp32 accumulate; '
                       'its operand-split and split-K reduce launches are inside the timed intervals'
                       % ('bf16x6 arithmetic (three planes per operand, six v_mfma_f32_32x32x16_bf16 products)' if dom == 'bf16'
                          else 'f16x3 arithmetic (fp16 hi + mid planes, three f16 MFMA products)' if dom == 'f16x3'
                          else 'bf16x3 arithmetic (hi + mid planes, three bf16 MFMA products)')) if dom != 'fp32' else
                      'conv_igemm_pipe_kernel: implicit-GEMM conv on v_mfma_f32_32x32x2_f32',
            'achieved': round(dk_ach, 2), 'peak': peaks[dk[0]], 'unit': 'TFLOP/s',
            'frac': round(dk_ach / peaks[dk[0]], 4), 'traffic': traffic, 'traffic_source': tsrc,
            'dominant_kernel': {'rocprof_name': dk_name, 'plan_tile_variant': list(dk[1:]), 'launches_per_frame': dkd['n'] / nprof,
                                'avg_launch_us': round(1e3 * dkd['ms'] / dkd['n'], 2),
                                'share_of_conv_time': round(dkd['ms'] / sum(d_['ms'] for d_ in kern.values()), 3),
                                'gflop_per_launch': round(dkd['flops'] / dkd['n'] / 1e9, 3),
                                'algorithmic_bytes_per_launch': int(dkd['bytes'] / dkd['n']),
                                'whole_pipe': {'achieved': per_pipe[dom]['achieved'], 'frac': per_pipe[dom]['frac']}},
            # every conv kernel instantiation that holds >= 3 % of the conv time, largest first (round 5: the f16x3 layers are
            # shared between the 128x128 kernel and the 256-column tiles of conv_t256_kernel, one instantiation per tile height)
            'conv_kernels': [{'rocprof_name': (bf3s_name(*k_) if k_[0] != 'fp32' else 'conv_igemm_pipe_kernel<%d, %d>' % (k_[1], k_[2])),
                              'share_of_conv_time': round(d_['ms'] / sum(x_['ms'] for x_ in kern.values()), 3),
                              'launches_per_frame': round(d_['n'] / nprof, 1), 'avg_launch_us': round(1e3 * d_['ms'] / d_['n'], 2),
                              'achieved': round(d_['flops'] / (d_['ms'] * 1e-3) / 1e12, 2),
                              'frac': round(d_['flops'] / (d_['ms'] * 1e-3) / 1e12 / peaks[k_[0]], 4)}
                             for k_, d_ in sorted(kern.items(), key=lambda kv: -kv[1]['ms'])
                             if d_['ms'] >= 0.03 * sum(x_['ms'] for x_ in kern.values())],
            'traffic_note': 'fabric-side bytes per launch of the dominant kernel, (2*FETCH_SIZE + WRITE_SIZE)*1024 / launches, from '
                            'separate rocprofv3 --pmc passes (tools/pmc_bench_traffic.sh, tools/pmc_by_kernel.py); NOT re-measured by '
                            'this run',
            'peak_note': 'bf16 pipes: 2500 TFLOP/s dense bf16 MFMA / products per fp32 product: bf16x6 %.1f, bf16x3 %.1f useful '
                         'TFLOP/s; fp32 pipe: %.1f (MI355X_MICROARCH.md)' % (BF16X6_PEAK_TFLOPS, BF16X3_PEAK_TFLOPS,
                                                                             FP32_MATRIX_PEAK_TFLOPS),
            'pipes': per_pipe,
            'frac_bf16_pipe': per_pipe.get('bf16', {}).get('frac'), 'frac_bf16x3_pipe': per_pipe.get('bf16x3', {}).get('frac'),
            'frac_f16x3_pipe': per_pipe.get('f16x3', {}).get('frac'),
            'frac_fp32_pipe': per_pipe.get('fp32', {}).get('frac'),
            'conv_ms_per_frame_eager_one_stream': round(sum(d['ms'] for d in pipes.values()) / nprof, 3),
            'note': 'useful conv FLOPs (2*M*Cout*KH*KW*Cin, unpadded) of %d eager frames of %s / summed per-launch '
                    'HIP-event durations on the launch stream (the queue held full behind a spin kernel: the intervals are '
                    'GPU time between back-to-back packets, not host enqueue time); the timed region above is graph replay of %d sequence(s) on %d '
                    'stream(s), whose kernels overlap -- `whole_frame` prices THAT'
                    % (nprof, 'ONE sequence' if per == 1 else 'ONE lock-step lane of %d sequences (the launches the timed graphs replay)' % per,
                       nseq, nseq // per),
            'plans_bf16x6': hist['bf16x6'], 'plans_bf16x3': hist['bf16x3'], 'plans_f16x3': hist['f16x3'],
            'plans_total': sum(hist.values())}
        return roof, pipes, per_pipe, peaks, nprof

    # ---------------- the same workload in the reference's own FPS semantics (one sequence at a time,
    # basic_evaluator.py:171-176) and in the EXACT-SPLIT arithmetic (fp32 MFMA / bf16x6 only: every operand bit of the fp32
    # reference enters the products), same steps, same clock; the second leg with its own roofline and single-sequence figure
    def single_leg(seed_base, n_objects=n_obj, tune_=tune):
        r1, s1 = make_runners(1, args.pipeline != 'off', seed_base, tune=tune_, n_obj=n_objects)
        f1, t1, reg1 = timed_median(r1, s1, args.steps)
        d = {'value': round(f1 / t1, 3), 'value_min': min(reg1), 'value_max': max(reg1), 'timed_regions': len(reg1),
             'unit': 'frames/s', 'ms_per_frame': round(1e3 * t1 / f1 * world, 3), 'steps': args.steps,
             'sequences_per_gpu': 1, 'objects': n_objects, 'launch': launch_text(args.pipeline != 'off')}
        del r1, s1
        return d

    # (a plain run ends at the headline: every leg below runs with --full only)
    if args.full and not args.no_legs and world == 1:
        if nseq != 1 and not args.no_graph:
            d1 = single_leg(2234)
            if rank == 0:
                out['single_sequence_fps'] = d1['value']
                out['single_sequence'] = dict(d1, plans_digest=book.digest())
        with ops.conv_math((0, 1)):
            # (a loaded plan file may hold only the default leg's plans: this leg then tunes its own)
            have32 = any(k_[-3:] == ('math', 0, 1) for k_ in book.conv)
            tune32 = tune or (not args.no_autotune and not have32)
            r32, s32 = make_runners(nseq, pipelined, 3234, tune=tune32)
            f32_, t32, reg32 = timed_median(r32, s32, args.steps)
            h32 = book.math_histogram(('math', 0, 1))
            leg = {'value': round(f32_ / t32, 3), 'value_min': min(reg32), 'value_max': max(reg32), 'timed_regions': len(reg32),
                   'unit': 'frames/s', 'ms_per_frame': round(1e3 * t32 / f32_ * world, 3),
                   'steps': args.steps, 'sequences_per_gpu': nseq, 'conv_layer_shapes_by_math': {k_: v_ for k_, v_ in h32.items() if v_},
                   'dtype': 'f32 storage + accumulate; conv operands fp32 (v_mfma_f32_32x32x2_f32) or bf16x6 (exact 3-way bf16 split = '
                            '24 significant bits, 6 MFMA products)',
                   'note': 'the same workload with the conv tuner restricted to fp32 MFMA and bf16x6 (both operands split exactly '
                           'into three bf16 terms), ops.conv_math((0, 1)): no operand bit of the fp32 reference is dropped'}
            if not args.no_roofline:
                roof32, _, _, _, _ = leg_roofline(r32[0], h32, '_exact')      # (a lock-step lane traces its own eager groups)
                leg['roofline'] = roof32
            del r32, s32
            torch.cuda.empty_cache()
            if nseq != 1 and not args.no_graph:
                leg['single_sequence'] = single_leg(4234, tune_=tune32)
                leg['single_sequence_fps'] = leg['single_sequence']['value']
        if rank == 0:
            out['fp32_level'] = leg
            # (the headline runs on 22-23 operand bits; the figure at all 24 bits belongs next to it, at top level)
            out['exact_split_fps'] = leg['value']
            out['exact_split_single_sequence_fps'] = leg.get('single_sequence_fps')
            # both arithmetics side by side at top level (a reader must not mistake one leg for the other)
            out['value_by_arithmetic'] = {
                'f16x3 (shipped plans; fp16 hi+mid operands, 22-23 significant bits; error against float64 = the fp32 kernels\', '
                'tests/test_gpu_ops.py::test_conv2d_f16x3_mode)': {'frames_per_s': out['value'], 'single_sequence_fps': out.get('single_sequence_fps')},
                'exact split (fp32 MFMA / bf16x6: all 24 operand bits)': {'frames_per_s': leg['value'],
                                                                           'single_sequence_fps': leg.get('single_sequence_fps')}}
        torch.cuda.empty_cache()
        # ---------------- other object counts (DAVIS17-val sequences carry 1-5 objects, swem_evaluator.py:59-102; SURVEY 8d:
        # N in {1, 2, 3}): one sequence at a time, both arithmetics, the shipped plans of those shapes
        if args.object_legs and not args.no_graph:
            legs_n = {}
            for n_ in args.object_legs:
                if n_ == n_obj:
                    continue
                d_ = {'f16x3': single_leg(5234 + n_, n_objects=n_)}
                with ops.conv_math((0, 1)):
                    d_['exact_split'] = single_leg(6234 + n_, n_objects=n_, tune_=tune or not args.no_autotune)
                d_['algorithmic_gflop_per_frame'] = round(algorithmic_flops_per_frame(n_) / 1e9, 1)
                legs_n[str(n_)] = d_
            if rank == 0 and legs_n:
                out['objects'] = legs_n
        if args.save_plans and rank == 0:
            book.save(args.save_plans)             # again: with the plans the extra legs tuned

    if args.full and world == 1 and not args.no_roofline:
        roof, pipes, per_pipe, peaks, nprof = leg_roofline(runners[0] if lockstep else runner, hist, pmc_tag)
        out['roofline'] = roof
        out['conv_frac_time_weighted'] = roof['frac_time_weighted_all_conv_kernels']    # (beside roofline.frac: VERDICT r05 item 8)
        # whole frame of the TIMED configuration against the blended ceiling: every FLOP priced at its pipe's peak
        conv_fl = {k: d['flops'] / nprof for k, d in pipes.items()}
        em_fl = em_flops_per_frame(n_obj)
        t_ideal = sum(conv_fl.get(k, 0.0) / (peaks[k] * 1e12) for k in peaks) + em_fl / (FP32_MATRIX_PEAK_TFLOPS * 1e12)
        t_frame = max_t / total_frames * world
        out['whole_frame'] = {'executed_gflop_per_frame': round((sum(conv_fl.values()) + em_fl) / 1e9, 1),
                              'gflop_bf16_pipe': round(conv_fl.get('bf16', 0.0) / 1e9, 1),
                              'gflop_bf16x3_pipe': round(conv_fl.get('bf16x3', 0.0) / 1e9, 1),
                              'gflop_f16x3_pipe': round(conv_fl.get('f16x3', 0.0) / 1e9, 1),
                              'gflop_fp32_pipe': round((conv_fl.get('fp32', 0.0) + em_fl) / 1e9, 1),
                              'ms_per_frame_timed': round(1e3 * t_frame, 3), 'ms_per_frame_at_pipe_peaks': round(1e3 * t_ideal, 3),
                              'frac_of_blended_mfma_ceiling': round(t_ideal / t_frame, 4),
                              'achieved_tflops': round((sum(conv_fl.values()) + em_fl) / t_frame / 1e12, 1)}
        if args.no_em:
            if not args.no_cpu_baseline and world == 1:
                out['cpu_baseline'] = cpu_baseline(frames_cpu, m0_cpu, sd, n_frames=args.cpu_frames)
            print(json.dumps(out))
            if torch.distributed.is_initialized():
                torch.distributed.destroy_process_group()
            return
        # EM / matching: capture the arguments of one real memorize + match call, then time 20 back-to-back
        # repetitions of each with HIP events (queue kept full, so this is device time, not host launch time)
        # (the calls below are made outside model(...): they must see the plans of the timed run -- matching's readout plan --
        # so its book is made current for the whole leg; round 3's first bench lines ran this leg on the EMPTY default book,
        # i.e. with the fp32 three-kernel readout, and read 0.35 where tools/em_bench.py read 0.39)
        book_ctx = ops.use_book(book)
        book_ctx.__enter__()
        orig_mem, orig_match = ops.memorize, ops.match_packed
        cap = {}

        def grab(name, fn):
            def wrap(*a, **k):
                cap[name] = (a, k)
                return fn(*a, **k)
            return wrap
        ops.memorize, ops.match_packed = grab('mem', orig_mem), grab('match', orig_match)
        runner.step()
        ops.memorize, ops.match_packed = orig_mem, orig_match
        torch.cuda.synchronize()
        reps = 20
        em_ms = 0.0
        for name, fn in (('mem', orig_mem), ('match', orig_match)):
            a, k = cap[name]
            fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn(*a, **k)
            e1.record()
            e1.synchronize()
            em_ms += e0.elapsed_time(e1) / reps
        em_tf = em_flops_per_frame(n_obj) / (em_ms * 1e-3) / 1e12
        out['em_matching'] = {'ms_per_frame': round(em_ms, 3), 'achieved': round(em_tf, 2), 'unit': 'TFLOP/s',
                              'peak': FP32_MATRIX_PEAK_TFLOPS, 'frac': round(em_tf / FP32_MATRIX_PEAK_TFLOPS, 4),
                              'note': 'swem_memorize_f32 + swem_match_f32 on one frame\'s real arguments, 20 back-to-back '
                                      'repetitions each; algorithmic FLOPs 4PL(C(3T-1)+V) + 4LmP(C+V) per object'}
        # the same kernels when several independent sequences share the GPU, as the product runs them (--seqs): one HIP
        # graph of memorize + match per stream, replayed together.  A single sequence exposes 204 blocks to 256 CUs and a
        # chain of dependent launches; concurrent sequences fill the rest.
        def em_concurrent(n_streams, reps=20):
            a_mem, k_mem = cap['mem']
            a_mat, k_mat = cap['match']
            graphs, sts, keep = [], [], []      # keep: the graphs replay on these argument tensors
            em_streams = evaluator.overlapping_streams(n_streams)
            for si in range(n_streams):
                am = [t.clone() if torch.is_tensor(t) else t for t in a_mem]
                aq = [t.clone() if torch.is_tensor(t) else t for t in a_mat]
                pk = tuple(t.clone() for t in k_mem['pack'])          # every stream its own packed banks
                k_mem = dict(k_mem, pack=pk)
                aq[1] = pk
                st_ = em_streams[si]
                st_.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st_):
                    def fn(am=am, aq=aq, k_mem=k_mem):
                        orig_mem(*am, **k_mem)
                        orig_match(*aq, **k_mat)
                    fn()
                    st_.synchronize()
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=st_, **ops.graph_capture_kwargs()):
                        for _ in range(reps):
                            fn()
                graphs.append(gr)
                sts.append(st_)
                keep.append((am, aq))
            torch.cuda.synchronize()
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                for gr, st_ in zip(graphs, sts):
                    with torch.cuda.stream(st_):
                        gr.replay()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            tf = em_flops_per_frame(n_obj) * n_streams * reps / best / 1e12
            return {'sequences': n_streams, 'us_per_round': round(1e6 * best / reps, 1), 'achieved': round(tf, 2),
                    'frac': round(tf / FP32_MATRIX_PEAK_TFLOPS, 4)}
        # (lock-step lanes run the per-sequence EM of their sequences one after the other: `lanes` of them are in flight at a time)
        em_streams = (nseq // args.lockstep) if lockstep else nseq
        conc = [em_concurrent(n) for n in sorted({1, 2, em_streams, 4})]
        book_ctx.__exit__(None, None, None)
        em = out['em_matching']
        ex_ratio = em_flops_executed_per_frame(n_obj) / em_flops_per_frame(n_obj)
        em['concurrent'] = [c for c in conc if c['sequences'] > 1]
        mine = [c for c in conc if c['sequences'] == em_streams]
        if mine:       # the number for THIS run's configuration first; the single-sequence figures stay as `isolated`
            one = [c for c in conc if c['sequences'] == 1][0]
            em['isolated'] = {'ms_per_frame': round(one['us_per_round'] / 1e3, 3), 'achieved': one['achieved'],
                              'frac': one['frac'], 'frac_executed_flops': round(one['frac'] * ex_ratio, 4),
                              'launch': 'hipGraph replay, one stream',
                              'eager': {'ms_per_frame': em['ms_per_frame'], 'achieved': em['achieved'], 'frac': em['frac']}}
            em['achieved'], em['frac'] = mine[0]['achieved'], mine[0]['frac']
            em['frac_executed_flops'] = round(mine[0]['frac'] * ex_ratio, 4)
            # the headline of this object: ONE sequence alone, on the FLOPs the kernels really issue
            f16_readout = any((v >> 16) & 3 == 3 for v in book.match.values()) or (book.fallback >> 16) & 3 == 3
            ideal_us = 1e6 * em_ideal_seconds_executed(n_obj, readout_f16=f16_readout)
            em['headline'] = {'frac_executed_flops_one_sequence': round(one['frac'] * ex_ratio, 4),
                              'frac_algorithmic_flops_one_sequence': one['frac'], 'us_per_frame_one_sequence': one['us_per_round'],
                              # every GEMM against the peak of the pipe it runs on (the readout: f16x3, 833 TFLOP/s)
                              'frac_of_blended_ceiling_one_sequence': round(ideal_us / one['us_per_round'], 4),
                              'us_per_frame_at_pipe_peaks': round(ideal_us, 1),
                              'note': 'frac_executed_flops_one_sequence divides ALL executed FLOPs by the fp32 matrix peak (round 3-4 '
                                      'definition, kept for continuity); the value readout (%.1f of the %.1f executed GFLOP) runs on the '
                                      'f16 pipe: frac_of_blended_ceiling prices it there and is the honest figure'
                                      % (n_obj * 4.0 * 512 * 1620 * 512 / 1e9, em_flops_executed_per_frame(n_obj) / 1e9)}
            em['flops_note'] = ('frac = ALGORITHMIC FLOPs (the 3T - 1 key GEMMs of the reference + the value GEMM per memorize) / time / '
                                'fp32 matrix peak; frac_executed_flops counts what the kernels issue (E and W steps share one '
                                'GEMM: 2T key GEMMs), %.3f of the algorithmic figure' % ex_ratio)
            em['ms_per_frame'] = round(mine[0]['us_per_round'] / em_streams / 1e3, 3)
            em['note'] = ('memorize + match of the %d sequences this configuration keeps in flight per GPU, one HIP graph per '
                          'stream replayed together (device time per frame = round time / sequences); `isolated` = one '
                          'sequence alone (the same graph on one stream; `eager` = 20 back-to-back eager calls); algorithmic FLOPs '
                          '4PL(C(3T-1)+V) + 4LmP(C+V) per object' % em_streams)
        if not args.no_cpu_baseline and world == 1:     # reported at N = 1 only
            out['cpu_baseline'] = cpu_baseline(frames_cpu, m0_cpu, sd, n_frames=args.cpu_frames)
    if args.full and rank == 0 and world == 1 and not args.no_training and not args.no_legs:
        out['training'] = training_leg(cpu=not args.no_cpu_baseline)
    if rank == 0:
        print(json.dumps(out))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
