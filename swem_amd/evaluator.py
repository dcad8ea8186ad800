"""Per-sequence inference loop (reference methods/SWEM/swem_evaluator.py:59-102) and the FPS meter
(utils/logger.py:87-108, basic_evaluator.py:171-176).

Same call order as the reference: frame 0 encode_key -> encode_value -> init; then for every frame
encode_key -> match -> segment -> argmax/one-hot -> [bilinear resize -> encode_value -> memorize]
(every frame but the last is memorised).  The reference loop is plain Python over ``model(mode, ...)``;
so is this one, with the resize / argmax / one-hot steps on HIP kernels instead of ATen.
"""
import contextlib
import os
import sys
import time

import torch

from . import ops
from .modules import as_nchw, to_pixel_major


class FrameSecondMeter:
    """utils/logger.py:87-108: fps = frames / synchronised wall time of the per-sequence loops."""

    def __init__(self):
        self.frame_n = 0
        self.total_time = 1e-12
        self.ti = time.time()

    def tic(self):
        self.ti = time.time()

    def toc(self, frame_n):
        self.frame_n += frame_n
        self.total_time += time.time() - self.ti

    @property
    def fps(self):
        return self.frame_n / self.total_time


def range_fallback(model, err, what):
    """A sequence raised SwemRangeError: an activation of THIS model on THIS input left the fp16 range of the f16x3 arithmetic
    (the reference's fp32 inference has no such limit, networks.py:22-32).  The model's book leaves f16x3 for the bf16x6 /
    fp32 kernels (ops.PlanBook.to_full_range: all 24 operand bits, fp32 exponent range) and stays there -- a checkpoint that
    overflows once will again -- and the caller re-runs the sequence, fresh work in this process.  Loud: a warning per model."""
    import warnings
    if model.book.full_range:
        raise err            # (cannot happen: a full-range book produces no fp16 pair)
    n = model.book.to_full_range()
    warnings.warn('swem_amd: %s: %s -- this model now runs the full-range arithmetic (bf16x6 / fp32 kernels; %d tuned f16x3 '
                  'plans converted): about 0.6x the f16x3 frame rate, the reference\'s fp32 range' % (what, err, n), RuntimeWarning)


def retry_full_range(model, what, run, reset=None):
    """run(); if it raises SwemRangeError, move the model's book to the full-range arithmetic (`range_fallback`), let the caller
    drop what the failed attempt left behind (`reset`) and run() again: the result is then the fp32-range result, never a
    silently wrong mask."""
    try:
        return run()
    except ops.SwemRangeError as err:
        range_fallback(model, err, what)
        if reset is not None:
            reset()
        return run()


# ---------------------------------------------------------------------- the pieces of a sequence (swem_evaluator.py:59-102)
def start_sequence(model, frame0, init_mask):
    """The first frame of a sequence (swem_evaluator.py:66-70): encode_key -> nearest resize of the given mask -> encode_value ->
    init.  frame0 (1,3,H,W), init_mask (1,N+1,Ho,Wo)."""
    h, w = frame0.shape[-2:]
    mk16, _, s16, _, _ = model('encode_key', frame0)
    m0 = ops.resize_planes(init_mask.float().contiguous(), (h, w), 'nearest')
    model('init', mk16, model('encode_value', frame0, m0, s16), init_mask)


def frame_scores(model, keys, out_size):
    """match -> segment from a frame's key-encoder outputs `keys` = (qk16, qv16, s16, s8, s4); returns (context, logits,
    probability maps)."""
    qk16, qv16, s16, s8, s4 = keys
    context, n = model('match', qk16, qv16)
    logits, pred_mask = model('segment', n, context, s8, s4, None, out_size)
    return context, logits, pred_mask


def frame_pick(pred_mask, keys, frame, memorize=True):
    """argmax / one-hot -> [bilinear resize to the frame's size]; returns the index map and what the frame's memorize needs
    (`frame_back`; None for a frame that is not memorised)."""
    pred, hard = ops.argmax_onehot(pred_mask, want_onehot=memorize)
    if not memorize:
        return pred, None
    h, w = frame.shape[-2:]
    pm = ops.resize_planes(pred_mask, (h, w), 'bilinear')
    return pred, (frame, pm, hard, keys[0], keys[2])


def frame_front(model, keys, frame, out_size, memorize=True):
    """The front of a steady-state frame: from its keys to the index map plus what `frame_back` needs."""
    return frame_pick(frame_scores(model, keys, out_size)[2], keys, frame, memorize)


def frame_back(model, pending, em_stream=None):
    """The back of a steady-state frame: encode_value -> memorize, from `frame_front`'s second result.
    em_stream: run the part of memorize that does not read the value map -- every E, W and key M step, 2T - 1 of its 2T
    launches (modules.py:129-163 need the key, the masks and the prior only) -- on that stream BESIDE encode_value, and only
    the value update behind it (SWEM.memorize_begin / memorize_end: the same blocks on the same data, identical results)."""
    frame, pm, hard, qk16, s16 = pending
    tok = None
    if em_stream is not None:
        main = torch.cuda.current_stream()
        em_stream.wait_stream(main)
        with torch.cuda.stream(em_stream):
            tok = model.memorize_begin(qk16, hard, pm)
    mv16 = model('encode_value', frame, pm, s16)
    if em_stream is not None:
        main.wait_stream(em_stream)
    if tok is None:
        model('memorize', qk16, mv16, hard, pm)
    else:
        if not torch.cuda.is_current_stream_capturing():
            for t_ in (tok['kappa'], tok['zita'], tok['z']):
                t_.record_stream(main)
        model.memorize_end(tok, mv16)


def frame_chain(model, keys, frame, out_size, memorize=True, em_stream=None):
    """The part of a frame that depends on the memory (swem_evaluator.py:77-97): match -> segment -> argmax / one-hot ->
    [bilinear -> encode_value -> memorize], from the frame's key-encoder outputs `keys` (em_stream: see frame_back)."""
    pred, pending = frame_front(model, keys, frame, out_size, memorize)
    if pending is not None:
        frame_back(model, pending, em_stream)
    return pred


def frame_step(model, frame, out_size, memorize=True):
    """One steady-state frame (swem_evaluator.py:72-97) for a (1,3,H,W) device tensor; returns the index map."""
    return frame_chain(model, model('encode_key', frame), frame, out_size, memorize)


# ---------------------------------------------------------------------- the eager per-sequence loops
def evaluate_davis_seq(model, frames, init_masks, out_size, trace=None):
    """frames (1,T,3,H,W) in [0,1] on the device; init_masks list with a (1,N+1,Ho,Wo) float mask first;
    returns (list of (1,Ho,Wo) int64 index maps, list of (1,N+1,Ho,Wo) probability maps).
    A sequence whose activations leave the fp16 range of the default f16x3 arithmetic is re-run in the full-range one
    (`retry_full_range`)."""
    return retry_full_range(model, 'evaluate_davis_seq', lambda: _davis_seq(model, frames, init_masks, out_size, trace),
                            reset=None if trace is None else trace.clear)


def _davis_seq(model, frames, init_masks, out_size, trace=None):
    ops.drain_faults('evaluate_davis_seq')      # (a fault left by earlier work is not this sequence's: ops.FAULT_OWNERS)
    preds, pred_scores = [], []
    t = frames.shape[1]
    out_size = (int(out_size[0]), int(out_size[1]))
    start_sequence(model, frames[:, 0], init_masks[0])
    for i in range(1, t):
        keys = model('encode_key', frames[:, i])
        context, logits, pred_mask = frame_scores(model, keys, out_size)
        pred_scores.append(pred_mask)
        pred, pending = frame_pick(pred_mask, keys, frames[:, i], memorize=i < t - 1)
        if trace is not None:
            trace.append(dict(zip(('qk16', 'qv16', 's16', 's8', 's4'), keys), context=context, logits=logits))
        if pending is not None:
            frame_back(model, pending)
        preds.append(pred)
    # the sequence boundary is where the host waits anyway (basic_evaluator.py:171-176 synchronises around every sequence):
    # asynchronous faults of the sequence's launches surface here, not as a silently wrong mask
    ops.check_faults()
    return preds, pred_scores


def evaluate_ytvos_seq(model, frames, init_masks, out_size):
    """swem_evaluator.py:104-148: like the DAVIS loop, but objects may be annotated from a later frame on:
    ``init_masks[i]`` (1,N'+1,Ho,Wo) then zeroes the predicted scores where a new object sits and appends the new
    masks as extra channels; the memory grows by random-initialised bases for the new ids (modules.py:140-146).
    Range faults of the f16x3 arithmetic: as evaluate_davis_seq."""
    return retry_full_range(model, 'evaluate_ytvos_seq', lambda: _ytvos_seq(model, frames, init_masks, out_size))


def _ytvos_seq(model, frames, init_masks, out_size):
    ops.drain_faults('evaluate_ytvos_seq')
    preds = []
    t = frames.shape[1]
    out_size = (int(out_size[0]), int(out_size[1]))
    start_sequence(model, frames[:, 0], init_masks[0])
    for i in range(1, t):
        keys = model('encode_key', frames[:, i])
        pred_mask = frame_scores(model, keys, out_size)[2]
        if init_masks[i] is not None:
            pred_mask = ops.inject_objects(pred_mask, init_masks[i])
        pred, pending = frame_pick(pred_mask, keys, frames[:, i], memorize=i < t - 1)
        if pending is not None:
            frame_back(model, pending)
        preds.append(pred)
    ops.check_faults()
    return preds


def evaluate_davis_seq_ms(model, frames, init_masks, out_size, scales=(480,), is_flip=False):
    """swem_evaluator.py:34-57: multi-scale / flip test-time augmentation: the probability maps of every pass are
    averaged, the index map is their argmax.  frames (1,T,C,H,W)."""
    assert len(scales) > 0
    final = None
    masks = [m for m in init_masks if m is not None]
    for scale in scales:
        h, w = scale, int((scale / 480) * 864)
        in_frames = ops.resize_planes(frames[0].contiguous(), (h, w), 'bicubic').unsqueeze(0)
        _, scores = evaluate_davis_seq(model, in_frames, init_masks, out_size)
        if is_flip:
            flipped = ops.flip_w(in_frames)
            fmasks = [ops.flip_w(m.float().contiguous()) for m in masks]
            _, fscores = evaluate_davis_seq(model, flipped, fmasks + [None] * (frames.shape[1] - len(fmasks)), out_size)
            scores = [ops.lincomb(a, 0.5, ops.flip_w(bf), 0.5) for a, bf in zip(scores, fscores)]
        k = 1.0 / len(scales)
        final = [ops.lincomb(sc, k) for sc in scores] if final is None else \
            [ops.lincomb(f, 1.0, sc, k) for f, sc in zip(final, scores)]
    return [ops.argmax_onehot(f, want_onehot=False)[0] for f in final]



# ---------------------------------------------------------------------- what the captured graphs share
def _copy_bases(dst, src):
    for key in dst:
        dst[key].copy_(src[key])


def _under(book):
    """The block's current PlanBook: `book`, or whichever is current already (None)."""
    return contextlib.nullcontext() if book is None else ops.use_book(book)


def _need_banks(cores, name):
    if any(c.memories['update'].bases is None or c.memories['first'].bases is None for c in cores):
        raise RuntimeError('%s needs an initialised memory with both banks in every model (run two frames eagerly first)' % name)


def adopt_banks(cores, firsts, states, packs, book=None):
    """Adopt the cores' CURRENT memories (new sequences initialised eagerly, same shapes) into captured graphs' static buffers
    `firsts[s]` / `states[s]`, so one capture serves every sequence of that shape.  False, with nothing touched, unless EVERY
    core holds both banks in the captured shapes and still owns the pack the graphs hold the addresses of (`packs[s]`)."""
    for c, first, pack in zip(cores, firsts, packs):
        cur_first, cur_upd = c.memories['first'].bases, c.memories['update'].bases
        if cur_first is None or cur_upd is None or cur_first['kappa'].shape != first['kappa'].shape or c._pack is not pack:
            return False
    for c, first, state in zip(cores, firsts, states):
        cur_first, cur_upd = c.memories['first'].bases, c.memories['update'].bases
        with _under(book):
            c.repack()                         # (no-op when memorize kept it current, as it does)
        for key in first:
            if cur_first[key] is not first[key]:
                first[key].copy_(cur_first[key])
            if cur_upd[key] is not state[key]:
                state[key].copy_(cur_upd[key])
        c.memories['first'].bases = first
        c.memories['update'].bases = state
        c.restamp()
    return True


class FrameGraph:
    """The steady-state frame captured once into a HIP graph and replayed per frame.

    A frame is ~300 short kernel launches; replaying them from a graph removes the host launch cost and the
    inter-kernel gaps.  Shapes are static within a sequence, the kernels never synchronise and the library
    allocates nothing, so the capture is a plain ``torch.cuda.graph``.  The recurrent state (the 'update' bank)
    lives in static buffers: the captured memorize writes fresh bases, a device copy moves them into the static
    ones at the end of the graph.  Requires both banks to exist (i.e. at least two frames already processed)."""

    def __init__(self, model, frame_shape, out_size, streams=None):
        """streams: (warm-up stream, capture stream) to reuse (SequencePool keeps one pair per lane: a DAVIS / YouTube-VOS
        sweep re-captures for every new object count or frame shape, and HIP streams are never garbage collected)."""
        self.model, self.out_size = model, (int(out_size[0]), int(out_size[1]))
        self.streams = streams
        core = model.swem_core
        _need_banks([core], type(self).__name__)
        upd = core.memories['update'].bases
        self.frame = torch.empty(frame_shape, dtype=torch.float32, device=upd['kappa'].device)
        self.state = {k: v.clone() for k, v in upd.items()}
        core.memories['update'].bases = self.state
        self.first = core.memories['first'].bases           # the captured kernels read these tensors in place
        self.graph = torch.cuda.CUDAGraph()
        self.pred = self.pack = None

    def _warm(self, warm):
        frame_step(self.model, self.frame, self.out_size)

    def _body(self, main):
        pred = frame_step(self.model, self.frame, self.out_size)
        _copy_bases(self.state, self.model.swem_core.memories['update'].bases)
        return pred

    def capture(self, example_frame):
        core = self.model.swem_core
        self.frame.copy_(example_frame)
        with torch.no_grad():
            # one eager pass on a side stream (also sizes every workspace), then restore the state it consumed
            self.streams = self.streams or (ops.new_stream(), ops.new_stream())
            warm, cap = self.streams
            saved = {k: v.clone() for k, v in self.state.items()}
            warm.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(warm):
                self._warm(warm)
            torch.cuda.current_stream().wait_stream(warm)
            _copy_bases(self.state, saved)
            core.memories['update'].bases = self.state
            # matching's packed banks (SWEMCore._pack) are static buffers of the model: bring them in line with the restored
            # state now, so that the captured frame finds them current and contains no repacking
            self.pack = core.repack()
            # capture on a stream of this graph's own: scratch buffers are per stream (ops.workspace), and graphs that are
            # replayed concurrently must not share one (torch's default capture stream is one object for all captures)
            # (scratch requested while capturing is allocated inside the capture and owned by the graph: ops.workspace)
            cap.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(self.graph, stream=cap, **ops.graph_capture_kwargs()):
                self.pred = self._body(cap)
            core.memories['update'].bases = self.state
            core.restamp()          # the captured memorize rewrites the pack's 'update' half together with the state
        return self

    def rebind(self):
        """Adopt the model's CURRENT memory into the captured graph's static buffers (adopt_banks)."""
        return adopt_banks([self.model.swem_core], [self.first], [self.state], [self.pack])

    def run(self, frame):
        """Stage the frame into the static input buffer and replay; returns the (static) int64 index map."""
        self.frame.copy_(frame)
        self.graph.replay()
        return self.pred


class PipelinedFrameGraph(FrameGraph):
    """FrameGraph with the frame software-pipelined for ONE sequence.  Within a sequence the only thing frame t needs from
    frame t-1 is its memory update, and only at `match`: frame t's key encoder is independent of it.  The captured graph
    therefore forks -- frame t-1's encode_value + memorize (its inputs kept in static "pending" buffers) run on a side branch
    under frame t's encode_key -- and joins in front of match.  Every kernel sees exactly the data of the sequential order:
    the index maps are bit-identical (tests/test_gpu_model.py); measured on config B, one sequence: 3.43 -> ~3.0 ms per frame.

    The first run() after capture() / rebind() processes its frame eagerly with the memorize deferred (there is nothing pending
    yet); flush() applies a pending memorize eagerly (the model's memory then equals the sequential loop's)."""

    def __init__(self, model, frame_shape, out_size, streams=None, side_stream=None):
        super().__init__(model, frame_shape, out_size, streams)
        self.side = side_stream
        self.pend = None            # static buffers: frame, soft masks, one-hot masks, key, 1/16 features of the pending frame
        self.primed = False

    def _front(self, keys, frame):
        """The front of one frame; returns its index map, what its deferred memorize needs goes to the pending buffers."""
        pred, cur = frame_front(self.model, keys, frame, self.out_size)
        if self.pend is None:
            self.pend = [t.clone() for t in cur]
        else:
            for dst, src in zip(self.pend, cur):
                if dst is not src:
                    dst.copy_(src)
        return pred

    def _warm(self, warm):
        # a pending frame to size the buffers (any frame will do: everything it touches is restored by capture())
        self._front(self.model('encode_key', self.frame), self.frame)
        self._body(warm)                      # one eager pass: sizes every workspace of both branches
        warm.wait_stream(self.side)

    def _body(self, main):
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            frame_back(self.model, self.pend)
            _copy_bases(self.state, self.model.swem_core.memories['update'].bases)
        keys = self.model('encode_key', self.frame)        # under the side branch
        main.wait_stream(self.side)
        return self._front(keys, self.frame)

    def capture(self, example_frame):
        if self.side is None:
            self.side = overlapping_streams(2)[1]
        super().capture(example_frame)
        self.primed = False
        return self

    def rebind(self):
        ok = super().rebind()
        self.primed = False
        return ok

    def run(self, frame):
        if not self.primed:        # nothing pending yet: this frame eagerly, its memorize deferred
            with torch.no_grad():
                pred = self._front(self.model('encode_key', frame), frame)
            self.primed = True
            return pred
        return super().run(frame)

    def flush(self):
        """Apply the pending memorize (eagerly): afterwards the model's memory is that of the sequential loop."""
        if self.primed:
            with torch.no_grad():
                frame_back(self.model, self.pend)
                core = self.model.swem_core
                _copy_bases(self.state, core.memories['update'].bases)
                core.memories['update'].bases = self.state
                core.restamp()
            self.primed = False


def key_item(keys, j):
    """Frame j's share of a batched encode_key result (NCHW-shaped views of NHWC maps), with the planes the batch carries."""
    return tuple(as_nchw(ops.batch_item(to_pixel_major(t), j)) for t in keys)


def key_items(keys, j, n):
    """Frames j .. j + n - 1 of a batched encode_key result (see key_item)."""
    return tuple(as_nchw(ops.batch_item(to_pixel_major(t), j, n)) for t in keys)


class GroupGraph:
    """k frames per replay of S sequences in lock step, with the key encoder batched over the k x S frames: the skeleton of
    LookaheadGraph (S = 1) and LockstepGraph.

    `encode_key` does not read the memory (swem_evaluator.py:75 vs :77) and the whole sequence is device-resident inside the
    timed region (basic_evaluator.py:157-176), so the key encoder of the NEXT group runs as one batched pass while the k steps of
    the CURRENT group run their memory-dependent chains one after the other.  Two HIP graphs per buffer parity: `kg[p]` (one
    batched pass over the staged `frames[p]`; its outputs `keys[p]` live in that graph's pool) and `cg[p]` (the k chain steps
    reading keys[p]); a replay runs cg[p] and kg[1-p] for the following group on a probed pair of side streams (overlap=True) or
    one behind the other on the caller's stream.  `models[s]` holds sequence s's memory (both banks initialised, the same number
    of objects; replicas share models[0]'s PlanBook).  The recurrent state lives in static buffers, one dict per sequence:
    the steps of a group write their new bases alternately into `state2` and back into `state` -- no copy of the update bank
    per frame (an odd k pays one copy back per group).

    A subclass supplies `_encode(p)` (the key-encoder pass over frames[p]) and `_step(p, j, nxt)` (step j of the group from
    keys[p], the new bases of sequence s into nxt[s]; returns the step's index maps)."""

    def __init__(self, models, frame_shape, out_size, k, lead=(), streams=None, side_stream=None, overlap=True, book=False):
        """lead: the axes of a group between k and the frame's own (3,H,W).  book: run the bare repacks under models[0]'s book
        (False: under whichever book is current, as a single model's graphs always have)."""
        self.models, self.k, self.out_size = list(models), int(k), (int(out_size[0]), int(out_size[1]))
        self.S = len(self.models)
        self.streams, self.side, self.overlap, self.shared_book = streams, side_stream, overlap, book
        name, cores = type(self).__name__, self._cores()
        _need_banks(cores, name)
        if len({tuple(c.memories['first'].bases['kappa'].shape) for c in cores}) != 1:
            raise RuntimeError('%s: the sequences must hold the same number of objects' % name)
        for m in self.models[1:]:
            m.book = self.models[0].book
        dev = cores[0].memories['update'].bases['kappa'].device
        self.frame_shape = tuple(frame_shape)                 # (1, 3, H, W)
        self.frames = [torch.empty((self.k,) + tuple(lead) + self.frame_shape[1:], dtype=torch.float32, device=dev)
                       for _ in range(2)]
        self.state = [{key: v.clone() for key, v in c.memories['update'].bases.items()} for c in cores]
        self.state2 = [{key: torch.empty_like(v) for key, v in st.items()} for st in self.state]
        for c, st in zip(cores, self.state):
            c.memories['update'].bases = st
        self.first = [c.memories['first'].bases for c in cores]           # the captured kernels read these tensors in place
        self.kg = [torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()]
        self.cg = [torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()]
        self.keys = [None, None]
        self.preds = [None, None]
        self.packs = None
        self.p = 0                   # parity of the group whose keys are ready (after prime() / run())
        self.primed = False

    def _cores(self):
        return [m.swem_core for m in self.models]

    def _book(self):
        return self.models[0].book if self.shared_book else None

    def _chains(self, p):
        cores, sets, preds = self._cores(), (self.state, self.state2), []
        for j in range(self.k):
            nxt = sets[(j + 1) % 2]
            preds.append(self._step(p, j, nxt))
            for c, st in zip(cores, nxt):
                c.memories['update'].bases = st       # (the tensors memorize wrote, under their own names)
                c.restamp()
        if self.k % 2:
            for c, a, b in zip(cores, self.state, self.state2):
                _copy_bases(a, b)
                c.memories['update'].bases = a
                c.restamp()
        return preds

    def _restore(self, saved):
        for c, st, sv in zip(self._cores(), self.state, saved):
            _copy_bases(st, sv)
            c.memories['update'].bases = st

    def capture(self, example_frames):
        """example_frames (k,) + lead + (3,H,W): any frames of the sequences' shape (everything the warm-up touches is restored)."""
        with torch.no_grad():
            self.streams = self.streams or (ops.new_stream(), ops.new_stream())
            if self.side is None:
                # (the chains and the side branch replay on a PROBED pair: two streams may share a hardware queue, and the
                # stream the caller happens to be on was never probed against anything)
                self.side = tuple(overlapping_streams(2)) if self.overlap else ()
            warm, cap = self.streams
            saved = [{key: v.clone() for key, v in st.items()} for st in self.state]
            warm.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(warm):
                for p in (0, 1):
                    self.frames[p].copy_(example_frames)
                # eager passes: size every workspace, let the batched layers' consumers report their split requests (the
                # producers then write the planes themselves) and -- while ops.AUTOTUNE is on -- tune the batched layer shapes
                for _ in range(2):
                    self.keys[0] = self._encode(0)
                    self._chains(0)
            torch.cuda.current_stream().wait_stream(warm)
            for p in (0, 1):
                self._restore(saved)
                with _under(self._book()):      # (a shared book: the packs with the value planes THIS book's readout reads)
                    self.packs = [c.repack() for c in self._cores()]
                cap.wait_stream(torch.cuda.current_stream())
                with torch.cuda.graph(self.kg[p], stream=cap, **ops.graph_capture_kwargs()):
                    self.keys[p] = self._encode(p)
                with torch.cuda.graph(self.cg[p], stream=cap, **ops.graph_capture_kwargs()):
                    self.preds[p] = self._chains(p)
                torch.cuda.current_stream().wait_stream(cap)
            self._restore(saved)
            for c in self._cores():
                c.restamp()
        self.primed = False
        return self

    def rebind(self):
        """Adopt the models' CURRENT memories (new sequences of the same shapes) into the captured graphs' static buffers."""
        if not adopt_banks(self._cores(), self.first, self.state, self.packs or [None] * self.S, self._book()):
            return False
        self.primed = False
        return True

    def prime(self, group):
        """Key-encoder pass of the first group."""
        self.frames[self.p].copy_(group)
        self.kg[self.p].replay()
        self.primed = True

    def run(self, next_group=None):
        """The k chain steps of the group whose keys are ready; `next_group` = the following group, whose key encoder runs next
        to them (None: the sequences end).  Returns the k (static) int64 index maps."""
        if not self.primed:
            raise RuntimeError('%s.run before prime()' % type(self).__name__)
        p, main = self.p, torch.cuda.current_stream()
        if next_group is None:
            self.cg[p].replay()
            self.primed = False
            return self.preds[p]
        self.frames[1 - p].copy_(next_group)
        if self.overlap:
            s0, s1 = self.side
            s0.wait_stream(main)
            s1.wait_stream(main)
            with torch.cuda.stream(s0):
                self.cg[p].replay()
            with torch.cuda.stream(s1):
                self.kg[1 - p].replay()
            main.wait_stream(s0)
            main.wait_stream(s1)
        else:
            self.cg[p].replay()
            self.kg[1 - p].replay()
        self.p = 1 - p
        return self.preds[p]


class LookaheadGraph(GroupGraph):
    """k frames of ONE sequence per replay (GroupGraph with S = 1; groups are (k,3,H,W)).

    The key encoder of the NEXT k frames runs as one B = k pass -- a k-th of the launches, k times the grid: the B = 1 layers of
    the ResNet-50 trunk are 10-25 us launches that leave most of the chip idle -- while the k frames of the CURRENT group run
    their frame chains (match -> segment -> encode_value -> memorize).  overlap=True (one lane): the two on a side-stream pair;
    False (several lanes: their streams already fill the hardware queues): one behind the other.  Every kernel sees the data of
    the sequential order; with batch-invariant plans (ops.PlanBook.fallback without a K-split) index maps and memory are those
    of the frame-by-frame loop bit for bit (tests/test_gpu_model.py)."""

    def __init__(self, model, frame_shape, out_size, k, streams=None, side_stream=None, overlap=True, em_overlap=False):
        super().__init__([model], frame_shape, out_size, k, (), streams, side_stream, overlap)
        self.model = model
        # em_overlap: the key half of every memorize (9 of its 10 launches: SWEM.memorize_begin) on a side stream beside the
        # frame's value encoder.  Identical results (tested); measured NEUTRAL on config B (chains 2.26 -> 2.23 ms per frame
        # alone, 2.71 -> 2.72 with the next group's key encoder beside them: the frame is bound by the kernel sum), so off
        self.em_stream = ops.new_stream() if em_overlap else None

    def _encode(self, p):
        return self.model('encode_key', self.frames[p])

    def _step(self, p, j, nxt):
        core = self.model.swem_core
        core._next_out = nxt[0]
        pred = frame_chain(self.model, key_item(self.keys[p], j), self.frames[p][j:j + 1], self.out_size, em_stream=self.em_stream)
        core._next_out = None
        return pred


def lockstep_middle(m0, n, context, keys, frames, out_size):
    """The part of a lock-step frame that treats the objects of all S sequences as one batch (swem.py:52-53, 94-95), through
    models[0]'s engine: decoder -> argmax / one-hot -> bilinear -> value encoder.  context: pixel-major, S * n objects.
    Returns the (S,Ho,Wo) index maps and memorize's inputs (one-hot masks, soft masks, (S,N,V,h,w) value maps)."""
    _, pred_mask = m0('segment', n, as_nchw(context), keys[3], keys[4], None, out_size)
    pred, (_, pm, hard, _, s16) = frame_pick(pred_mask, keys, frames)
    return pred, hard, pm, m0('encode_value', frames, pm, s16)


def lockstep_chain(models, keys, keys_each, frames, out_size, forks, outs=None, fuse_batched=False):
    """frame_chain for ONE frame of each of S sequences in lock step: `models[s]` holds sequence s's memory,
    `keys` = (qk16, qv16, s16, s8, s4) with batch S (models[0]'s key encoder over the S frames), keys_each[s] = sequence s's item of
    them (key_item: with the planes the batch carries), `frames` (S,3,H,W).
    What depends on one sequence's memory only -- match (affinity, top-l, readout, fusion conv) and memorize (EM) -- runs per
    sequence on `forks[s]` (S streams that overlap: evaluator.overlapping_streams), exactly the launches of frame_chain; the
    decoder and the value encoder run ONCE for the S * N objects of all sequences on the caller's stream (lockstep_middle; the
    models are replicas: same weights, one PlanBook) -- 4 x 3,240 rows per 1/16-scale layer instead of four launches of 3,240.
    Needs the same N in every sequence.  outs[s]: the tensors sequence s's new bases go to (GroupGraph's alternating state sets).
    Returns the (S,Ho,Wo) int64 index maps."""
    main = torch.cuda.current_stream()
    S = len(models)
    ctxs, n = [], None
    forks = forks or [main] * S          # (no forks: the per-sequence parts one after the other on the caller's stream)

    def join():
        for st in forks:
            if st is not main:
                main.wait_stream(st)
    for s, (m, st) in enumerate(zip(models, forks)):
        if st is not main:
            st.wait_stream(main)
        with torch.cuda.stream(st):
            if fuse_batched:        # affinity / top-l / readout per sequence; the fusion conv (modules.py:286-291) below, batched
                core = m.swem_core
                with ops.use_book(m.book):
                    c = core._affinity_readout(keys_each[s][0], core.memories['first'].bases, core.memories['update'].bases)
                n_s = core.memories['first'].bases['kappa'].shape[1]
            else:
                c, n_s = m('match', keys_each[s][0], keys_each[s][1])
        if n is not None and n_s != n:
            raise RuntimeError('lockstep_chain: the sequences hold %d and %d objects' % (n, n_s))
        n = n_s
        ctxs.append(c)
    join()
    m0 = models[0]
    if fuse_batched:
        with ops.use_book(m0.book):
            context = m0.engine().fuse_context(torch.cat([c[1].contiguous() for c in ctxs]), to_pixel_major(keys[1]),
                                               torch.cat([c[0] for c in ctxs]))
    else:
        context = torch.cat([to_pixel_major(c) for c in ctxs])
    pred, hard, pm, mv16 = lockstep_middle(m0, n, context, keys, frames, out_size)
    for s, (m, st) in enumerate(zip(models, forks)):
        if st is not main:
            st.wait_stream(main)
        with torch.cuda.stream(st):
            if outs is not None:
                m.swem_core._next_out = outs[s]
            m('memorize', keys_each[s][0], mv16[s:s + 1], hard[s:s + 1], pm[s:s + 1])
            m.swem_core._next_out = None
    join()
    return pred


def lockstep_chain_batched(lane, keys, frames, out_size, nxt):
    """lockstep_chain with EM and matching batched over the lane's sequences as well (LockstepGraph(batched_em=True)): the lane keeps
    the sequences' banks as slices of ONE tensor per bank and their packs as slices of ONE pack, so that affinity / top-l / readout
    and the whole memorize run as single launches over the S * N objects with one key map per sequence
    (swem_match_packed_clips_f32, swem_memorize_packed_clips_f32: per object the same blocks on the same data), and the fusion conv
    takes the matching kernels' own output planes for all objects.  `nxt`: the per-sequence dicts of the state set the new bases go
    to (views of the lane-wide tensors `lane.sets_all[...]`).  Steady state only (both banks, the packs current)."""
    models, S = lane.models, lane.S
    m0 = models[0]
    cores = [m.swem_core for m in models]
    core0 = cores[0]
    qk16, qv16 = keys[:2]
    Ck, h16, w16 = qk16.shape[1:]
    P, L = h16 * w16, core0.n_bases
    cur_all = lane.sets_all[lane.cur]
    nxt_all = lane.sets_all[1 - lane.cur]
    N = cur_all['kappa'].shape[1]
    with ops.use_book(m0.book):
        for c in cores:     # (under the lane's book: whether the packs carry the fp16 value planes depends on the book's readout)
            if not (c._stamped(0, c.memories['first'].bases) and c._stamped(1, c.memories['update'].bases)):
                c.repack()
        xq = to_pixel_major(qk16).view(S, P, Ck)
        mem_img, s_img = ops.match_packed(xq, lane.pack_all, L, core0.topl, core0.tau, hw=(h16, w16), clips=S)
        context = m0.engine().fuse_context(mem_img, to_pixel_major(qv16), s_img)          # (S*N,h,w,V)
    pred, hard, pm, mv16 = lockstep_middle(m0, N, context, keys, frames, out_size)
    with ops.use_book(m0.book):
        masks = ops.mask_prep(hard.contiguous(), pm.float().contiguous(), h16, w16)          # (S*N,2,P)
        vp = to_pixel_major(mv16.flatten(0, 1)).view(S * N, P, -1)
        ops.memorize(xq, vp, masks, cur_all['kappa'].view(S * N, 2, Ck, L), cur_all['nu'].view(S * N, 2, -1, L),
                     cur_all['zita'].view(S * N, 2, L), core0.n_iters, core0.tau, pack=lane.pack_all, prior_packed=True, bank=1,
                     out=(nxt_all['kappa'].view(S * N, 2, Ck, L), nxt_all['nu'].view(S * N, 2, -1, L),
                          nxt_all['zita'].view(S * N, 2, L)), clips=S)
    for c, st in zip(cores, nxt):
        c.memories['update'].bases = st       # (the lane-wide tensors memorize wrote, under the sequence's own views)
        c.restamp()
    lane.cur = 1 - lane.cur
    return pred


class LockstepGraph(GroupGraph):
    """k frames of S sequences per replay, the sequences in lock step: LookaheadGraph with a second batch axis (GroupGraph with
    groups (k,S,3,H,W)).

    ONE key-encoder pass over the k x S frames of the next group (frame-major: the S frames of step j are contiguous), and k
    lockstep_chain steps per replay -- per sequence: match and memorize on S forked streams inside the graph; batched over the
    S * N objects: decoder and value encoder.  `models` are replicas (same weights, one PlanBook), each holding one sequence's
    memory (both banks initialised, the same number of objects)."""

    def __init__(self, models, frame_shape, out_size, k, streams=None, side_stream=None, overlap=True, forks=None, fuse_batched=False,
                 batched_em=False):
        super().__init__(models, frame_shape, out_size, k, (len(models),), streams, side_stream, overlap, book=True)
        self.forks, self.fuse_batched, self.batched_em = forks, fuse_batched, batched_em
        if batched_em:
            self._share_state()

    def _share_state(self):
        """batched_em: the sequences' banks as slices of ONE tensor per bank (the reference's own layout with B = S:
        kappa (S,N,2,C,L), modules.py:129-168) and their packs as slices of one pack -- every sequence's core keeps working on
        its own views (eager frames, re-binding), the lane's batched launches on the whole."""
        S, cores = self.S, self._cores()
        stack = lambda dicts: {key: torch.cat([d[key] for d in dicts]).contiguous() for key in dicts[0]}
        first_all, state_all = stack(self.first), stack(self.state)
        state2_all = {key: torch.empty_like(v) for key, v in state_all.items()}
        views = lambda whole: [{key: v[s_:s_ + 1] for key, v in whole.items()} for s_ in range(S)]
        self.first, self.state, self.state2 = views(first_all), views(state_all), views(state2_all)
        self.sets_all, self.cur = (state_all, state2_all), 0
        N, _, Ck, L = first_all['kappa'].shape[1:]
        self.pack_all = ops.new_pack(S * N, Ck, cores[0].valdim, L, first_all['kappa'].device)
        for s_, c in enumerate(cores):
            c.memories['first'].bases = self.first[s_]
            c.memories['update'].bases = self.state[s_]
            c._pack = (self.pack_all[0][2 * N * s_:2 * N * (s_ + 1)], self.pack_all[1][N * s_:N * (s_ + 1)],
                       self.pack_all[2][N * s_:N * (s_ + 1)])
            c._stamp = [None, None]

    def _encode(self, p):
        return self.models[0]('encode_key', self.frames[p].view((self.k * self.S,) + self.frame_shape[1:]))

    def _step(self, p, j, nxt):
        S = self.S
        if self.batched_em:
            self.cur = j % 2            # (a group starts from the first state set, `state`, and alternates)
            return lockstep_chain_batched(self, key_items(self.keys[p], j * S, S), self.frames[p][j], self.out_size, nxt)
        each = [key_item(self.keys[p], j * S + s) for s in range(S)]
        return lockstep_chain(self.models, key_items(self.keys[p], j * S, S), each, self.frames[p][j], self.out_size, self.forks,
                              outs=nxt, fuse_batched=self.fuse_batched)

    def capture(self, example_frames):
        if self.forks is None:
            self.forks = overlapping_streams(self.S)
        elif self.forks == 'none':
            self.forks = ()
        return super().capture(example_frames)


def run_sequences(model, sequences, meter=None):
    """basic_evaluator.py:149-199 without the disk IO: sequences = iterable of (frames, init_mask, out_size)."""
    meter = meter or FrameSecondMeter()
    results = []
    for frames, init_mask, out_size in sequences:
        with torch.no_grad():
            torch.cuda.synchronize()
            meter.tic()
            preds, _ = evaluate_davis_seq(model, frames, [init_mask] + [None] * (frames.shape[1] - 1), out_size)
            torch.cuda.synchronize()
            meter.toc(frames.shape[1])
        results.append(preds)
    return results, meter


_PROBED = {}


def overlapping_streams(n, device=None, tries=12):
    """n HIP streams that really run concurrently.  HIP multiplexes streams onto a few hardware queues, and two streams on
    one queue execute strictly one after the other (measured: two sequences on two such streams took exactly twice the time
    of one).  There is no query for the queue of a stream, so candidates are probed: a short chain of small kernels is
    replayed on a pair, and a candidate is kept if the pair finishes in well under twice the single-stream time.
    The probe is timed ON THE GPU (HIP events around the replays, which are held back behind a short spin kernel until the
    host has enqueued all of them), not with the host clock: on an 8-GPU node eight ranks share one container's CPU quota,
    and a host that is late by a replay's 0.2 ms would make every pair look serial.  Found streams are
    cached per device for the life of the process."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    have = _PROBED.setdefault(dev.index, [])       # streams found earlier in this process: probe only for the missing ones
    if len(have) >= n:
        return list(have[:n])
    buf = [torch.zeros(1 << 18, dtype=torch.float32, device=dev) for _ in range(tries + n)]

    def chain(st, k):
        g = torch.cuda.CUDAGraph()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            ops.lincomb(buf[k], 1.0)
            st.synchronize()
            with torch.cuda.graph(g, stream=st, **ops.graph_capture_kwargs()):
                for _ in range(60):
                    ops.lincomb(buf[k], 1.0)
        return g

    def run(pairs):
        """GPU time (ms) from the common start to the last stream's end, best of five."""
        main = torch.cuda.current_stream()
        best = None
        for _ in range(5):
            torch.cuda.synchronize()
            start = torch.cuda.Event(enable_timing=True)
            ends = [torch.cuda.Event(enable_timing=True) for _ in pairs]
            torch.cuda._sleep(2_000_000)                 # ~1 ms: the replays below are all enqueued before it ends
            start.record(main)
            for (st, g), e in zip(pairs, ends):
                st.wait_event(start)
                with torch.cuda.stream(st):
                    g.replay()
                    e.record(st)
            torch.cuda.synchronize()
            dt = max(start.elapsed_time(e) for e in ends)
            best = dt if best is None else min(best, dt)
        return best
    chosen = [(st, chain(st, i)) for i, st in enumerate(have)]
    k = len(chosen)
    if not chosen:
        first = ops.new_stream()
        chosen.append((first, chain(first, 0)))
        k = 1
    t1 = run(chosen[:1])
    while len(chosen) < n and k < tries + n:
        cand = ops.new_stream()
        pair = (cand, chain(cand, k))
        k += 1
        # (measured with this probe: pairs on different queues 1.3-1.5 x the single-stream time, pairs on one queue 1.8-1.9 x)
        ratios = [run([c, pair]) / t1 for c in chosen]
        if os.environ.get('SWEM_PROBE_DEBUG'):
            print('probe: candidate %d ratios %s' % (k, ' '.join('%.2f' % v for v in ratios)), file=sys.stderr)
        if all(v < 1.65 for v in ratios):
            chosen.append(pair)
    while len(chosen) < n:                     # no further overlapping candidate found: fall back to plain streams
        chosen.append((ops.new_stream(), None))
    have[:] = [st for st, _ in chosen]
    return list(have)



# what a lane does next (lane_schedule)
BIND, GROUP_AND_NEXT, LAST_GROUP, GRAPH_FRAME, EAGER, EAGER_LAST = 'bind', 'group+next', 'last group', 'graph frame', 'eager', 'eager last'


def lane_schedule(t, k, i, bound, pipelined=False, may_bind=True):
    """Which frames of a sequence go to a captured graph: what a lane whose sequences have `t` frames does at frame `i`
    (frames 1 .. t-1 are processed; frame 0 starts the sequence) with `k` frames per replay (0: the one-frame graphs), and by how
    many frames `i` advances.  bound: a graph is bound to the lane's sequences (pipelined: it is the PipelinedFrameGraph);
    may_bind: binding may be tried now (the pool uses graphs, and this frame's attempt has not failed).

    A captured frame always memorizes; the reference's loop does not memorize a sequence's LAST frame (swem_evaluator.py:89:
    `if i < t - 1`).  The graphs therefore never take the last frame: a group of k frames runs from the graph only while MORE
    than k frames remain, the tail (1 .. k frames) eagerly -- no wasted encode_value + memorize per sequence, and the model's
    memory after run() is the eager loop's.  (The software-pipelined one-frame graph defers every memorize by a frame and simply
    never applies the last one.)  The first two frames run eagerly: they build the two banks.

    BIND (0): get the lane's graph (and prime it with frames i .. i+k-1), then ask again with may_bind=False;
    GROUP_AND_NEXT (k): replay frames i .. i+k-1, the key encoder of i+k .. i+2k-1 beside them;
    LAST_GROUP (k): replay frames i .. i+k-1 and unbind; GRAPH_FRAME (1): replay the one-frame graph;
    EAGER (1): frame_step with memorize; EAGER_LAST (1): frame_step without (frame t-1)."""
    left = t - i
    if not bound and may_bind and i >= 2 and left > max(k, 1):
        return BIND, 0
    if bound and k > 0 and left > k:
        return (GROUP_AND_NEXT if left > 2 * k else LAST_GROUP), k
    if bound and k == 0 and (left > 1 or pipelined):
        return GRAPH_FRAME, 1
    return (EAGER if left > 1 else EAGER_LAST), 1


class LanePool:
    """Sequences in flight on lanes: `lanes[li]` = the models of lane li (one sequence's memory each), `streams[li]` its stream,
    `graphs[li]` the graph captured for it.  A lane takes a chunk of len(lanes[li]) sequences of one shape, runs them frame by
    frame in lock step as `lane_schedule` says, then takes the next chunk.  A subclass supplies `_graph_for(li, clips, i,
    out_size)` (the lane's graph re-bound to the lane's current sequences, None if there cannot be one) and `_group(clips, a, b)`
    (frames a .. b-1 of the lane's clips as the graph stages them)."""

    def _setup(self, lanes, use_graph, lookahead):
        self.lanes = lanes
        for m in self.models[1:]:            # the lanes run the same layers on the same shapes: one PlanBook for all of them
            m.book = self.models[0].book
        # (probed for real concurrency: two streams can share a hardware queue)
        self.streams = overlapping_streams(len(lanes)) if len(lanes) > 1 else [torch.cuda.current_stream()]
        self.graphs = [None] * len(lanes)
        self.graph_streams = [None] * len(lanes)      # per lane: (warm-up stream, capture stream), reused by every re-capture
        self.use_graph, self.lookahead = use_graph, int(lookahead)

    def _drop_graphs(self):
        self.graphs = [None] * len(self.lanes)

    def run(self, sequences, seeds=None):
        """sequences: list of (frames (1,T,3,H,W), init_mask (1,N+1,Ho,Wo), out_size); returns one list of (1,Ho,Wo)
        int64 index maps per sequence (frames 1..T-1), in input order.  seeds: optional torch seed per sequence, set
        right before its memory is initialised (reproducible random bases whatever the interleaving).
        A range fault of the f16x3 arithmetic (ops.SwemRangeError at the final check) moves the lanes' shared book to the
        full-range arithmetic, drops the captured graphs (they hold f16x3 launches) and runs the call's sequences again."""
        return retry_full_range(self.models[0], type(self).__name__ + '.run', lambda: self._run(sequences, seeds), self._drop_graphs)

    def _drive(self, sequences, seeds, chunks, results):
        """Run the chunks (lists of sequence indices, one lane's worth each) over the lanes; fills results[si]."""
        ops.drain_faults(type(self).__name__ + '.run')
        k, todo = self.lookahead, list(chunks)
        state = [None] * len(self.lanes)           # per lane: [chunk, clips, out_size, next frame, preds per sequence, bound graph]
        main = torch.cuda.current_stream()
        for st in self.streams:
            st.wait_stream(main)
        with torch.no_grad():
            while todo or any(l is not None for l in state):
                for li, (models, st) in enumerate(zip(self.lanes, self.streams)):
                    with torch.cuda.stream(st):
                        if state[li] is None:
                            if not todo:
                                continue
                            chunk = todo.pop(0)
                            for m, si in zip(models, chunk):
                                if seeds is not None:
                                    torch.manual_seed(seeds[si])
                                start_sequence(m, sequences[si][0][:, 0], sequences[si][1])
                            clips, out_size = [sequences[si][0] for si in chunk], sequences[chunk[0]][2]
                            # (a graph is bound to ONE chunk of ONE run() call: the record below is unique per chunk)
                            state[li] = [chunk, clips, (int(out_size[0]), int(out_size[1])), 1, [[] for _ in chunk], None]
                            if clips[0].shape[1] <= 1:        # (one-frame sequences: nothing to segment, swem_evaluator.py:72)
                                for si in chunk:
                                    results[si] = []
                                state[li] = None
                            continue
                        chunk, clips, out_size, i, preds, bound = state[li]
                        t = clips[0].shape[1]
                        act, step = lane_schedule(t, k, i, bound is not None, isinstance(bound, PipelinedFrameGraph), self.use_graph)
                        if act == BIND:
                            bound = self._graph_for(li, clips, i, out_size)
                            if bound is not None and k > 0:
                                bound.prime(self._group(clips, i, i + k))
                            act, step = lane_schedule(t, k, i, bound is not None, isinstance(bound, PipelinedFrameGraph), False)
                        if act in (GROUP_AND_NEXT, LAST_GROUP):
                            for p_ in bound.run(self._group(clips, i + k, i + 2 * k) if act == GROUP_AND_NEXT else None):
                                for s_ in range(len(chunk)):
                                    preds[s_].append(p_[s_:s_ + 1].clone())
                            if act == LAST_GROUP:
                                bound = None        # the rest of the sequences (at most k frames) eagerly
                        elif act == GRAPH_FRAME:
                            preds[0].append(bound.run(clips[0][:, i]).clone())
                        else:
                            for s_, m in enumerate(models):
                                preds[s_].append(frame_step(m, clips[s_][:, i], out_size, memorize=act == EAGER))
                        state[li][3], state[li][5] = i + step, bound
                        if i + step >= t:
                            for s_, si in enumerate(chunk):
                                results[si] = preds[s_]
                            state[li] = None
        for st in self.streams:
            main.wait_stream(st)
        ops.check_faults()       # (synchronises: the results are about to be read; a range fault of the lanes raises here)


class SequencePool(LanePool):
    """Several sequences in flight on one GPU, each on its own stream with its own model instance (memory banks):
    sequences are independent and one sequence alone leaves the GPU under-filled (204 blocks in the
    EM kernels, ~300 short launches per frame), so a second one's kernels fill the gaps (+18..25 % frames/s, bench.py).
    A lane of this pool is a lane of one sequence (LanePool; the lanes' streams are probed for real concurrency).
    After a sequence's first two frames (eager: they build the two banks) the steady state runs from HIP graphs captured once
    per lane and re-bound to each new sequence of the same shape: `lookahead` frames per replay with the key encoder batched
    over them (LookaheadGraph; with ONE lane the next group's key encoder runs on a side stream next to the current group's
    frame chains), the last frames of a sequence that do not fill a group eagerly.  lookahead = 0: one frame per replay
    (FrameGraph; a pool of one model then runs the software-pipelined PipelinedFrameGraph)."""

    def __init__(self, models, use_graph=True, lookahead=8, plans='shipped'):
        self.models = list(models)
        # plans='shipped' (default): a pool whose book holds no tuned conv plan yet loads the plan file that ships with the
        # library (swem_amd/plans/: 480p, K = 256, 1-5 objects on MI355X) -- layer shapes it does not hold run the
        # book's fallback (f16x3 on the heuristic tile).  plans=None: the book as it is; a path: that file.
        # The shipped file is f16x3 plans tuned on an MI355X: it is NOT loaded into a book whose owner chose another default
        # arithmetic (book.fallback = 0: the exact fp32 kernels; a book that has left the fp16 range) nor on a device of
        # another architecture -- those run the book as it is.
        book = self.models[0].book
        dev = next(self.models[0].parameters()).device
        if plans is not None and not book.conv and (plans != 'shipped' or
                                                    ((book.fallback >> 16) & 7 == 7 and not book.full_range)):
            path = ops.shipped_plans() if plans == 'shipped' else plans
            if os.path.exists(path):
                book.load(path, device=dev if plans == 'shipped' else None)
        self._setup([[m] for m in self.models], use_graph, lookahead)

    def _group(self, clips, a, b):
        return clips[0][0, a:b]

    def _graph_for(self, li, clips, i, out_size):
        """The lane's graph for this sequence's steady state, (re-)captured if its shapes changed; None if it cannot be used."""
        model, g, k = self.models[li], self.graphs[li], self.lookahead
        frame = clips[0][:, i]
        shape = tuple(frame.shape)
        if k > 0:
            ok = isinstance(g, LookaheadGraph) and g.frame_shape == shape and g.out_size == out_size and g.k == k
        else:
            ok = isinstance(g, FrameGraph) and g.frame.shape == frame.shape and g.out_size == out_size
        if ok and g.rebind():
            return g
        if model.swem_core.memories['update'].bases is None:
            return None
        self.graphs[li] = None                # the replaced graph (and its private pool) goes first
        if k > 0:
            g = LookaheadGraph(model, shape, out_size, k, streams=self.graph_streams[li], overlap=len(self.models) == 1)
            g.capture(self._group(clips, i, i + k))
        else:
            # one lane: the frame software-pipelined (+12 % frames/s); several lanes already fill the hardware queues, a
            # forked graph per lane costs ~10 % there (bench.py --pipeline)
            cls = PipelinedFrameGraph if len(self.models) == 1 else FrameGraph
            g = cls(model, shape, out_size, streams=self.graph_streams[li])
            g.capture(frame)
        self.graphs[li], self.graph_streams[li] = g, g.streams
        return g

    def _run(self, sequences, seeds=None):
        results = [None] * len(sequences)
        self._drive(sequences, seeds, [[si] for si in range(len(sequences))], results)
        return results


class LockstepPool(LanePool):
    """SequencePool for sequences that can march in LOCK STEP: len(models) / lockstep lanes, each a pipeline of `lockstep`
    sequences of the same frame size, length, mask shape and output size (LockstepGraph: one key-encoder pass over
    lockstep x lookahead frames, decoder and value encoder batched over the objects of all its sequences; match and memorize per
    sequence).  run() cuts its sequences into such groups; what does not fill a group runs on a SequencePool over the first
    models.  `models` are replicas (same weights); they share models[0]'s PlanBook.  Measured on config B (two lanes of four
    sequences against four independent pipelines): bench.py, DESIGN.md section 5."""

    def __init__(self, models, lockstep=4, use_graph=True, lookahead=10, plans='shipped', batched_em=True):
        # batched_em (default): a lane runs EM and matching -- and with them the fusion conv -- once for the objects of all its
        # sequences (LockstepGraph(batched_em=True)); False: per sequence (bit-identical to the per-sequence loops under
        # batch-invariant plans; the batched fusion conv picks its tile by ITS row count)
        self.batched_em = bool(batched_em)
        self.models, self.S = list(models), int(lockstep)
        if self.S < 2 or len(self.models) % self.S:
            raise ValueError('LockstepPool: %d models do not make lanes of %d sequences' % (len(self.models), self.S))
        self.rest = SequencePool(self.models[:min(len(self.models), 4)], use_graph=use_graph, lookahead=lookahead, plans=plans)
        self._setup([self.models[i:i + self.S] for i in range(0, len(self.models), self.S)], use_graph, lookahead)

    def _drop_graphs(self):
        super()._drop_graphs()
        self.rest._drop_graphs()

    def _group(self, clips, a, b):
        return torch.stack([f[0, a:b] for f in clips], dim=1)

    def _graph_for(self, li, clips, i, out_size):
        models, g, k = self.lanes[li], self.graphs[li], self.lookahead
        shape = tuple(clips[0][:, i].shape)
        if isinstance(g, LockstepGraph) and g.frame_shape == shape and g.out_size == out_size and g.k == k and g.rebind():
            return g
        if any(m.swem_core.memories['update'].bases is None for m in models):
            return None
        if len({tuple(m.swem_core.memories['first'].bases['kappa'].shape) for m in models}) != 1:
            return None                       # (sequences with different numbers of objects: the lane runs them frame by frame)
        self.graphs[li] = None
        g = LockstepGraph(models, shape, out_size, k, streams=self.graph_streams[li], overlap=False, forks='none',
                          batched_em=self.batched_em)
        g.capture(self._group(clips, i, i + k))
        self.graphs[li], self.graph_streams[li] = g, g.streams
        return g

    def _run(self, sequences, seeds=None):
        """Lanes for every S sequences of one shape; the others on `rest` (as SequencePool.run: same arguments, same results)."""
        S, buckets = self.S, {}
        for si, (frames, init_mask, out_size) in enumerate(sequences):
            key = (tuple(frames.shape), tuple(init_mask.shape), (int(out_size[0]), int(out_size[1])))
            buckets.setdefault(key, []).append(si)
        chunks, rest = [], []
        for idx in buckets.values():
            while len(idx) >= S and self.lookahead > 0 and self.use_graph:
                chunks.append(idx[:S])
                idx = idx[S:]
            rest += idx
        results = [None] * len(sequences)
        self._drive(sequences, seeds, chunks, results)
        if rest:
            sub = self.rest._run([sequences[si] for si in rest], None if seeds is None else [seeds[si] for si in rest])
            for si, r in zip(rest, sub):
                results[si] = r
        return results
