"""Thin Python wrappers over the C ABI (include/swem_hip.h).

torch is used for device memory and the current HIP stream only; every value is computed by
a kernel of libswem_hip.so.  All activations are NHWC fp32 tensors ``(B, H, W, C)``.
"""
import ctypes as C
import os

import torch

from . import _lib

RELU_IN, RELU_OUT, GLU = 1, 2, 4
# plane-count code of the fp16 (hi, mid) pair (include/swem_hip.h, SWEM_PLANES_F16): the operand format of the f16x3 conv
# arithmetic (plan math field 7 = math 3 + SWEM_PLAN_F16); 2 / 3 = bf16 planes
PLANES_F16 = 4
MATH_NAMES = {0: 'fp32', 1: 'bf16x6', 2: 'bf16', 3: 'bf16x3', 7: 'f16x3'}

_ws = {}
# bench.py sets this to a list to time every conv launch with HIP events on the launch stream:
# entries are (start_event, end_event, flops, description)
CONV_TRACE = None
# When True, the first call of a conv layer at a new input shape times a few tilings / K-splits on the device and
# keeps the fastest (passed to the library as the `plan` hint).  Off by default: results never depend on it beyond
# fp32 summation order, but tuning costs a few milliseconds per layer shape.
AUTOTUNE = False
# conv epilogues write the bf16 planes of outputs that later convolutions consume pre-split (learned per layer on the first
# frames: SPLIT_HINTS) instead of a separate split launch per consumer tensor
FUSE_SPLIT = True
# conv2d(planes_only=True) may skip the fp32 map of an output whose only consumer reads the planes
PLANES_ONLY = os.environ.get('SWEM_PLANES_ONLY', '1') != '0'
# True: the tuner also offers the round-3 kernel forms (prefetched fragments, stream-K).  Off by default: timed ALONE they tie
# with the plain forms (the tuner then picks them by noise), in the frame they lose -- persistent and 256-register blocks
# crowd out the kernels of the other streams (inference, four sequences: 427 frames/s with a plan set holding two of them,
# 446 without on the same box; training, 4 clips in flight, AMP: 102 clips/s without, 71-89 with).  The kernels stay
# reachable through an explicit plan (tests/test_gpu_ops.py runs them).
TUNE_ROUND3_FORMS = False


_MODE_GEN = [0]       # bumped by conv_math / flags (process-wide switches that change which kernels a conv call reaches)


class _Plans(dict):
    """A plan table that counts its changes into its book's epoch."""

    def __init__(self, gen):
        super().__init__()
        self._gen = gen

    def _bump(self):
        self._gen[0] += 1

    def __setitem__(self, k, v):
        if self.get(k, None) != v:
            self._bump()
        super().__setitem__(k, v)

    def __delitem__(self, k):
        self._bump()
        super().__delitem__(k)

    def pop(self, *a):
        self._bump()
        return super().pop(*a)

    def clear(self):
        self._bump()
        super().clear()

    def update(self, *a, **kw):
        self._bump()
        super().update(*a, **kw)

    def setdefault(self, k, v=None):
        if k not in self:
            self._bump()
        return super().setdefault(k, v)


class PlanBook:
    """What a model LEARNS about its own launches: the tuned conv plans (layer signature + input shape -> plan hint), the
    tuned readout plans of matching, and the fused-split hints (producer site -> planes its consumers asked for).  Every
    `SWEM` owns one (`model.book`) and makes it the current one for the duration of a `model(mode, ...)` call; models that
    run the same layers on the same shapes -- the lanes of a `SequencePool` -- share one.  Nothing learned under one model
    reaches another: the arithmetic a conv runs (plan bits 16-17: 0 fp32 MFMA, 1 bf16x6, 2 plain bf16, 3 bf16x3) is a
    property of the model under test, never of what ran earlier in the process.  Free-standing `ops.*` calls use the
    process-wide default book (`ops.reset_plans()` empties it)."""

    def __init__(self, fallback=0):
        # `epoch`: bumped by every change of a plan (conv / match tables, fallback).  A planes-only output (conv2d) is allowed
        # only while the consumer's request for planes is of the CURRENT epoch: after any change that could send that consumer
        # down the fp32 path the producer writes the fp32 map again until the consumer has asked anew.
        self._gen = [0]
        self.conv, self.match, self.hints, self.hint_epoch = _Plans(self._gen), _Plans(self._gen), {}, {}
        # producer site -> epoch at which the convolution that ADDS this tensor as its residual last said it can read the addend
        # from operand planes (None: it cannot -- an fp32 kernel).  conv2d(planes_only='block') needs it current.
        self.res_epoch = {}
        # plan hint of a layer shape nobody tuned (0 = the library's heuristic, which picks tile and K-split from the GEMM's
        # size).  A fixed hint without K-split, e.g. 0x111, makes a layer's arithmetic independent of the batch it is called
        # with: every output element is then one k-ordered MFMA chain whatever the grid (tests compare batched and per-frame
        # passes bit for bit under it).
        self.fallback = fallback
        # True once the book has left the f16x3 arithmetic for good (to_full_range): no launch under it reads or writes an fp16
        # operand pair any more, and nothing re-loads f16x3 plans into it
        self.full_range = False

    @property
    def fallback(self):
        return self._fallback

    @fallback.setter
    def fallback(self, v):
        self._fallback = v
        self._gen[0] += 1

    def epoch(self):
        # (AUTOTUNE is part of it: with the tuner on, a consumer whose plan is still 0 times fp32 candidates on its source --
        # a producer that skipped the fp32 map for it under the tuner-off heuristic must write it again)
        return (self._gen[0], _MODE_GEN[0], bool(AUTOTUNE))

    def clear(self):
        self.conv.clear()
        self.match.clear()
        self.hints.clear()
        self.hint_epoch.clear()
        self.res_epoch.clear()

    def to_full_range(self):
        """Leave the f16x3 arithmetic (range |x| < 65520) for the full-range ones, in place: after a SWEM_FAULT_RANGE
        (`check_faults` raised SwemRangeError) the work is re-run under this book and cannot fault again.  Every tuned conv plan
        in math 7 keeps its block tile and K-split and becomes bf16x6 (math 1: three bf16 planes per operand = all 24 bits, the
        fp32 exponent range; kernel variant and tail-split bits are dropped -- some f16x3 variants have no three-plane form);
        matching's readout plans are dropped (-> the fp32 readout from `mvp`); untuned shapes run bf16x6 on the heuristic tile;
        the fused-split hints are forgotten (their producers wrote fp16 pairs) and re-learned on the next frames.  This is the
        reference's own range: its inference runs in fp32 (networks.py:22-32).  Returns the number of conv plans changed."""
        n = 0
        for k, v in list(self.conv.items()):
            w = self._plan_full_range(v)
            if w != v:
                self.conv[k] = w
                n += 1
        self.match.clear()
        self.hints.clear()
        self.hint_epoch.clear()
        self.res_epoch.clear()
        self.fallback = 1 << 16
        self.full_range = True
        return n

    @staticmethod
    def _plan_full_range(v):
        """A tuned plan as a full-range book may hold it: math 7 (f16x3) and math 3 (bf16x3: 16 operand bits -- not the reference's
        arithmetic either) become bf16x6 (math 1) on the same block tile and K-split, kernel variant and tail-split bits dropped
        (some two-plane variants have no three-plane form); the 256-column tile (0x44: the f16x3 kernel's; its bf16x6 form needs
        its own tile height) becomes the 128x128 tile.  ONE conversion for `to_full_range` and `load` (`load` used to
        keep 0x44 with math 1 and no variant, which resolve_plan rejects -> the heuristic tile without the tuned K-split)."""
        if (v >> 16) & 7 in (7, 3):
            if v & 0xff == 0x44:
                v = (v & 0xff00) | 0x22
            return (v & 0xffff) | (1 << 16)
        return v

    def math_histogram(self, tag=()):
        """{'fp32': n, 'bf16x6': n, 'bf16': n, 'bf16x3': n, 'f16x3': n} over the conv plans tuned under the conv_math tag `tag`
        (default: the untagged ones; a plan of 0 is the fp32 heuristic)."""
        out = {n: 0 for n in MATH_NAMES.values()}
        for k, v in self.conv.items():
            if tuple(k[10:]) == tuple(tag):
                out[MATH_NAMES.get((v >> 16) & 7, 'fp32')] += 1
        return out

    def digest(self):
        """Short hash of the plans (which arithmetic and tiling a run used: printed by bench.py, recorded by the tests)."""
        import hashlib
        txt = repr(sorted((tuple(k), v) for k, v in self.conv.items())) + repr(sorted(self.match.items()))
        return hashlib.sha1(txt.encode()).hexdigest()[:12]

    def save(self, path):
        import json
        with open(path, 'w') as f:
            json.dump({'device': device_arch(), 'conv': [[list(k), v] for k, v in self.conv.items()],
                       'match': [[list(k), v] for k, v in self.match.items()]}, f)

    def load(self, path, device=None):
        """Add the plans of a file.  device (a torch device): the plans are only taken if the file names that device's
        architecture ('device': the gcnArchName prefix it was tuned on) -- tile choices tuned on an MI355X are not a default for
        anything else; a mismatch loads nothing and returns False (no device given: loaded unconditionally)."""
        import json
        with open(path) as f:
            d = json.load(f)
        if device is not None and d.get('device') and d['device'] != device_arch(device):
            return False
        conv = {tuple(k): v for k, v in d.get('conv', [])}
        match = {tuple(k): v for k, v in d.get('match', [])}
        if self.full_range:          # (a book that faulted out of the fp16 range stays out of it)
            conv = {k: self._plan_full_range(v) for k, v in conv.items()}
            match = {}
        self.conv.update(conv)
        self.match.update(match)
        return self

    def load_shipped(self, name='mi355x_480p_k256'):
        """The plan file that ships with the library for a named workload (swem_amd/plans/): the per-layer tuner's choices
        checked in the whole frame (tools/tune_in_context.py).  Opt-in: a fresh book is empty = the fp32 kernels."""
        return self.load(shipped_plans(name))


def device_arch(device=None):
    """'gfx950' for an MI355X: the architecture name plan files are keyed by."""
    if not torch.cuda.is_available():
        return None
    return torch.cuda.get_device_properties(device if device is not None else torch.cuda.current_device()).gcnArchName.split(':')[0]


def shipped_plans(name='mi355x_480p_k256'):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), 'plans', name + '.json')


# What a MODEL's book answers for a layer shape nobody tuned (SWEM.__init__): the library's heuristic tile / K-split in the
# f16x3 arithmetic -- fp32-level error (tests/test_gpu_ops.py::test_conv2d_f16x3_mode) at 2-4 x the exact fp32 kernels' speed, so
# that an object count or a frame size outside the shipped plan file is not a performance cliff.  Layers the
# pre-split kernel cannot take (stems on 4 / 8 channels) run the fp32 kernels as before.  model.book.fallback = 0 gives the exact
# fp32 MFMA kernels everywhere; the free-standing default book (plain ops.* calls) keeps 0.
MODEL_FALLBACK = 7 << 16
BOOK = PlanBook()     # the current book (the default one until a model makes its own current: use_book)
MATH_RAN = None       # tests / bench set this to a dict: plan math field of every conv LAUNCH (what really ran) -> count


class flags:
    """Context: set module switches (FUSE_SPLIT, TUNE_ROUND3_FORMS, ...) for the duration of a block."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        g = globals()
        self.saved = {k: g[k] for k in self.kw}
        g.update(self.kw)
        _MODE_GEN[0] += 1

    def __exit__(self, *a):
        globals().update(self.saved)
        _MODE_GEN[0] += 1


class use_book:
    """Context: make `book` the current PlanBook (SWEM.forward, SWEMTrainer.one_step)."""

    def __init__(self, book):
        self.book = book

    def __enter__(self):
        global BOOK
        self.saved, BOOK = BOOK, self.book
        return self.book

    def __exit__(self, *a):
        global BOOK
        BOOK = self.saved


def reset_plans():
    """Forget everything the CURRENT book learned (tests: before every test)."""
    BOOK.clear()


def __getattr__(name):
    # the current book's tables under their round-1/2 names (tools and tests poke them directly)
    if name == '_CONV_PLANS':
        return BOOK.conv
    if name == '_MATCH_PLANS':
        return BOOK.match
    if name == 'SPLIT_HINTS':
        return BOOK.hints
    raise AttributeError(name)


_PACK_KEY = [('pack',), 0]


class pack_keys:
    """Context: ConvPacks built inside get the site keys (prefix, 1), (prefix, 2), ... in construction order, so that a
    re-built Engine of the same model finds the hints its predecessor's layers left in the model's book."""

    def __init__(self, *prefix):
        self.prefix = tuple(prefix)

    def __enter__(self):
        self.saved = list(_PACK_KEY)
        _PACK_KEY[0], _PACK_KEY[1] = self.prefix, 0

    def __exit__(self, *a):
        if self.saved[0] == ('pack',):
            self.saved[1] = max(self.saved[1], 0)
        _PACK_KEY[0], _PACK_KEY[1] = self.saved


def _next_pack_key():
    _PACK_KEY[1] += 1
    return _PACK_KEY[0] + (_PACK_KEY[1],)
# math modes the conv tuner may choose from: 0 = fp32 MFMA, 1 = bf16x6 (exact 3-way bf16 split, six products: fp32-level
# error), 3 = bf16x3 (hi + mid planes, the three products above 2^-16: 16 significant bits per operand, half the MFMA work
# of bf16x6; the per-stage 1e-4 and per-frame 1e-3 parity bars are asserted with it enabled)
# 7 = f16x3 (round 4): the bf16x3 kernel on fp16 (hi, mid) planes -- 23 significant bits per operand, fp32-level error
# (measured beside fp32 MFMA and bf16x6: tests/test_gpu_ops.py::test_conv2d_f16x3_mode) at the bf16x3 cost.  It replaces
# bf16x3 in the default set: bf16x3 (16 bits) stays reachable through conv_math((3,)) or an explicit plan.
CONV_MATH_MODES = (0, 1, 7)
_TUNE_TILES = ((2, 2), (1, 2), (2, 1), (1, 1))   # (2, 1) = 128x64: pre-split kernels only (64-channel layers)
_TUNE_SPLITS = (1, 2, 3, 4, 6, 8, 12, 16)
TUNE_T256 = True     # offer the tuner the 256-column tiles of conv_t256_kernel (round 5)


def _stream():
    # (the raw handle of torch's current stream of the current device, straight from the C++ binding: the Python-level
    # torch.cuda.current_stream() costs ~5 us per call -- device-index plumbing and a Stream object -- and an eager frame asks
    # ~800 times: a quarter of the host time of the reference's loop as written, tools/host_profile.py)
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


_hip = None


# The key encoder of an eager model('encode_key', frame) call on a side stream (swem.SWEM._encode_key_side)
ASYNC_KEY_ENCODER = os.environ.get('SWEM_ASYNC_KEY', '1') != '0'


def record_stream_deep(t, stream):
    """Tell the caching allocator that `t` -- and what this package hangs on it: producer-written operand planes, the decoder's
    skip convolution computed in the key pass -- is used on `stream` although another stream allocated it."""
    if not t.is_cuda:
        return
    t.record_stream(stream)
    d = t.__dict__
    for planes, _npl in (d.get('_swem_split') or {}).values():
        planes.record_stream(stream)
    sk = d.get('_swem_skip')
    if sk is not None:
        record_stream_deep(sk[0], stream)


def graph_capture_kwargs():
    """Keyword arguments for torch.cuda.graph(...) in this process: with a torch.distributed process group alive, the collective
    library's watchdog thread polls events of earlier collectives, and under the default capture mode ("global") such a call from
    ANOTHER thread while this thread captures invalidates the capture -- measured in round 6 on a one-rank RCCL group (the trainer's
    first captured step aborted the process, tests/_rccl_single_rank_probe.py).  This package's captures only concern the capturing
    thread's own launches: "thread_local".  Without a process group: the default."""
    import torch.distributed as dist
    return {'capture_error_mode': 'thread_local'} if (dist.is_available() and dist.is_initialized()) else {}


# engine.py, _SharedSourceSplit: the clip's key feature split off the value encoder's fusion block (computed once per clip, not per
# object).  SWEM_SPLIT_SHARED=0 / False: the one-launch form of rounds 1-5.
SPLIT_SHARED_SOURCE = os.environ.get('SWEM_SPLIT_SHARED', '1') != '0'
# ... and its two per-clip halves (conv1's, the downsample's) as ONE launch where the shared feature is known to be non-negative
SPLIT_SHARED_MERGE = os.environ.get('SWEM_SPLIT_SHARED_MERGE', '1') != '0'


def new_stream():
    """A HIP stream of its own.  torch.cuda.Stream() hands out 32 pooled streams round robin, so the 33rd request is the
    first stream again; scratch buffers are keyed by stream (workspace()) and captured graphs own theirs, so an aliased
    stream would let two concurrent users share one.  hipStreamCreateWithFlags + ExternalStream has no such limit."""
    _hip_runtime()
    h = C.c_void_p()
    torch.cuda.current_device()                      # the HIP context of the current device exists
    rc = _hip.hipStreamCreateWithFlags(C.byref(h), 1)   # hipStreamNonBlocking
    if rc != 0 or not h.value:
        raise _lib.SwemHipError('hipStreamCreateWithFlags failed (%d)' % rc)
    return torch.cuda.ExternalStream(h.value)


def spin_sync(streams=None):
    """Wait for the work queued so far on `streams` (default: the current stream) by POLLING events, with a short sleep between
    polls.  Rounds 1-3 saw blocking waits return up to 100 ms late and blamed interrupt delivery; the cause was the container's
    CFS CPU quota (16 CPUs per 100 ms period on this pool): once a process has burnt the period's budget -- a torch CPU op waking
    a 128-thread pool does it in milliseconds, train.one_cpu_thread -- EVERY thread of it stalls until the next period, a thread
    blocked in hipEventSynchronize included.  The cure is not to burn the budget: this loop therefore yields the CPU between
    polls (a busy loop per rank is itself 1 CPU of the quota; eight ranks share one container), at a resolution of ~50 us."""
    import time
    evs = []
    for st in (streams or [torch.cuda.current_stream()]):
        e = torch.cuda.Event()
        e.record(st)
        evs.append(e)
    for e in evs:
        while not e.query():
            time.sleep(2e-5)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _chk(t, name='tensor'):
    if t.__dict__.get('_swem_planes_only'):
        raise _lib.SwemHipError('%s is a planes-only convolution output (ops.conv2d(planes_only=True)): its fp32 map was never '
                                'written; only a pre-split convolution may consume it' % name)
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise _lib.SwemHipError('%s must be a contiguous fp32 device tensor (got %s %s contiguous=%s)'
                                % (name, t.device, t.dtype, t.is_contiguous()))
    return t


def _hip_runtime():
    """The HIP runtime instance torch itself has mapped (ctypes handle)."""
    global _hip
    if _hip is None:
        path = 'libamdhip64.so'
        try:
            with open('/proc/self/maps') as f:
                for line in f:
                    if 'libamdhip64' in line:
                        path = line.split()[-1]
                        break
        except OSError:
            pass
        _hip = C.CDLL(path)
        _hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        _hip.hipStreamCreateWithFlags.restype = C.c_int
        _hip.hipStreamGetCaptureInfo.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
        _hip.hipStreamGetCaptureInfo.restype = C.c_int
    return _hip


def _capture_id(stream_ptr):
    """Id of the graph capture the stream is recording into, or None."""
    if not torch._C._cuda_isCurrentStreamCapturing():      # (the common case, without a ctypes round trip)
        return None
    status, cid = C.c_int(0), C.c_ulonglong(0)
    rc = _hip_runtime().hipStreamGetCaptureInfo(C.c_void_p(stream_ptr), C.byref(status), C.byref(cid))
    return cid.value if rc == 0 and status.value == 1 else None       # hipStreamCaptureStatusActive


_ws_capture = {}     # (capture id, device, stream) -> buffer allocated INSIDE that capture


def workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream): the library never allocates, and sequences that run
    concurrently on different streams must not share scratch.  While the stream is being captured into a HIP graph the
    buffer is allocated inside that capture (one per capture, device and stream): it then belongs to the graph's private
    pool and lives exactly as long as the graph.  A captured launch never sees a buffer of the eager cache (a later, larger
    eager request on that stream replaces and frees it) nor one of an earlier capture (its graph may be gone)."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    st = _stream()
    cid = _capture_id(st)
    if cid is None:
        cache, key = _ws, (dev, st)
    else:
        cache, key = _ws_capture, (cid, dev, st)
        if _ws_capture and next(iter(_ws_capture))[0] != cid:
            _ws_capture.clear()                # a new capture: the previous one's buffers stay with their graph
    buf = cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        cache[key] = buf
    return buf


_ctr = {}
_ctr_capture = {}
_ctr_all = []            # weak references to every counter buffer handed out (a wait fault zeroes them)
N_COUNTERS = 16384
FAULT_KSPLIT, FAULT_STREAMK, FAULT_RANGE = 1, 2, 4      # include/swem_hip.h, SWEM_FAULT_*
FAULT_BITS = {FAULT_KSPLIT: 'a K-split reducer gave up waiting for the other splits\' partial tiles (those output tiles are wrong; '
                            'the tile counters have been reset)',
              FAULT_STREAMK: 'a stream-K tile owner gave up waiting for a producer\'s partial tile (those output tiles are '
                             'wrong; the tile counters have been reset)',
              FAULT_RANGE: 'a value beyond the fp16 range (|x| >= 65520, inf or NaN) went into an fp16 operand pair of the f16x3 '
                           'arithmetic: everything computed from those planes is wrong, possibly FINITE (a ReLU epilogue maps the '
                           'resulting NaN to 0) -- re-run in a full-range arithmetic (PlanBook.to_full_range)'}
SwemRangeError = _lib.SwemRangeError


def counters(device):
    """Tile counters for the K-split / stream-K convolution launches of the current stream (include/swem_hip.h,
    swem_conv2d_nhwc_bf16x3_planes_ctr): a zero-initialised buffer per (device, stream) that the kernels leave all zero, so no
    memset launch precedes each of them.  Inside a graph capture the buffer belongs to that capture (like `workspace`): graphs
    captured on one stream may be replayed on different streams at the same time and must not share counters; its zero fill is
    one node at the head of the graph, replayed with it (which is why the fault word is NOT part of it: `fault_word`)."""
    import weakref
    dev = device.index if device.index is not None else torch.cuda.current_device()
    st = _stream()
    cid = _capture_id(st)
    if cid is None:
        cache, key = _ctr, (dev, st)
    else:
        cache, key = _ctr_capture, (cid, dev, st)
        if _ctr_capture and next(iter(_ctr_capture))[0] != cid:
            _ctr_capture.clear()               # a new capture: the previous one's buffer stays with its graph
    buf = cache.get(key)
    if buf is None:
        buf = cache[key] = torch.zeros(N_COUNTERS, dtype=torch.int32, device=device)
        _ctr_all[:] = [r for r in _ctr_all if r() is not None]
        _ctr_all.append(weakref.ref(buf))
    return buf


_fault = {}              # device index -> that device's sticky fault word (held for the life of the process)


def fault_word(device=None):
    """The device's sticky FAULT word (include/swem_hip.h, "Asynchronous faults"): ONE int32 per device, zero-initialised once,
    allocated outside any graph capture and never touched by a graph's memset nodes, so a fault raised inside replay k of a
    HIP graph is still there after replay k + 1 (as the last word of the per-capture counter buffer it was
    re-zeroed at the head of every replay and unreachable once a newer capture existed).  Kernels only ever OR bits into it;
    `check_faults` reads and clears it."""
    if device is None or device.index is None:
        dev = torch.cuda.current_device()
    else:
        dev = device.index
    t = _fault.get(dev)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.SwemHipError('ops.fault_word: the first launch on device %d falls inside a graph capture; call '
                                    'ops.fault_word(device) (or run one eager pass) before capturing' % dev)
        t = _fault[dev] = torch.zeros(1, dtype=torch.int32, device=torch.device('cuda', dev))
    return t


def _fault_ptr(device):
    return fault_word(device).data_ptr()


def _collect_faults():
    """Synchronise every device this process used, read AND clear its fault word (on a WAIT fault also every tile-counter
    buffer of that device: a stale counter would corrupt the next launch the same way); returns the OR of the words."""
    bits = 0
    for dev, t in _fault.items():
        torch.cuda.synchronize(dev)            # (every stream: a lane of a SequencePool may still be running)
        w = int(t.item())
        if not w:
            continue
        bits |= w
        t.zero_()
        if w & (FAULT_KSPLIT | FAULT_STREAMK):
            for b in (r() for r in _ctr_all):
                if b is not None and b.device.index == dev:
                    b.zero_()
        torch.cuda.synchronize(dev)
    return bits


def _fault_text(bits):
    what = '; '.join(t for b, t in FAULT_BITS.items() if bits & b)
    if bits & ~(FAULT_KSPLIT | FAULT_STREAMK | FAULT_RANGE):
        what += '; unknown fault bits %#x' % bits
    return what


def check_faults():
    """Asynchronous faults of the launches made so far on every device this process used (the C ABI's return codes only cover
    what is known at enqueue time).  Synchronises each device and reads its fault word: call it where the host waits anyway
    (the evaluator does at the end of every sequence, bench.py behind its timed regions, the trainer where it reads the
    loss).  On a fault the word is cleared, on a WAIT fault every tile-counter buffer of that device is zeroed too (a stale
    counter would corrupt the next launch the same way), and an exception is raised: SwemRangeError when the only fault is
    SWEM_FAULT_RANGE (the launches themselves were sound: re-run in a full-range arithmetic), else SwemHipError."""
    bits = _collect_faults()
    if bits:
        cls = SwemRangeError if bits == FAULT_RANGE else _lib.SwemHipError
        raise cls('asynchronous fault (fault word %#x): %s' % (bits, _fault_text(bits)))


# Ownership of the fault word.  The word is one per DEVICE; whoever reads it next would otherwise be blamed for
# whatever was left in it -- a validation sequence converting its model's book to the full-range arithmetic because a training
# step faulted ten steps earlier, while the trainer never learns.  So: an owner of launches drains the word when it takes the
# device over (`drain_faults` at the start of every evaluator loop / SequencePool.run) and collects its own faults where it ends
# (`check_faults`).  What a drain finds belongs to EARLIER work: it is handed to the long-lived owners that registered
# (`FAULT_OWNERS`: trainers, by weak reference -- `on_foreign_fault(bits)`), or, with nobody to take it, raised as what it is: a
# stale fault, not this caller's.
FAULT_OWNERS = []


def register_fault_owner(obj):
    import weakref
    FAULT_OWNERS[:] = [r for r in FAULT_OWNERS if r() is not None]
    FAULT_OWNERS.append(weakref.ref(obj))


def drain_faults(what):
    """Called by an owner BEFORE its first launch (synchronises): a set fault word is earlier work's -- see FAULT_OWNERS."""
    if not _fault:
        return
    bits = _collect_faults()
    if not bits:
        return
    owners = [o for o in (r() for r in FAULT_OWNERS) if o is not None]
    if not owners:
        raise _lib.SwemHipError('stale asynchronous fault (fault word %#x) found at the start of %s: it was raised by EARLIER work '
                                'on this device that never called ops.check_faults() -- that work\'s results are suspect, not this '
                                'call\'s: %s' % (bits, what, _fault_text(bits)))
    import warnings
    for o in owners:
        o.on_foreign_fault(bits)
    warnings.warn('swem_amd: %s found fault word %#x left by earlier work and handed it to %d registered owner(s) (trainers)'
                  % (what, bits, len(owners)), RuntimeWarning)


class ConvPack:
    """Weights of one conv in kernel layout: w [Cout'][KH][KW][Cin_pad] plus per-filter scale / shift."""

    def __init__(self, w, scale, shift, cout, kh, kw, stride, pad, glu=False, lazy_planes=False):
        self.w, self.scale, self.shift = w, scale, shift
        self.cout, self.kh, self.kw, self.stride, self.pad, self.glu = cout, kh, kw, stride, pad, glu
        self.cin = w.shape[-1]
        self.cin_true = self.cin          # channels of the reference conv (without layout padding)
        # names this layer in the fused-split hints (PlanBook.hints); unique per process unless built under pack_keys (never
        # id(self): a recycled address would inherit a dead layer's hints)
        self.site_key = _next_pack_key()
        co, kk = w.shape[0], w.shape[1] * w.shape[2] * w.shape[3]
        # the same filters as three bf16 planes, k/8-group major [K/8][Cout'][8] (bf16x6 math mode, pre-split form)
        # (the activation split kernel on the [Cout'][K] matrix: one launch; the training step re-packs every step)
        # the planes' K axis runs (ci / 32, ky, kx, ci % 32), not (ky, kx, ci): swem_conv2d_nhwc_bf16x3 walks the taps of
        # one 32-channel block back to back, so a tile's activations are fetched once instead of once per tap
        self._w3 = None
        self._w16 = None                  # (fp16 filter planes, scale with the planes' power-of-two column factors folded in)
        # the training step re-packs every filter every step: its packs make the fp16 planes in ONE launch
        # (swem_pack_filters_f16x2_f32: exponent bits instead of log2, otherwise the arithmetic of planes16 below)
        self.fast16 = False
        self.presplit_form = kk % 8 == 0 and self.cin % 32 == 0 and kh * kw <= 64     # (the pre-split kernel can take this layer)
        if self.presplit_form and not lazy_planes:
            self._make_w3()

    def _make_w3(self):
        wk = self._k_ordered()
        co, kk = wk.shape[0], wk[0].numel()
        self._w3 = torch.empty((3, co * kk), dtype=torch.bfloat16, device=wk.device)
        _lib.call('swem_split_bf16x3_f32', _stream(), wk.data_ptr(), self._w3.data_ptr(), co, kk, 0)

    @property
    def w3(self):
        """The three bf16 filter planes (None where the layer has no pre-split form).  A per-step pack of the training step
        (`lazy_planes`) builds them on first use: a layer whose plan is f16x3 never reads them."""
        if self._w3 is None and self.presplit_form:
            self._make_w3()
        return self._w3


    def _k_ordered(self):
        w = self.w
        co, khw = w.shape[0], w.shape[1] * w.shape[2]
        if khw > 1:
            return w.reshape(co, khw, self.cin // 32, 32).permute(0, 2, 1, 3).contiguous()
        return w

    def planes16(self):
        """(w16, scale16): the filters as the fp16 (hi, mid) pair of the f16x3 arithmetic (include/swem_hip.h,
        swem_split_f16x2_f32) and the epilogue scale that goes with them.  Every output column n is multiplied by 2^e[n] so that
        its largest weight lies in [2^13, 2^14) before the split -- conv weights are O(1e-2), and the `mid` term of a value below
        2^-2 would be a subnormal fp16 number -- and scale16[n] = scale[n] * 2^-e[n] undoes it in the epilogue (exact: powers of
        two).  Built on first use, once per pack."""
        if self._w16 is None:
            if not self.presplit_form:
                raise _lib.SwemHipError('this layer has no pre-split form (K %% 8, Cin %% 32, at most 64 taps)')
            wk = self._k_ordered()
            co, kk = wk.shape[0], wk[0].numel()
            if self.fast16:
                w16 = torch.empty((2, co * kk), dtype=torch.float16, device=wk.device)
                sc = torch.empty(co, dtype=torch.float32, device=wk.device)
                _lib.call('swem_pack_filters_f16x2_f32', _stream(), wk.data_ptr(), w16.data_ptr(), co, kk, _ptr(self.scale),
                          sc.data_ptr())
                self._w16 = (w16, sc)
                return self._w16
            amax = wk.reshape(co, kk).abs().amax(dim=1)
            e = torch.where(amax > 0, 13 - torch.floor(torch.log2(amax.clamp_min(1e-30))), torch.zeros_like(amax))
            # (log2 of a float just below a power of two may round up: the column then peaks in [2^12, 2^13), equally fine)
            f = torch.exp2(e.clamp(-100, 100))
            w16 = torch.empty((2, co * kk), dtype=torch.float16, device=wk.device)
            _lib.call('swem_split_f16x2_f32', _stream(), (wk.reshape(co, kk) * f[:, None]).contiguous().data_ptr(),
                      w16.data_ptr(), co, kk, 0, 0)      # (scaled into [2^13, 2^14): cannot leave the range)
            sc = (self.scale if self.scale is not None else torch.ones_like(f)) / f
            self._w16 = (w16, sc.contiguous())
        return self._w16


def pack_conv(weight, bias=None, bn=None, stride=1, pad=None, cin_pad=None, eps=1e-5, lazy_planes=False):
    """OIHW weight (+bias, + frozen BatchNorm (gamma, beta, mean, var)) -> ConvPack.
    BN folding follows ATen's eval-mode batch_norm: alpha = gamma/sqrt(var+eps), y = x*alpha + (beta - mean*alpha)."""
    co, ci, kh, kw = weight.shape
    w = weight.detach().float().permute(0, 2, 3, 1)
    cp = cin_pad if cin_pad is not None else (ci + 3) // 4 * 4
    if cp != ci:
        w = torch.nn.functional.pad(w, (0, cp - ci))
    w = w.contiguous()
    dev = weight.device
    scale = shift = None
    if bn is not None:
        g, b, m, v = [t.detach().float() for t in bn]
        alpha = g / torch.sqrt(v + eps)
        scale = alpha.contiguous()
        shift = b - m * alpha
        if bias is not None:
            shift = shift + bias.detach().float() * alpha
        shift = shift.contiguous()
    elif bias is not None:
        shift = bias.detach().float().contiguous()
    pk = ConvPack(w.to(dev), scale, shift, co, kh, kw, stride, kh // 2 if pad is None else pad, lazy_planes=lazy_planes)
    pk.cin_true = ci
    return pk


def pack_glu(wf, bf, wa, ba):
    """Two 3x3 convs (f, a) -> one GLU pack with filters grouped [Cout/32][f|a][32] (modules.py:13-26)."""
    co, ci, kh, kw = wf.shape
    assert co % 32 == 0 and ci % 4 == 0
    f = wf.detach().float().permute(0, 2, 3, 1).reshape(co // 32, 1, 32, kh, kw, ci)
    a = wa.detach().float().permute(0, 2, 3, 1).reshape(co // 32, 1, 32, kh, kw, ci)
    w = torch.cat([f, a], 1).reshape(2 * co, kh, kw, ci).contiguous()
    shift = torch.cat([bf.detach().float().reshape(co // 32, 1, 32), ba.detach().float().reshape(co // 32, 1, 32)],
                      1).reshape(2 * co).contiguous()
    return ConvPack(w, None, shift, co, kh, kw, 1, kh // 2, glu=True)


def _chk_src(t):
    """A conv source: fp32 device tensor (B,H,W,C) whose images are contiguous; the batch stride is free
    (match's mem_out keeps a row pitch per object)."""
    if t.__dict__.get('_swem_planes_only'):
        return t                           # (no fp32 map behind it: only its planes are read, conv2d checks that)
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t[0].is_contiguous()):
        raise _lib.SwemHipError('conv input must be an fp32 device tensor (B,H,W,C) with contiguous images')
    return t


def presplit(t, relu=False, nplanes=3):
    """bf16 planes, each [C/8][npix][8], of an NHWC fp32 activation with t = hi + mid + lo (of relu(t) if asked), computed
    once per tensor and cached on it: conv inputs are never modified after they are produced.  npix covers the tensor's
    storage range (a batch stride larger than one image, as match's mem_out has, is kept).  nplanes: how many of the three
    the caller reads (2 for a bf16x3 / plain-bf16 consumer; PLANES_F16: the fp16 (hi, mid) pair of an f16x3 consumer, its
    own cache entry.  In the producer's hint the LATEST request decides the format: a planes-only output has ONE consumer,
    which must find its format; a tensor with consumers of BOTH formats -- mixed tuned plans -- therefore settles on
    whichever asks last, and the other pays a split launch per frame: counted in `RESPLITS`, tools/split_sites.py lists the
    sites).  A producer that knows its consumers writes the planes itself
    (conv2d's epilogue, the frozen-BN stages of the training step): the request is recorded under the producer's site so
    that it can do so from the next frame / step on."""
    cache = t.__dict__.setdefault('_swem_split', {})
    if cache and t.__dict__.get('_swem_split_ver', t._version) != t._version:
        cache.clear()                      # the tensor was modified in place after its planes were made
    t.__dict__['_swem_split_ver'] = t._version
    f16 = nplanes == PLANES_F16
    key = _pkey(relu, nplanes)
    ent = cache.get(key)
    if ent is not None and f16 and t.__dict__.get('_swem_grad') and '_swem_inv' not in t.__dict__:
        # a gradient map whose fp16 pair was cached UNSCALED (a producer epilogue, a caller that split it before autograd marked
        # it): its consumers read the scale from `_swem_inv` -- make the scaled pair (this used to be a KeyError)
        ent = None
        cache.pop(key, None)
    site = t.__dict__.get('_swem_site')
    if site is not None and not _IN_TUNER[0]:
        # (the tuner's candidates do not count: a bf16x6 candidate that lost would leave the producer writing a third plane --
        # a quarter more plane bytes -- for a consumer that reads two)
        h = BOOK.hints.setdefault(site, {})
        cur = h.get(relu, 0)
        if cur < nplanes or (cur == PLANES_F16) != f16:
            # the producer of this tensor can write the planes itself next time: more bf16 planes than it writes now, or the
            # other format (the latest request decides: a planes-only output has ONE consumer, and it must find its format)
            h[relu] = nplanes
        BOOK.hint_epoch[site] = BOOK.epoch()   # ... and, while no plan changes, leave the fp32 map out (conv2d planes_only)
    if ent is None or (not f16 and ent[1] < nplanes):
        if t.__dict__.get('_swem_planes_only'):
            raise _lib.SwemHipError('presplit: a planes-only convolution output is asked for planes its producer did not write '
                                    '(relu=%s, plane code %d): it has more than the one consumer conv2d(planes_only=True) promises'
                                    % (relu, nplanes))
        B, H, W, Cc = t.shape
        if B > 1 and t.stride(0) % Cc:
            raise _lib.SwemHipError('presplit: batch stride must be a multiple of the channel count')
        if site is not None and cache and not _IN_TUNER[0]:
            # the producer DID write planes for this tensor, only not these: a consumer of the other format (or of more planes)
            # pays this launch every frame -- ADVICE r04: count it instead of paying it silently
            RESPLITS[site] = RESPLITS.get(site, 0) + 1
        npix = (B - 1) * (t.stride(0) // Cc) + H * W if B > 1 else H * W
        if f16 and t.__dict__.get('_swem_grad'):
            # a GRADIENT map (autograd marks them): the pair of t * 2^s, s chosen on the device from max |t|; the consumers
            # multiply by scratch[0] = 2^-s (include/swem_hip_train.h, swem_split_f16x2_scaled_f32)
            if relu:
                raise _lib.SwemHipError('presplit: a gradient map has no input ReLU')
            sp = torch.empty((2, npix * Cc), dtype=torch.float16, device=t.device)
            have = t.__dict__.get('_swem_amax')        # (scratch, nparts): block maxima the map's producer wrote (autograd._BNAct)
            scratch, nparts = have if have is not None else (torch.empty(AMAX_PARTS + 1, dtype=torch.float32, device=t.device), 0)
            _lib.call('swem_split_f16x2_scaled_f32', _stream(), t.data_ptr(), sp.data_ptr(), npix, Cc, scratch.data_ptr(), nparts,
                      _fault_ptr(t.device))
            t.__dict__['_swem_inv'] = scratch
            ent = cache[key] = (sp, PLANES_F16)
        elif f16:
            sp = torch.empty((2, npix * Cc), dtype=torch.float16, device=t.device)
            _lib.call('swem_split_f16x2_f32', _stream(), t.data_ptr(), sp.data_ptr(), npix, Cc, int(relu), _fault_ptr(t.device))
            ent = cache[key] = (sp, PLANES_F16)
        else:
            sp = torch.empty((3, npix * Cc), dtype=torch.bfloat16, device=t.device)
            _lib.call('swem_split_bf16x3_f32', _stream(), t.data_ptr(), sp.data_ptr(), npix, Cc, int(relu))
            ent = cache[key] = (sp, 3)
    return ent[0]


AMAX_PARTS = 256   # include/swem_hip_train.h, SWEM_AMAX_PARTS
# per-step packs (ConvPack.fast16: the training step's) that ran an f16x3 plan: their fp16 filter planes are built lazily, which
# inside a step would happen on ONE lane's stream while the other lanes read the shared pack -- autograd.new_step(prebuild=True)
# builds them with the pack, on the main stream, before the lanes fork
F16_PACK_SITES = set()
BF16_PACK_SITES = set()     # ... and the same for the bf16 planes (built lazily for those packs: ConvPack(lazy_planes=True))
RESPLITS = {}      # producer site -> split launches made for a tensor that already carried producer-written planes
FLOPS = None        # a dict while somebody counts useful FLOPs (ops.flags(FLOPS={})): conv2d, autograd._wgrad / _Memorize / _Match add to it
# The decoder's two skip convolutions (networks.py:190-196: UpsampleBlock.skip_conv on s8 / s4) read the KEY encoder's features only:
# the same for every object (round 2: computed once per frame) and independent of the memory.  With this switch (default on;
# SWEM_SKIP_IN_KEY_PASS=0) Engine.encode_key computes them right behind the trunk and hands them on with s8 / s4 -- in the look-ahead
# graphs that moves 0.2 ms per frame of B = 1 launches out of the memory-dependent frame chain into the batched key-encoder pass
# (ten frames per launch, on the side stream); Engine.decoder_logit computes them itself whenever the s8 / s4 it is given do not carry
# them (tensors that did not come from this engine's encode_key).  Same kernels on the same data: results unchanged.
SKIP_IN_KEY_PASS = os.environ.get('SWEM_SKIP_IN_KEY_PASS', '1') != '0'


def _pkey(relu, npl):
    """Key of a tensor's plane cache (`_swem_split`): relu (False / True = 0 / 1) for bf16 planes, 2 + relu for the fp16 pair."""
    return int(bool(relu)) + (2 if npl == PLANES_F16 else 0)


def _new_planes(npl, numel, device):
    """Storage for a producer-written plane set: (3, numel) bf16, or (2, numel) fp16 for PLANES_F16."""
    if npl == PLANES_F16:
        return torch.empty((2, numel), dtype=torch.float16, device=device)
    return torch.empty((3, numel), dtype=torch.bfloat16, device=device)


def _keyed(planes):
    """{relu: (tensor, npl)} as a producer collected it -> the `_swem_split` cache of its output."""
    return {_pkey(r, e[1]): e for r, e in planes.items()}


def batch_item(t, j, n=1):
    """Items j .. j + n - 1 of a batched NHWC activation as an (n, H, W, C) view that keeps what the batch carries: the bf16
    planes a producing kernel wrote (planes are [plane][C/8][pixel][8] over ALL pixels of the batch: the items are the pixel
    range [j*H*W, (j+n)*H*W) of every channel group, i.e. the same planes from an offset base with the same strides) and the
    producer's site, so that a consumer's split request is still reported to the producer."""
    v = t[j:j + n]
    d = t.__dict__
    sp = d.get('_swem_split')
    if sp and d.get('_swem_split_ver', t._version) == t._version and (t.is_contiguous() or d.get('_swem_planes_only')):
        off = j * t.shape[1] * t.shape[2] * 8
        v.__dict__['_swem_split'] = {relu: (planes[:, off:], npl) for relu, (planes, npl) in sp.items()}
        v.__dict__['_swem_split_ver'] = v._version
    if '_swem_site' in d:
        v.__dict__['_swem_site'] = d['_swem_site']
    if d.get('_swem_planes_only'):
        v.__dict__['_swem_planes_only'] = True
    if d.get('_swem_nonneg', -1) == t._version:
        v.__dict__['_swem_nonneg'] = v._version
    sk = d.get('_swem_skip')              # (the decoder's skip convolution of this feature map, computed in the key pass)
    if sk is not None and sk[1] == t._version:
        v.__dict__['_swem_skip'] = (batch_item(sk[0], j, n), v._version, sk[2])
    return v


DGRAD, DGRAD_EH, DGRAD_EW, MASK_POS = 8, 16, 32, 64
_WSB = {}      # conv workspace bytes by (shape, plan)
_NAN = {}


def _nan_cell(device):
    """One NaN per device, made once outside any graph capture (a fill inside a capture would be a node of that graph and live
    in its pool); None while the first request falls into a capture -- the caller then allocates an ordinary tensor."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    t = _NAN.get(dev)
    if t is None and not torch.cuda.is_current_stream_capturing():
        t = _NAN[dev] = torch.full((1,), float('nan'), dtype=torch.float32, device=device)
    return t


def conv2d(srcs, pack, relu_in=False, relu_out=False, residual=None, res_broadcast=False, batch=None, out=None,
           plan=None, dgrad=None, mask=None, planes_only=False):
    """srcs: list of up to three NHWC tensors concatenated on C; a source with batch 1 is broadcast over `batch`.
    plan: explicit plan hint (include/swem_hip.h); default = tuned plan of this layer shape, else the heuristic.
    dgrad=(H, W): data-gradient mode (SWEM_CONV_DGRAD): srcs = [dY], pack = the transposed filters, the result has the
    forward input's size H x W.  mask: tensor of the output's shape; the result is zeroed where mask <= 0.
    planes_only: the caller promises that the ONLY consumer of the result is one pre-split convolution (conv1 -> conv2 -> conv3
    inside a ResNet block, conv1 -> conv2 of a ResBlock).  Once that consumer has asked for the planes (BOOK.hints, from the
    second frame on) the fp32 map is not written at all -- half the output bytes of such a layer, which is what bounds the
    64-channel and 1x1 layers -- and the returned tensor only carries the planes; any other use of it raises.
    planes_only='block' (round 4): the result is a ResNet block's output inside a stage -- its consumers are the next block's
    convolutions (planes, without an input ReLU) AND the next block's residual add (mod_resnet.py:77-113).  The map is left out
    once the convolution that adds it has also said, for the current plans, that it reads the addend from the planes
    (BOOK.res_epoch): a third of the bytes of the byte-bound 1x1 expansion layers.  `residual` may then be such a tensor."""
    x0 = _chk_src(srcs[0])
    B = batch if batch is not None else max(s.shape[0] for s in srcs)
    _, H, W, _ = x0.shape
    args = []
    cin = 0
    for s in srcs:
        _chk_src(s)
        if s.shape[1] != H or s.shape[2] != W:
            raise _lib.SwemHipError('conv2d: sources differ in spatial size')
        bs = 0 if (s.shape[0] == 1 and B > 1) else (s.stride(0) if s.shape[0] > 1 else H * W * s.shape[3])
        if s.__dict__.get('_swem_planes_only') and s.shape[0] > 1:
            bs = H * W * s.shape[3]        # (the stand-in tensor of a planes-only output has no strides of its own)
        args += [s.data_ptr(), s.shape[3], bs]
        cin += s.shape[3]
    for _ in range(3 - len(srcs)):
        args += [0, 0, 0]
    if cin != pack.cin:
        raise _lib.SwemHipError('conv2d: input has %d channels, pack expects %d' % (cin, pack.cin))
    Ho = (H + 2 * pack.pad - pack.kh) // pack.stride + 1
    Wo = (W + 2 * pack.pad - pack.kw) // pack.stride + 1
    flags = (RELU_IN if relu_in else 0) | (RELU_OUT if relu_out else 0) | (GLU if pack.glu else 0)
    if dgrad is not None:
        Ho, Wo = dgrad
        eh = Ho - ((H - 1) * pack.stride + pack.kh - 2 * pack.pad)
        ew = Wo - ((W - 1) * pack.stride + pack.kw - 2 * pack.pad)
        if eh not in (0, 1) or ew not in (0, 1):
            raise _lib.SwemHipError('conv2d dgrad: %dx%d is not an input size of this %dx%d output' % (Ho, Wo, H, W))
        flags |= DGRAD | (DGRAD_EH if eh else 0) | (DGRAD_EW if ew else 0)
    if mask is not None:
        if residual is not None:
            raise _lib.SwemHipError('conv2d: mask and residual share the res operand')
        residual, flags = mask, flags | MASK_POS
    y = out
    res_bs = 0
    res_planes = None          # (planes tensor, plane code) of a planes-only residual
    if residual is not None:
        if residual.__dict__.get('_swem_planes_only'):
            ent = None
            for npl_ in (PLANES_F16, 3):          # (two bf16 planes carry 16 bits: not an addend)
                e_ = residual.__dict__.get('_swem_split', {}).get(_pkey(False, npl_))
                if e_ is not None and (npl_ == PLANES_F16 or e_[1] == 3):
                    ent = (e_[0], npl_)
                    break
            if ent is None or mask is not None or pack.glu:
                raise _lib.SwemHipError('conv2d: the residual is a planes-only block output without planes an addend can be read '
                                        'from (an fp16 pair or three bf16 planes), or this call cannot take a plane residual')
            res_planes = ent
        else:
            _chk(residual, 'conv residual')
        res_bs = 0 if (res_broadcast or (residual.shape[0] == 1 and B > 1)) else Ho * Wo * pack.cout

    pipe_ok = all(s_.shape[3] % 32 == 0 for s_ in srcs)      # (the register-staged kernels' condition, conv.hip)
    presplit_ok = pack.presplit_form and pipe_ok

    # the output's own bf16 planes, if the convolutions that consumed this layer's output on an earlier frame split it:
    # the epilogue writes them (fused operand split: no split launch, no re-read of y)
    site = ('conv', pack.site_key, B, H, W, flags)
    want = BOOK.hints.get(site) if (FUSE_SPLIT and dgrad is None and pack.cout % 8 == 0) else None
    planes = {}
    skip_y = bool(planes_only and want and out is None and PLANES_ONLY and BOOK.hint_epoch.get(site) == BOOK.epoch())
    if skip_y and planes_only == 'block':
        # ... and the adding convolution reads planes, and planes of the values themselves (no input ReLU) in a format an
        # addend can come from are among those this launch writes
        # (fp16 pair only: from three bf16 planes the addend costs 6 bytes per element against the map's 4, and the exact-split
        # leg measured 4 % SLOWER with it -- the C ABI takes them, this policy does not use them)
        skip_y = BOOK.res_epoch.get(site) == BOOK.epoch() and want.get(False) == PLANES_F16
    if y is None:
        # a planes-only output has no fp32 map at all: the tensor that carries its planes is one NaN expanded to the shape
        # (no allocation of the map; anything that reads it by accident sees NaN, _chk / _chk_src refuse it by its flag)
        nan1 = _nan_cell(x0.device) if skip_y else None
        y = (nan1.expand(B, Ho, Wo, pack.cout) if nan1 is not None
             else torch.empty((B, Ho, Wo, pack.cout), dtype=torch.float32, device=x0.device))
    y_ptr = 0 if skip_y else y.data_ptr()

    def launch(plan, fresh=False):
        wkey = (B, H, W, cin, pack.cout, pack.kh, pack.kw, pack.stride, pack.pad, flags, plan)
        wsb = _WSB.get(wkey)
        if wsb is None:                    # (a pure function of the shape and the plan: asked once, not per launch)
            wsb = _WSB[wkey] = _lib.query('swem_conv2d_workspace', *wkey)
        ws = workspace(wsb, x0.device) if wsb else None
        pargs = [0, 3, 0, 3]
        if want:
            for relu_v, npl in want.items():
                sp = planes.get(relu_v)
                if sp is None:
                    sp = planes[relu_v] = (_new_planes(npl, B * Ho * Wo * pack.cout, x0.device), npl)
                pargs[2 * int(relu_v)], pargs[2 * int(relu_v) + 1] = sp[0].data_ptr(), npl
        if (plan >> 16) & 3 and presplit_ok:
            # bf16 / fp16 math: sources split once per tensor (input ReLU folded into the split), filters split at pack time
            f16 = (plan >> 16) & 7 == 7
            need = 3 if (plan >> 16) & 3 == 1 else (PLANES_F16 if f16 else 2)
            w3, scale = pack.planes16() if f16 else (pack.w3, pack.scale)
            if pack.fast16 and not _IN_TUNER[0]:
                # (the training step pre-builds the planes its packs' plans read: autograd.new_step)
                (F16_PACK_SITES if f16 else BF16_PACK_SITES).add(pack.site_key)
            sargs = []
            for i, s_ in enumerate(srcs):
                # (tuning charges a candidate the split of its inputs -- except inputs a conv epilogue produces: those arrive
                # with their planes from the second frame on, FUSE_SPLIT)
                if fresh and not (FUSE_SPLIT and s_.__dict__.get('_swem_site', (None,))[0] in ('conv', 'upsample_add', 'prep_s2d')):
                    s_.__dict__.pop('_swem_split', None)
                sp = presplit(s_, relu_in, need)
                sargs += [sp.data_ptr(), s_.shape[3], args[3 * i + 2], sp.stride(0)]
                if f16 and s_.__dict__.get('_swem_grad'):
                    # the planes hold dY * 2^s (presplit): the epilogue scale takes the 2^-s (device side: graph-safe)
                    if len(srcs) != 1:
                        raise _lib.SwemHipError('conv2d: a scaled gradient map is the only source of its data-gradient convolution')
                    ncol = pack.cout * (2 if pack.glu else 1)
                    sc_ = torch.empty(ncol, dtype=torch.float32, device=x0.device)
                    _lib.call('swem_vec_scale_f32', _stream(), _ptr(scale), s_.__dict__['_swem_inv'].data_ptr(), sc_.data_ptr(), ncol)
                    scale = sc_
            for _ in range(3 - len(srcs)):
                sargs += [0, 0, 0, 0]
            ctr = counters(x0.device)
            if res_planes is not None:
                rp, rnpl = res_planes
                _lib.call('swem_conv2d_nhwc_bf16x3_planes_res', _stream(), *sargs, B, H, W, w3.data_ptr(), _ptr(scale),
                          _ptr(pack.shift), rp.data_ptr(), rp.stride(0), rp.stride(0) // pack.cout, rnpl, res_bs, y_ptr,
                          pack.cout, pack.kh, pack.kw, pack.stride, pack.pad, flags & ~RELU_IN, plan, _ptr(ws), wsb, *pargs,
                          _ptr(ctr), 0 if ctr is None else ctr.numel(), _fault_ptr(x0.device))
                return
            _lib.call('swem_conv2d_nhwc_bf16x3_planes_ctr', _stream(), *sargs, B, H, W, w3.data_ptr(), _ptr(scale),
                      _ptr(pack.shift), _ptr(residual), res_bs, y_ptr, pack.cout, pack.kh, pack.kw,
                      pack.stride, pack.pad, flags & ~RELU_IN, plan, _ptr(ws), wsb, *pargs, _ptr(ctr),
                      0 if ctr is None else ctr.numel(), _fault_ptr(x0.device))
            return
        if res_planes is not None or any(s_.__dict__.get('_swem_planes_only') for s_ in srcs):
            raise _lib.SwemHipError('conv2d: a planes-only source or residual reached a convolution that reads the fp32 map (plan %#x)' % plan)
        _lib.call('swem_conv2d_nhwc_f32_planes', _stream(), *args, B, H, W, pack.w.data_ptr(), 0, _ptr(pack.scale),
                  _ptr(pack.shift), _ptr(residual), res_bs, y_ptr, pack.cout, pack.kh, pack.kw, pack.stride,
                  pack.pad, flags, plan, _ptr(ws), wsb, *pargs, _fault_ptr(x0.device))

    sig = (cin, pack.cout, pack.kh, pack.kw, pack.stride, pack.pad, flags, B, H, W) + _PLAN_TAG
    explicit = plan is not None
    if not explicit:
        plan = BOOK.conv.get(sig)
        if plan is None:
            # a shape nobody tuned: under conv_math((m,)) the heuristic tile in math mode m; else the book's fallback (a model's
            # book: MODEL_FALLBACK, the heuristic tile in f16x3; the free-standing default book: 0, the exact fp32 kernels)
            plan = _PLAN_TAG[1] << 16 if (len(_PLAN_TAG) == 2 and not AUTOTUNE) else BOOK.fallback
            if _PLAN_TAG and (plan >> 16) & 7 not in CONV_MATH_MODES:
                plan = (plan & 0xffff) | max(CONV_MATH_MODES) << 16    # (a restricted block: its most capable allowed mode)
            if BOOK.full_range:
                plan = PlanBook._plan_full_range(plan)                 # (whatever the block asks for: no fp16 / 16-bit operands)
            if AUTOTUNE and plan & 0xffff == 0 and not torch.cuda.is_current_stream_capturing():
                # (a fallback that names a tile is a decision -- batch-invariant plans -- and is not tuned over)
                plan = BOOK.conv[sig] = _autotune(launch, B * Ho * Wo, pack.cout * (2 if pack.glu else 1),
                                                    -(-pack.kh * pack.kw * cin // 32), pack.glu, fresh_kw=True, t256=presplit_ok)
    if residual is not None and mask is None and not _IN_TUNER[0]:
        rsite = residual.__dict__.get('_swem_site')
        if rsite is not None:
            # (this convolution adds a tensor some producer made: tell that producer whether the addend may come from planes --
            # it may when this launch runs the pre-split kernel, which is the only one with that path)
            BOOK.res_epoch[rsite] = BOOK.epoch() if ((plan >> 16) & 3 and presplit_ok and not pack.glu) else None
    if CONV_TRACE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if FLOPS is not None and not _IN_TUNER[0]:
        # useful multiply-adds x 2 of this launch (unpadded channels; a data gradient has the forward layer's count: every
        # (output pixel, filter tap) pair once) -- tools/train_bench.py's roofline accounting
        if dgrad is None:
            fl = 2.0 * B * Ho * Wo * pack.cout * (2 if pack.glu else 1) * pack.kh * pack.kw * getattr(pack, 'cin_true', pack.cin)
        else:
            fl = 2.0 * B * H * W * pack.cin * pack.kh * pack.kw * pack.cout
        k_ = 'conv_dgrad' if dgrad is not None else 'conv_fwd'
        FLOPS[k_] = FLOPS.get(k_, 0.0) + fl
        FLOPS['conv_launches'] = FLOPS.get('conv_launches', 0) + 1
    launch(plan)
    if MATH_RAN is not None:
        m_ = (plan >> 16) & 7
        m_ = m_ if m_ == 7 else m_ & 3
        if not presplit_ok:                # (what the library runs on the fp32 entry point: conv.hip, `emulate`)
            m_ = 1 if (m_ & 1 and pipe_ok) else 0
        MATH_RAN[m_] = MATH_RAN.get(m_, 0) + 1
    if out is None:
        y.__dict__['_swem_site'] = site
        if planes:
            y.__dict__['_swem_split'] = _keyed(planes)
            y.__dict__['_swem_split_ver'] = y._version
        if skip_y:
            y.__dict__['_swem_planes_only'] = True
    if CONV_TRACE is not None:
        e1.record()
        ncols = pack.cout * (2 if pack.glu else 1)
        in_bytes = 4.0 * sum(s_.shape[0] * H * W * s_.shape[3] for s_ in srcs)
        # (events, useful FLOPs, label, algorithmic bytes, plan, pipe: 'bf16' = six bf16-MFMA products per fp32 product,
        # 'bf16x3' = three, 'fp32' = v_mfma_f32_32x32x2_f32)
        CONV_TRACE.append((e0, e1, 2.0 * B * Ho * Wo * ncols * pack.kh * pack.kw * pack.cin_true,
                           '%dx%dx%d k%d s%d %d->%d' % (B, H, W, pack.kh, pack.stride, pack.cin_true, ncols),
                           in_bytes + 4.0 * ncols * pack.kh * pack.kw * pack.cin_true + 4.0 * B * Ho * Wo * pack.cout,
                           plan, ('f16x3' if (plan >> 16) & 7 == 7 and presplit_ok else
                                  'bf16x3' if (plan >> 16) & 3 == 3 and presplit_ok else
                                  'bf16' if ((plan >> 16) & 3 and (presplit_ok or ((plan >> 16) & 1 and pipe_ok))) else 'fp32')))
    return y


_PLAN_TAG = ()

# The identity bottleneck blocks of the key encoder's layer1 as ONE launch (include/swem_hip.h, swem_bottleneck_f16x3) wherever the
# book runs all three of the block's convolutions in f16x3.  OFF by default (SWEM_FUSE_BOTTLENECK=1 / ops.flags(FUSE_BOTTLENECK=
# True) turn it on): measured in round 5 (profiles/r05_bottleneck_fusion.txt) the fused block is 1.35 x the three launches for one
# frame and 1.08 x for the ten-frame batch the look-ahead graphs run -- below the 1.4 x bar VERDICT r04 item 6 set for shipping it --
# and the frame rate does not move (468 against 467 frames/s with four sequences, 387.7 against 387.6 with one): with the 64-channel
# intermediates gone the block is bound by what is left, its 256-channel input (read once more as the identity, and 1.4 x for the
# 3x3's halo) and output, at the memory system's ~5 TB/s.
FUSE_BOTTLENECK = os.environ.get('SWEM_FUSE_BOTTLENECK', '0') == '1'


def _plan_of(pack, flags, B, H, W):
    """The plan conv2d would run this layer with under the current book / conv_math block (no tuning)."""
    sig = (pack.cin, pack.cout, pack.kh, pack.kw, pack.stride, pack.pad, flags, B, H, W) + _PLAN_TAG
    plan = BOOK.conv.get(sig)
    if plan is None:
        plan = _PLAN_TAG[1] << 16 if len(_PLAN_TAG) == 2 else BOOK.fallback
        if _PLAN_TAG and (plan >> 16) & 7 not in CONV_MATH_MODES:
            plan = (plan & 0xffff) | max(CONV_MATH_MODES) << 16
    return plan


def bottleneck_ok(x, c1, c2, c3):
    """Whether `bottleneck` can stand in for conv1 -> conv2 -> conv3 (+ identity) of this block: the layer1 geometry
    (256 -> 64 -> 64 -> 256, stride 1, folded BatchNorm on every convolution) and all three layers in f16x3 under the current
    book (tuned plans or its fallback) -- a book on the exact / bf16 arithmetics keeps the three launches, as does the tuner."""
    if not FUSE_BOTTLENECK or AUTOTUNE or _IN_TUNER[0] or x.dim() != 4 or x.shape[3] != 256:
        return False
    geo = ((c1, 256, 64, 1, 0), (c2, 64, 64, 3, 1), (c3, 64, 256, 1, 0))
    for pk, ci, co, k, pad in geo:
        if (pk.cin, pk.cout, pk.kh, pk.kw, pk.stride, pk.pad, pk.glu) != (ci, co, k, k, 1, pad, False) or not pk.presplit_form \
                or pk.scale is None or pk.shift is None:
            return False
    B, H, W, _ = x.shape
    if B * H * W * 16 >= 1 << 32:
        return False
    return all((_plan_of(pk, RELU_OUT, B, H, W) >> 16) & 7 == 7 for pk, *_ in geo)


def bottleneck(x, c1, c2, c3, planes_only=False):
    """relu(bn3(conv1x1(relu(bn2(conv3x3(relu(bn1(conv1x1(x)))))))) + x) for an identity bottleneck block (mod_resnet.py:77-113)
    in one launch; x NHWC (B,H,W,256), possibly a planes-only block output.  The result carries its site and -- once its consumers
    have asked for the fp16 pair -- its planes; planes_only='block' as conv2d: inside a stage the fp32 map is left out when every
    consumer reads the planes (the next block's convolutions and its identity, which this kernel reads from the planes too)."""
    B, H, W, Cc = x.shape
    xp = presplit(x, False, PLANES_F16)                 # (2, ...) fp16: the block's input AND its identity
    xsite = x.__dict__.get('_swem_site')
    if xsite is not None and not _IN_TUNER[0]:
        BOOK.res_epoch[xsite] = BOOK.epoch()             # (this block reads its identity from the planes)
    site = ('bneck', c3.site_key, B, H, W)
    want = BOOK.hints.get(site) if FUSE_SPLIT else None
    f16_only = bool(want) and set(want.items()) == {(False, PLANES_F16)}
    skip_y = bool(planes_only and f16_only and PLANES_ONLY and BOOK.hint_epoch.get(site) == BOOK.epoch()
                  and (planes_only != 'block' or BOOK.res_epoch.get(site) == BOOK.epoch()))
    nan1 = _nan_cell(x.device) if skip_y else None
    if skip_y and nan1 is None:
        skip_y = False
    y = nan1.expand(B, H, W, Cc) if skip_y else torch.empty((B, H, W, Cc), dtype=torch.float32, device=x.device)
    yp = _new_planes(PLANES_F16, B * H * W * Cc, x.device) if (want and want.get(False) == PLANES_F16) else None
    if CONV_TRACE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    (w1, s1), (w2, s2), (w3, s3) = c1.planes16(), c2.planes16(), c3.planes16()
    _lib.call('swem_bottleneck_f16x3', _stream(), xp.data_ptr(), xp.stride(0), B, H, W, Cc, w1.data_ptr(), s1.data_ptr(),
              c1.shift.data_ptr(), w2.data_ptr(), s2.data_ptr(), c2.shift.data_ptr(), w3.data_ptr(), s3.data_ptr(),
              c3.shift.data_ptr(), 0 if skip_y else y.data_ptr(), _ptr(yp), 0 if yp is None else yp.stride(0),
              _fault_ptr(x.device))
    if MATH_RAN is not None:
        MATH_RAN[7] = MATH_RAN.get(7, 0) + 1
    y.__dict__['_swem_site'] = site
    if yp is not None:
        y.__dict__['_swem_split'] = {_pkey(False, PLANES_F16): (yp, PLANES_F16)}
        y.__dict__['_swem_split_ver'] = y._version
    if skip_y:
        y.__dict__['_swem_planes_only'] = True
    if CONV_TRACE is not None:
        e1.record()
        CONV_TRACE.append((e0, e1, 2.0 * B * H * W * (256 * 64 + 9 * 64 * 64 + 64 * 256),
                           'bneck %dx%dx%d 256->64->64->256' % (B, H, W), 8.0 * B * H * W * Cc + 4.0 * (2 * 256 * 64 + 9 * 64 * 64),
                           7 << 16, 'f16x3'))
    return y


class conv_math:
    """Context: restrict the math modes the conv tuner may choose (0 fp32 MFMA, 1 bf16x6, 2 plain bf16) and keep the plans
    tuned under it apart from the default ones.  The training step uses (2,) for config.AMP."""

    def __init__(self, modes):
        self.modes = tuple(modes)

    def __enter__(self):
        global CONV_MATH_MODES, _PLAN_TAG
        self.saved = (CONV_MATH_MODES, _PLAN_TAG)
        CONV_MATH_MODES, _PLAN_TAG = self.modes, ('math',) + self.modes
        _MODE_GEN[0] += 1

    def __exit__(self, *a):
        global CONV_MATH_MODES, _PLAN_TAG
        CONV_MATH_MODES, _PLAN_TAG = self.saved
        _MODE_GEN[0] += 1


def AUTOTUNE_PENDING():
    """True while the on-device tuner may still run (it must not run inside a graph capture)."""
    return bool(AUTOTUNE)


def save_plans(path, book=None):
    """Persist the tuned plans of `book` (default: the current one; profiling runs reload them instead of re-tuning)."""
    (book or BOOK).save(path)


def load_plans(path, book=None):
    return (book or BOOK).load(path)


def _autotune(launch, M, ncols, nkb, glu, reps=3, fresh_kw=False, modes=None, t256=True):
    """Time candidate (wave tile, K-split, math mode) plans for one layer shape; return the fastest as a plan hint.
    fresh_kw: the launcher takes fresh=True to re-split its inputs every time (the split cost is then part of the
    bf16x6 candidates' time, as if no other layer shared the input)."""
    if modes is None:
        modes = CONV_MATH_MODES
    if BOOK.full_range:
        # a book that left the fp16 range stays out of it: no f16x3 (7) and no 16-operand-bit bf16x3 (3) candidate (ADVICE r05:
        # with the tuner on they were offered again, and a second range fault hits range_fallback's "cannot happen" re-raise)
        modes = tuple(m_ for m_ in modes if m_ not in (7, 3)) or (1,)
    cands = [0]
    for wm, wn in _TUNE_TILES:
        if (glu and wn != 2) or (wn == 2 and ncols < 128):
            continue
        blocks = -(-M // (64 * wm)) * -(-ncols // (64 * wn))
        for ns in _TUNE_SPLITS:
            if ns > 1 and (nkb // ns < 2 or blocks * ns > 4096):
                continue
            for math in modes:
                if (wm, wn) == (2, 1) and (math == 0 or ncols > 64):
                    continue                       # the 128x64 tile: where a 64-wide N leaves nothing else to widen
                cands.append(wm | wn << 4 | ns << 8 | math << 16)
                if math in (1, 2, 3, 7):           # pre-split kernel variants: other stage count, 8-wave 128x128 tile
                    base = wm | wn << 4 | ns << 8 | math << 16
                    cands.append(base | 1 << 20)
                    cands.append(base | 4 << 20)              # 16x16x32 MFMA shape
                    if math != 1:                             # four-stage rings (one or two planes only)
                        cands.append(base | 10 << 20)
                        cands.append(base | 11 << 20)
                    if wm == 2 and wn == 2:
                        cands.append(base | 2 << 20)
                        cands.append(base | 6 << 20)
                        cands.append(base | 8 << 20)          # 16-k blocks: three blocks of four waves per CU
                        cands.append(base | 9 << 20)          # ... with three LDS stages (two blocks per CU)
                        cands.append(base | 14 << 20)         # eight waves, 16x16x32 MFMA, three stages
                        if math != 1 and not TUNE_ROUND3_FORMS:
                            cands.append(base | 12 << 20)
                            cands.append(base | 13 << 20)
                        elif math != 1:
                            cands.append(base | 12 << 20)     # eight waves, four stages
                            cands.append(base | 13 << 20)     # ... on the 16x16x32 MFMA
                            cands.append(base | 5 << 20)      # prefetched fragments: four waves of 64x64, two stages
                            cands.append(base | 15 << 20)     # ... three stages (one block per CU)
                            cands.append(base | 7 << 20)      # ... eight waves of 32x64, four stages
                            if ns == 1 and nkb >= 16 and math != 7:   # stream-K (plan bits 24-27 = 1): persistent workers, equal shares
                                cands.append(base | 6 << 20 | 1 << 24)
                                cands.append(base | 5 << 20 | 1 << 24)
                    if ns == 1 and blocks > 256 and nkb >= 16:   # tail split: the last, partly filled round over K
                        for ts in (4, 8):
                            cands.append(base | ts << 24)
                            if wm == 2 and wn == 2:
                                cands.append(base | 2 << 20 | ts << 24)
                                cands.append(base | 8 << 20 | ts << 24)
                                if math != 1 and TUNE_ROUND3_FORMS:
                                    cands.append(base | 5 << 20 | ts << 24)
    if t256 and 7 in modes and TUNE_T256 and ncols >= 192:
        # the 256-column tile of conv_t256_kernel (f16x3 only; one block per CU): tile heights 128 .. 256 rows (plan bits
        # 20-23 = rows / 32, 0 = 256: the only GLU form), K-split so that the tiles fill the 256 CUs about once
        for v in ((0,) if glu else (0, 4, 5, 6, 7)):
            rows = 32 * v if v else 256
            tiles = -(-M // rows) * -(-ncols // 256)
            for ns in sorted({1, max(1, min(nkb // 4, 256 // tiles)), max(1, min(nkb // 4, -(-256 // tiles)))}):
                cands.append(4 | 4 << 4 | ns << 8 | 7 << 16 | v << 20)
    if t256 and 1 in modes and TUNE_T256 and ncols >= 192 and not glu:
        # ... and its bf16x6 form (three planes: 128-row tiles only, plan bits 20-23 = 4)
        tiles = -(-M // 128) * -(-ncols // 256)
        for ns in sorted({1, max(1, min(nkb // 4, 256 // tiles)), max(1, min(nkb // 4, -(-256 // tiles)))}):
            cands.append(4 | 4 << 4 | ns << 8 | 1 << 16 | 4 << 20)

    def timed(plan, n):
        launch(plan)                               # warm (also grows the workspace)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        # a short spin kernel holds the queue while the host enqueues the n launches: the interval is then GPU time between
        # back-to-back packets -- with an empty queue a 15 us layer measures the host's ~10 us per Python launch instead
        torch.cuda._sleep(150_000 + 40_000 * n)
        e0.record()
        for _ in range(n):
            launch(plan, True) if fresh_kw else launch(plan)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n
    _IN_TUNER[0] += 1
    try:
        return _autotune_pick(cands, timed, reps)
    finally:
        _IN_TUNER[0] -= 1


_IN_TUNER = [0]


def _autotune_pick(cands, timed, reps):
    first = sorted((timed(plan, reps), plan) for plan in cands)
    # the candidates within 15 % of the fastest (at most four) are timed again: three interleaved rounds, the best round of
    # each counts (a round disturbed by another stream's kernels or a clock step does not decide a near tie; a plan must be
    # 1 % faster than the first pass's winner to replace it)
    short = [pl for t, pl in first[:4] if t <= 1.15 * first[0][0]]
    if len(short) == 1:
        return short[0]
    best = {pl: float('inf') for pl in short}
    for _ in range(3):
        for pl in short:
            best[pl] = min(best[pl], timed(pl, 2 * reps))
    lead = short[0]
    win = min(short, key=lambda pl: best[pl])
    return win if best[win] < 0.99 * best[lead] else lead


def _f3(t):
    v = [float(x) for x in t.detach().flatten().cpu().tolist()]
    return (C.c_float * 3)(*v)


def prep_key_input(frames, mean3, std3, out=None):
    """frames NCHW (B,3,H,W) -> normalised NHWC (B,H,W,4); mean3/std3 are ctypes float[3].  out: a (B,H,W,4) slice to fill."""
    _chk(frames, 'frames')
    B, _, H, W = frames.shape
    if out is None:
        out = torch.empty((B, H, W, 4), dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != (B, H, W, 4) or not out.is_contiguous():
        raise _lib.SwemHipError('prep_key_input: out must be a contiguous (B,H,W,4) tensor')
    _lib.call('swem_prep_key_input_f32', _stream(), frames.data_ptr(), C.addressof(mean3), C.addressof(std3),
              out.data_ptr(), B, H, W)
    return out


def prep_value_input(frame, masks, mean3, std3, single_obj):
    _chk(frame, 'frame')
    _chk(masks, 'masks')
    B, _, H, W = frame.shape
    N = masks.shape[1] - 1
    out = torch.empty((B * N, H, W, 8), dtype=torch.float32, device=frame.device)
    _lib.call('swem_prep_value_input_f32', _stream(), frame.data_ptr(), masks.data_ptr(), C.addressof(mean3),
              C.addressof(std3), out.data_ptr(), B, N, H, W, int(single_obj))
    return out


# conv1 of the encoders as a 4x4 / stride-1 convolution on the space-to-depth input (include/swem_hip.h,
# swem_prep_input_s2d_f32): inference only (the training step keeps the 7x7 form, whose weight gradient it needs)
S2D_STEMS = os.environ.get('SWEM_S2D_STEMS', '1') != '0'


def pack_stem_s2d(weight, bias=None, bn=None):
    """7x7 / stride-2 / pad-3 stem filters (Cout, Cin <= 8, 7, 7) -> the ConvPack of the equivalent 4x4 / stride-1 / pad-1
    convolution on the space-to-depth input: w'[co][(py*2+px)*8 + c][dy][dx] = w[co][c][2dy+py-1][2dx+px-1]."""
    co, ci, kh, kw = weight.shape
    assert kh == 7 and kw == 7 and ci <= 8
    w = weight.detach().float()
    w2 = torch.zeros((co, 32, 4, 4), dtype=torch.float32, device=w.device)
    for dy in range(4):
        for py in range(2):
            ky = 2 * dy + py - 1
            if not 0 <= ky < 7:
                continue
            for dx in range(4):
                for px in range(2):
                    kx = 2 * dx + px - 1
                    if 0 <= kx < 7:
                        w2[:, (py * 2 + px) * 8:(py * 2 + px) * 8 + ci, dy, dx] = w[:, :, ky, kx]
    pk = pack_conv(w2, bias, bn, 1, 1)
    pk.cin_true = ci * 49 / 16.0          # useful FLOPs of the layer are the 7x7 convolution's (bench accounting)
    return pk


def prep_input_s2d(frame, masks, mean3, std3, single_obj=False):
    """frame NCHW (B,3,H,W) [+ masks (B,N+1,H,W)] -> the normalised space-to-depth input NHWC (B*N, H/2+1, W/2+1, 32) with
    its bf16 planes already attached (ops.presplit finds them: no split launch)."""
    _chk(frame, 'frame')
    B, _, H, W = frame.shape
    N = 1
    if masks is not None:
        _chk(masks, 'masks')
        N = masks.shape[1] - 1
    Hb, Wb = H // 2 + 1, W // 2 + 1
    out = torch.empty((B * N, Hb, Wb, 32), dtype=torch.float32, device=frame.device)
    site = ('prep_s2d', B * N, H, W)
    # (three bf16 planes unless the stem that consumed this input on an earlier frame asked for the fp16 pair)
    npl = PLANES_F16 if BOOK.hints.get(site, {}).get(False) == PLANES_F16 else 3
    sp = _new_planes(npl, out.numel(), frame.device)
    _lib.call('swem_prep_input_s2d_f32', _stream(), frame.data_ptr(), _ptr(masks), C.addressof(mean3), C.addressof(std3),
              out.data_ptr(), sp.data_ptr(), npl, B, N, H, W, int(single_obj), _fault_ptr(frame.device))
    out.__dict__['_swem_split'] = {_pkey(False, npl): (sp, npl)}
    out.__dict__['_swem_split_ver'] = out._version
    out.__dict__['_swem_site'] = site
    return out


def maxpool(x):
    _chk(x)
    B, H, W, Cc = x.shape
    y = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), dtype=torch.float32, device=x.device)
    site = ('maxpool', B, H, W, Cc)
    planes, pargs = _fused_planes(site, y.numel(), y.device) if Cc % 8 == 0 else ({}, None)
    if planes:
        _lib.call('swem_maxpool3x3s2_nhwc_f32_planes', _stream(), x.data_ptr(), y.data_ptr(), B, H, W, Cc, *pargs,
                  _fault_ptr(x.device))
        y.__dict__['_swem_split'] = planes
        y.__dict__['_swem_split_ver'] = y._version
    else:
        _lib.call('swem_maxpool3x3s2_nhwc_f32', _stream(), x.data_ptr(), y.data_ptr(), B, H, W, Cc)
    y.__dict__['_swem_site'] = site
    return y


def _fused_planes(site, numel, device):
    """(planes dict {relu: (tensor, nplanes)}, C-ABI argument list) for a producer at `site` whose consumers split its output
    on an earlier frame (SPLIT_HINTS): the producer writes the planes itself."""
    want = BOOK.hints.get(site) if FUSE_SPLIT else None
    planes, pargs = {}, [0, 3, 0, 3]
    if want:
        for relu_v, npl in want.items():
            sp = _new_planes(npl, numel, device)
            planes[relu_v] = (sp, npl)
            pargs[2 * int(relu_v)], pargs[2 * int(relu_v) + 1] = sp.data_ptr(), npl
    return _keyed(planes), pargs


def upsample_add(skip, low, batch=None):
    """skip (B, 1 or B / n, Ho, Wo, C) + bilinear(low (B, Hl, Wl, C)); a skip batch of B / n: item b adds skip image b // n (the n
    objects of a clip share the clip's skip feature -- no per-object copy)."""
    _chk(skip)
    _chk(low)
    B = low.shape[0]
    Bs, Ho, Wo, Cc = skip.shape
    if B % Bs:
        raise _lib.SwemHipError('upsample_add: %d skip images for a batch of %d' % (Bs, B))
    y = torch.empty((B, Ho, Wo, Cc), dtype=torch.float32, device=low.device)
    sbs = 0 if (Bs == 1 and B > 1) else Ho * Wo * Cc
    group = B // Bs if Bs > 1 else 1
    site = ('upsample_add', B, Ho, Wo, Cc)
    planes, pargs = _fused_planes(site, y.numel(), y.device) if Cc % 8 == 0 else ({}, None)
    if planes:
        _lib.call('swem_upsample_add_grouped_nhwc_f32_planes', _stream(), skip.data_ptr(), sbs, group, low.data_ptr(), y.data_ptr(), B,
                  low.shape[1], low.shape[2], Ho, Wo, Cc, *pargs, _fault_ptr(low.device))
        y.__dict__['_swem_split'] = planes
        y.__dict__['_swem_split_ver'] = y._version
    else:
        _lib.call('swem_upsample_add_grouped_nhwc_f32', _stream(), skip.data_ptr(), sbs, group, low.data_ptr(), y.data_ptr(), B,
                  low.shape[1], low.shape[2], Ho, Wo, Cc)
    y.__dict__['_swem_site'] = site
    return y


def resize_planes(x, size, mode):
    """F.interpolate on the last two dims; mode 'nearest', 'bilinear' or 'bicubic' (align_corners=False), or 'flip'
    (horizontal flip, size unchanged)."""
    _chk(x)
    Hi, Wi = x.shape[-2:]
    planes = x.numel() // (Hi * Wi)
    y = torch.empty(tuple(x.shape[:-2]) + tuple(size), dtype=torch.float32, device=x.device)
    _lib.call('swem_resize_planes_f32', _stream(), x.data_ptr(), y.data_ptr(), planes, Hi, Wi, size[0], size[1],
              {'nearest': 0, 'bilinear': 1, 'bicubic': 2, 'flip': 3}[mode])
    return y


def flip_w(x):
    return resize_planes(x, tuple(x.shape[-2:]), 'flip')


def augment_clips(src, lab, params, frames, masks, valid, label, found, ws, b0=0, entry='swem_augment_clips_u8'):
    """swem_augment_clips_u8 (include/swem_hip_data.h): the clips of `src` (B,T,Hs,Ws,3) uint8 / `lab` (B,T,Hs,Ws) uint8 under the
    packed device parameter block `params` into slots b0..b0+B-1 of the five outputs.  `ws`: a uint8 tensor of at least
    swem_augment_workspace bytes (the caller's own: the warped labels and region codes stay readable in it)."""
    for t, dt, name in ((src, torch.uint8, 'src'), (lab, torch.uint8, 'lab'), (frames, torch.float32, 'frames'),
                        (masks, torch.float32, 'masks'), (valid, torch.float32, 'valid'), (label, torch.int64, 'label'),
                        (found, torch.int32, 'found'), (ws, torch.uint8, 'ws')):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise _lib.SwemHipError('augment_clips: %s must be a contiguous %s device tensor (got %s %s contiguous=%s)'
                                    % (name, dt, t.device, t.dtype, t.is_contiguous()))
    B, T, Hs, Ws = lab.shape
    Bo, To, C1, Ho, Wo = masks.shape
    if tuple(src.shape) != (B, T, Hs, Ws, 3) or To != T or tuple(frames.shape) != (Bo, T, 3, Ho, Wo) or \
            tuple(label.shape) != (Bo, T, Ho, Wo) or tuple(valid.shape) != (Bo, C1) or tuple(found.shape) != (Bo,):
        raise _lib.SwemHipError('augment_clips: inconsistent shapes src %s lab %s frames %s masks %s valid %s label %s found %s'
                                % tuple(tuple(t.shape) for t in (src, lab, frames, masks, valid, label, found)))
    if not (0 <= b0 and b0 + B <= Bo):
        raise _lib.SwemHipError('augment_clips: clips %d..%d do not fit a batch of %d' % (b0, b0 + B - 1, Bo))
    from .augment import frame_block_words
    words = frame_block_words(B, T)
    if not (params.is_cuda and params.is_contiguous() and params.element_size() == 4 and params.numel() >= words):
        raise _lib.SwemHipError('augment_clips: params must be a contiguous device block of %d 32-bit words' % words)
    _lib.call(entry, _stream(), src.data_ptr(), lab.data_ptr(), params.data_ptr(), frames[b0:].data_ptr(),
              masks[b0:].data_ptr(), valid[b0:].data_ptr(), label[b0:].data_ptr(), found[b0:].data_ptr(), B, T, Hs, Ws, Ho, Wo,
              C1 - 1, ws.data_ptr(), ws.numel())


def augment_static(src, lab, params, frames, masks, valid, label, found, ws, b0=0):
    """swem_augment_static_u8: `augment_clips` in the static chain's form (words 60..63 of the frame record are read; the last two
    dims of `lab` are the slot size)."""
    augment_clips(src, lab, params, frames, masks, valid, label, found, ws, b0, entry='swem_augment_static_u8')


def synth_frames(imgs, masks, params, comp, comp_lab, ws):
    """swem_synth_frames_u8 (include/swem_hip_data.h): `imgs` (B,N,Hmax,Wmax,3) / `masks` (B,N,Hmax,Wmax) uint8 slots under the
    packed device synth block `params` into the composites `comp` (B,T,Hmax,Wmax,3) and their labels `comp_lab` (B,T,Hmax,Wmax).
    `ws`: a uint8 tensor of at least swem_synth_workspace bytes (statistics and placement table stay readable in it)."""
    for t, name in ((imgs, 'imgs'), (masks, 'masks'), (comp, 'comp'), (comp_lab, 'comp_lab'), (ws, 'ws')):
        if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise _lib.SwemHipError('synth_frames: %s must be a contiguous uint8 device tensor (got %s %s contiguous=%s)'
                                    % (name, t.device, t.dtype, t.is_contiguous()))
    if masks.dim() != 4 or comp_lab.dim() != 4:
        raise _lib.SwemHipError('synth_frames: masks and comp_lab are 4-d, got %s %s' % (tuple(masks.shape), tuple(comp_lab.shape)))
    B, N, Hm, Wm = masks.shape
    T = comp_lab.shape[1]
    if tuple(imgs.shape) != (B, N, Hm, Wm, 3) or tuple(comp_lab.shape) != (B, T, Hm, Wm) or tuple(comp.shape) != (B, T, Hm, Wm, 3):
        raise _lib.SwemHipError('synth_frames: inconsistent shapes imgs %s masks %s comp %s comp_lab %s'
                                % tuple(tuple(t.shape) for t in (imgs, masks, comp, comp_lab)))
    from .augment import synth_block_words
    words = synth_block_words(B, T)
    if not (params.is_cuda and params.is_contiguous() and params.element_size() == 4 and params.numel() >= words):
        raise _lib.SwemHipError('synth_frames: params must be a contiguous device block of %d 32-bit words' % words)
    _lib.call('swem_synth_frames_u8', _stream(), imgs.data_ptr(), masks.data_ptr(), params.data_ptr(), comp.data_ptr(),
              comp_lab.data_ptr(), B, T, N, Hm, Wm, ws.data_ptr(), ws.numel())


def lincomb(a, alpha, b=None, beta=0.0):
    """alpha*a + beta*b on the device (TTA averaging)."""
    _chk(a)
    y = torch.empty_like(a)
    _lib.call('swem_lincomb_f32', _stream(), a.data_ptr(), float(alpha), _ptr(None if b is None else _chk(b)),
              float(beta), y.data_ptr(), a.numel())
    return y


def inject_objects(prob, new_masks):
    """swem_evaluator.py:124-130 -> (B, N1 + Nn1 - 1, H, W)."""
    _chk(prob)
    new_masks = _chk(new_masks.float().contiguous())
    B, N1, H, W = prob.shape
    Nn1 = new_masks.shape[1]
    out = torch.empty((B, N1 + Nn1 - 1, H, W), dtype=torch.float32, device=prob.device)
    _lib.call('swem_inject_objects_f32', _stream(), prob.data_ptr(), new_masks.data_ptr(), out.data_ptr(), B, N1, Nn1,
              H * W)
    return out


def mask_prep(hard, soft, h, w):
    """swem.py:79-84 -> (B*N, 2, h*w)."""
    if hard.dtype not in (torch.int64, torch.float32):
        hard = hard.float()
    if not (hard.is_cuda and hard.is_contiguous()):
        raise _lib.SwemHipError('mask_prep: hard mask must be a contiguous device tensor')
    _chk(soft, 'soft mask')
    B, N1 = hard.shape[:2]
    N = N1 - 1
    out = torch.empty((B * N, 2, h * w), dtype=torch.float32, device=soft.device)
    _lib.call('swem_mask_prep_f32', _stream(), hard.data_ptr(), int(hard.dtype == torch.int64), hard.shape[2],
              hard.shape[3], soft.data_ptr(), soft.shape[2], soft.shape[3], out.data_ptr(), B, N, h, w)
    return out


def cbam_residual(x, w1, b1, w2, b2, w7, b7):
    """x + CBAM(x) (networks.py:46-47)."""
    _chk(x)
    B, H, W, Cc = x.shape
    hid = w1.shape[0]
    y = torch.empty_like(x)
    cscale = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    wsb = _lib.query('swem_cbam_workspace', B, H, W, Cc)
    ws = workspace(wsb, x.device)
    site = ('cbam', B, H, W, Cc)
    planes, pargs = _fused_planes(site, y.numel(), y.device) if Cc % 8 == 0 else ({}, None)
    args = (_stream(), x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w7.data_ptr(),
            b7.data_ptr(), cscale.data_ptr(), y.data_ptr(), B, H, W, Cc, hid, ws.data_ptr(), wsb)
    if planes:
        _lib.call('swem_cbam_f32_planes', *args, *pargs, _fault_ptr(x.device))
        y.__dict__['_swem_split'] = planes
        y.__dict__['_swem_split_ver'] = y._version
    else:
        _lib.call('swem_cbam_f32', *args)
    y.__dict__['_swem_site'] = site
    return y


def pred_head(x, w, bias):
    _chk(x)
    B, H, W, Cc = x.shape
    out = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    _lib.call('swem_pred_head_f32', _stream(), x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, W,
              Cc)
    return out


def decode_head(logit4, B, N, out_size, valid=None, want_argmax=False):
    _chk(logit4)
    h4, w4 = logit4.shape[-2:]
    Ho, Wo = out_size
    dev = logit4.device
    logits = torch.empty((B, N + 1, Ho, Wo), dtype=torch.float32, device=dev)
    prob = torch.empty_like(logits)
    amax = torch.empty((B, Ho, Wo), dtype=torch.int64, device=dev) if want_argmax else None
    if valid is not None:
        valid = _chk(valid.float().contiguous(), 'valid_obj')
    _lib.call('swem_decode_head_f32', _stream(), logit4.data_ptr(), _ptr(valid), logits.data_ptr(), prob.data_ptr(),
              _ptr(amax), B, N, h4, w4, Ho, Wo)
    return logits, prob, amax


def argmax_onehot(prob, want_onehot=True):
    _chk(prob)
    B, N1, H, W = prob.shape
    amax = torch.empty((B, H, W), dtype=torch.int64, device=prob.device)
    onehot = torch.empty((B, N1, H, W), dtype=torch.int64, device=prob.device) if want_onehot else None
    _lib.call('swem_argmax_onehot_i64', _stream(), prob.data_ptr(), amax.data_ptr(), _ptr(onehot), B, N1, H * W)
    return amax, onehot


def concat2(x0, x1, batch):
    """NHWC channel concat; a source with batch 1 is shared by all `batch` items."""
    _chk(x0)
    _chk(x1)
    _, H, W, c0 = x0.shape
    c1 = x1.shape[3]
    y = torch.empty((batch, H, W, c0 + c1), dtype=torch.float32, device=x0.device)
    bs0 = 0 if (x0.shape[0] == 1 and batch > 1) else H * W * c0
    bs1 = 0 if (x1.shape[0] == 1 and batch > 1) else H * W * c1
    _lib.call('swem_concat2_nhwc_f32', _stream(), x0.data_ptr(), c0, bs0, x1.data_ptr(), c1, bs1, y.data_ptr(), batch,
              H * W)
    return y


def pack_u8(idx):
    """int64 index maps -> uint8 on the device (basic_evaluator.py:176)."""
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous()):
        raise _lib.SwemHipError('pack_u8: need a contiguous int64 device tensor')
    out = torch.empty(idx.shape, dtype=torch.uint8, device=idx.device)
    _lib.call('swem_pack_u8_i64', _stream(), idx.data_ptr(), out.data_ptr(), idx.numel())
    return out


def _chk_u8(t, name, ndim):
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == ndim):
        raise _lib.SwemHipError('%s: need a contiguous %d-d uint8 device tensor (got %s %s %s)'
                                % (name, ndim, t.device, t.dtype, tuple(t.shape)))
    return t


def _table_bytes(table, n, name):
    """A small host table (numpy array, list, bytes) as `n` bytes for a by-value launch argument."""
    import numpy as np
    b = np.ascontiguousarray(np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table).astype(np.uint8, casting='unsafe')).tobytes()
    if len(b) != n:
        raise _lib.SwemHipError('%s: the table holds %d entries, not %d' % (name, len(b), n))
    return b


def stage_frames_u8(frames_u8, size):
    """swem_stage_frames_u8 (include/swem_hip_io.h): (T,Hs,Ws,3) uint8 RGB on the device -> (T,3,Ho,Wo) fp32 in [0,1], b / 255
    then the bicubic resize of `resize_planes`."""
    _chk_u8(frames_u8, 'stage_frames_u8', 4)
    T, Hs, Ws, ch = frames_u8.shape
    if ch != 3:
        raise _lib.SwemHipError('stage_frames_u8: frames are (T,H,W,3) RGB, got %s' % (tuple(frames_u8.shape),))
    out = torch.empty((T, 3, int(size[0]), int(size[1])), dtype=torch.float32, device=frames_u8.device)
    _lib.call('swem_stage_frames_u8', _stream(), frames_u8.data_ptr(), out.data_ptr(), T, Hs, Ws, int(size[0]), int(size[1]))
    return out


def labels_onehot_u8(label_u8, chan_table, channels):
    """swem_labels_onehot_u8: (H,W) uint8 index map on the device + a 256-entry host table label -> channel (255: none) ->
    (channels,H,W) fp32 one-hot."""
    _chk_u8(label_u8, 'labels_onehot_u8', 2)
    H, W = label_u8.shape
    out = torch.empty((int(channels), H, W), dtype=torch.float32, device=label_u8.device)
    _lib.call('swem_labels_onehot_u8', _stream(), label_u8.data_ptr(), _table_bytes(chan_table, 256, 'labels_onehot_u8'),
              out.data_ptr(), int(channels), H, W)
    return out


def pack_u8_lut(idx, id_table):
    """swem_pack_u8_lut_i64: int64 index maps -> uint8 object ids `id_table[idx]` on the device (0 beyond the table):
    basic_evaluator.py:202-206 fused with `pack_u8`."""
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous()):
        raise _lib.SwemHipError('pack_u8_lut: need a contiguous int64 device tensor')
    n_ids = len(id_table)
    out = torch.empty(idx.shape, dtype=torch.uint8, device=idx.device)
    _lib.call('swem_pack_u8_lut_i64', _stream(), idx.data_ptr(), out.data_ptr(), idx.numel(),
              _table_bytes(id_table, n_ids, 'pack_u8_lut'), n_ids)
    return out


def overlay_u8(frames_u8, labels_u8, palette, alpha=0.4):
    """swem_overlay_u8: (T,H,W,3) uint8 RGB frames + (T,H,W) uint8 index maps + a 256x3 RGB palette -> (T,H,W,3) uint8 overlay
    pictures (utils/visualization.py:46-72)."""
    _chk_u8(frames_u8, 'overlay_u8 frames', 4)
    _chk_u8(labels_u8, 'overlay_u8 labels', 3)
    T, H, W, ch = frames_u8.shape
    if ch != 3 or tuple(labels_u8.shape) != (T, H, W) or labels_u8.device != frames_u8.device:
        raise _lib.SwemHipError('overlay_u8: frames (T,H,W,3) and labels (T,H,W) on one device, got %s and %s'
                                % (tuple(frames_u8.shape), tuple(labels_u8.shape)))
    out = torch.empty_like(frames_u8)
    nbytes = _lib.query('swem_overlay_workspace', T)
    ws = workspace(nbytes, frames_u8.device)
    alpha = float(alpha)
    _lib.call('swem_overlay_u8', _stream(), frames_u8.data_ptr(), labels_u8.data_ptr(), _table_bytes(palette, 768, 'overlay_u8'),
              alpha, 1.0 - alpha, out.data_ptr(), T, H, W, ws.data_ptr(), nbytes)
    return out


PNG_CODES = {'fixed': 0, 'dynamic': 1}       # SWEM_PNG_CODES_* of include/swem_hip_io.h


def png_encode_u8(maps_u8, palette768=None, blob=None, codes='fixed'):
    """swem_png_encode_u8 / swem_png_encode_px_u8: (T,H,W) uint8 index maps or (T,H,W,3) uint8 RGB pictures on the device ->
    (blob, offsets), both on the device: T complete PNG files back to back, file t = blob[offsets[t]:offsets[t + 1]] (offsets:
    T + 1 int64).  palette768: 256x3 RGB -> palette PNGs; None -> grayscale (utils/visualization.py:40-43 either way); the 4-d
    form writes colour type 2 and takes no palette.  codes: 'fixed' -- the fixed Huffman codes; 'dynamic' -- a table of each
    segment's own where that is smaller.  blob: a uint8 device buffer of at least T * io.png_capacity(H, W, channels) bytes to
    write into (default: a new one).  Nothing here waits for the device: copy `offsets`, then blob[:offsets[T]]."""
    if codes not in PNG_CODES:
        raise ValueError("png_encode_u8: codes is 'fixed' or 'dynamic', got %r" % (codes,))
    channels = 3 if maps_u8.dim() == 4 else 1
    _chk_u8(maps_u8, 'png_encode_u8', 4 if channels == 3 else 3)
    T, H, W = maps_u8.shape[:3]
    if channels == 3 and (maps_u8.shape[3] != 3 or palette768 is not None):
        raise _lib.SwemHipError('png_encode_u8: pictures are (T,H,W,3) and take no palette, got %s' % (tuple(maps_u8.shape),))
    px = channels == 3 or codes != 'fixed'         # the default call stays on the first entry point
    cap = _lib.query('swem_png_capacity_px', H, W, channels) if px else _lib.query('swem_png_capacity', H, W)
    if blob is None:
        blob = torch.empty(max(T * cap, 1), dtype=torch.uint8, device=maps_u8.device)
    elif _chk_u8(blob, 'png_encode_u8 blob', 1).device != maps_u8.device:
        raise _lib.SwemHipError('png_encode_u8: blob and maps on one device')
    offsets = torch.empty(T + 1, dtype=torch.int64, device=maps_u8.device)
    nbytes = _lib.query('swem_png_workspace_px', T, H, W, channels) if px else _lib.query('swem_png_workspace', T, H, W)
    ws = workspace(nbytes, maps_u8.device)
    pal = None if palette768 is None else _table_bytes(palette768, 768, 'png_encode_u8')
    if px:
        _lib.call('swem_png_encode_px_u8', _stream(), maps_u8.data_ptr(), channels, pal, PNG_CODES[codes], blob.data_ptr(),
                  blob.numel(), offsets.data_ptr(), T, H, W, ws.data_ptr(), nbytes)
    else:
        _lib.call('swem_png_encode_u8', _stream(), maps_u8.data_ptr(), pal, blob.data_ptr(), blob.numel(), offsets.data_ptr(),
                  T, H, W, ws.data_ptr(), nbytes)
    return blob, offsets


def png_decode_u8(blob, offsets, slot_hw, channels=1, want_palette=False):
    """swem_png_decode_u8: T PNG files back to back in `blob` (uint8, device), file t = blob[offsets[t]:offsets[t + 1]] (offsets:
    T + 1 int64 on the device -- what `png_encode_u8` returns goes straight in) -> (pixels, sizes, palettes, n_palette, status),
    all on the device: pixels (T,Hs,Ws) uint8 for channels=1 (palette and grayscale files at depths 1, 2, 4, 8, the samples as
    stored) or (T,Hs,Ws,3) for channels=3 (truecolour); a file of h x w fills the top-left corner of its slot, the rest is zero;
    sizes (T,2) int32; palettes (T,768) uint8 and n_palette (T,) int32 with want_palette, else None; status (T,) int32, 0 for a
    good file, io.PNG_STATUS names the others (such a file leaves a zero slot).  Nothing here waits for the device."""
    _chk_u8(blob, 'png_decode_u8 blob', 1)
    if not (offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.dim() == 1 and
            offsets.numel() >= 2 and offsets.device == blob.device):
        raise _lib.SwemHipError('png_decode_u8: offsets are T + 1 contiguous int64 on the blob\'s device')
    T = offsets.numel() - 1
    Hs, Ws = int(slot_hw[0]), int(slot_hw[1])
    if channels not in (1, 3):
        raise ValueError('png_decode_u8: channels is 1 or 3, got %r' % (channels,))
    dev = blob.device
    pixels = torch.empty((T, Hs, Ws, 3) if channels == 3 else (T, Hs, Ws), dtype=torch.uint8, device=dev)
    sizes = torch.empty((T, 2), dtype=torch.int32, device=dev)
    status = torch.empty(T, dtype=torch.int32, device=dev)
    palettes = torch.empty((T, 768), dtype=torch.uint8, device=dev) if want_palette else None
    n_palette = torch.empty(T, dtype=torch.int32, device=dev) if want_palette else None
    nbytes = _lib.query('swem_png_decode_workspace', T, Hs, Ws, channels, blob.numel())
    ws = workspace(nbytes, dev)
    _lib.call('swem_png_decode_u8', _stream(), blob.data_ptr(), blob.numel(), offsets.data_ptr(), T, Hs, Ws, channels,
              pixels.data_ptr(), sizes.data_ptr(), palettes.data_ptr() if want_palette else None,
              n_palette.data_ptr() if want_palette else None, status.data_ptr(), ws.data_ptr(), nbytes)
    return pixels, sizes, palettes, n_palette, status


def transpose(x, ld=None):
    """(batch, R, Cc) -> (batch, Cc, ld) with zero padded columns."""
    _chk(x)
    b, R, Cc = x.shape
    ld = R if ld is None else ld
    out = torch.empty((b, Cc, ld), dtype=torch.float32, device=x.device)
    _lib.call('swem_transpose_f32', _stream(), x.data_ptr(), out.data_ptr(), b, R, Cc, ld)
    return out


# ------------------------------------------------------------------ EM / matching
def em_pad(P):
    return _lib.query('swem_em_pad', P)


def em_norm_bases(kappa):
    """kappa (NK, C, L) -> kn (NK, C/4, L, 4): l2-normalised bases, channel-group major (include/swem_hip.h)."""
    _chk(kappa)
    NK, Cc, L = kappa.shape
    kn = torch.empty((NK, Cc // 4, L, 4), dtype=torch.float32, device=kappa.device)
    _lib.call('swem_em_norm_bases_f32', _stream(), kappa.data_ptr(), kn.data_ptr(), NK, Cc, L)
    return kn


def em_pack_bases(kappa):
    """kappa (NK, C, L) -> kp (NK, C/4 + 1, L, 4): the packed keys the E/W kernel reads (bases + their squared norms)."""
    _chk(kappa)
    NK, Cc, L = kappa.shape
    kp = torch.empty((NK, Cc // 4 + 1, L, 4), dtype=torch.float32, device=kappa.device)
    _lib.call('swem_em_pack_bases_f32', _stream(), kappa.data_ptr(), kp.data_ptr(), NK, Cc, L)
    return kp


def em_ew(x, kn, masks, w_in, tau, do_w, do_e):
    """x (P,C), kn = packed keys (NK,C/4+1,L,4), masks/w_in (NK,P) -> (weights (NK,P) or None, z (N,Pz,2L) pixel-major or None)."""
    _chk(x)
    _chk(kn)
    P, Cc = x.shape
    NK, _, L, _ = kn.shape
    w_out = torch.empty((NK, P), dtype=torch.float32, device=x.device) if do_w else None
    z = torch.zeros((NK // 2, em_pad(P), 2 * L), dtype=torch.float32, device=x.device) if do_e else None
    _lib.call('swem_em_ew_f32', _stream(), x.data_ptr(), kn.data_ptr(), _ptr(masks), _ptr(w_in), _ptr(w_out),
              _ptr(z), NK // 2, Cc, P, L, float(tau), int(do_w), int(do_e))
    return w_out, z


def em_mstep(A, per_object, z, prev, zita_prev, P, want_kn=False):
    """A (P,R) shared or (N,P,R) per object, pixel-major; z (N,Pz,2L); prev (NK,R,L); zita_prev (NK,L) -> out, zita, kn."""
    N, _, L2 = z.shape
    NK, L = 2 * N, L2 // 2
    R = prev.shape[1]
    out = torch.empty_like(prev)
    zita = torch.empty_like(zita_prev)
    kn = torch.empty((NK, R // 4 + 1, L, 4), dtype=torch.float32, device=prev.device) if want_kn else None
    wsb = _lib.query('swem_em_mstep_workspace', NK, R, P, L)
    ws = workspace(wsb, prev.device)
    _lib.call('swem_em_mstep_f32', _stream(), _chk(A).data_ptr(), int(per_object), _chk(z).data_ptr(), prev.data_ptr(),
              zita_prev.data_ptr(), out.data_ptr(), zita.data_ptr(), _ptr(kn), NK, R, P, L, ws.data_ptr(), wsb)
    return out, zita, kn


def memorize(x, v, masks, kappa_prev, nu_prev, zita_prev, T, tau, pack=None, prior_packed=False, bank=1, out=None, clips=1):
    """x (P,C); v (N,P,V); masks (N,2,P); bases (N,2,C,L)/(N,2,V,L)/(N,2,L) -> new bases.
    pack = (mkn, mvp): matching's packed banks, kept current by this call (swem_memorize_packed_f32).
    out = (kappa, nu, zita): write the new bases there (tensors of the priors' shapes that are NOT the priors: the prior is
    read by every M step); default: fresh tensors.
    clips > 1 (packed form only): the N objects are those of `clips` clips, N / clips each, with one key map per clip -- x
    (clips,P,C); per object the same launches as `clips` single-clip calls (swem_memorize_packed_clips_f32)."""
    for t in (x, v, masks, kappa_prev, nu_prev, zita_prev):
        _chk(t)
    if clips > 1:
        if pack is None or x.dim() != 3 or x.shape[0] != clips or v.shape[0] % clips:
            raise _lib.SwemHipError('memorize: clips = %d needs a pack, x (clips,P,C) and a multiple of clips objects' % clips)
        x = x.view(-1, x.shape[-1])[:x.shape[1]]          # (shape bookkeeping below: P, C of ONE clip; the pointer is the batch's)
    P, Cc = x.shape
    N, _, V = v.shape
    L = kappa_prev.shape[-1]
    if out is not None:
        kappa, nu, zita = (_chk(t) for t in out)
        if (kappa.shape != kappa_prev.shape or nu.shape != nu_prev.shape or zita.shape != zita_prev.shape
                or kappa.data_ptr() == kappa_prev.data_ptr() or nu.data_ptr() == nu_prev.data_ptr()
                or zita.data_ptr() == zita_prev.data_ptr()):
            raise _lib.SwemHipError('memorize: out must have the priors\' shapes and must not alias them')
    else:
        kappa, nu, zita = torch.empty_like(kappa_prev), torch.empty_like(nu_prev), torch.empty_like(zita_prev)
    wsb = _lib.query('swem_memorize_workspace', N, Cc, V, P, L)
    ws = workspace(wsb, x.device)
    if pack is not None and clips > 1:
        _lib.call('swem_memorize_packed_clips_f32', _stream(), x.data_ptr(), v.data_ptr(), masks.data_ptr(),
                  kappa_prev.data_ptr(), nu_prev.data_ptr(), zita_prev.data_ptr(), kappa.data_ptr(), nu.data_ptr(),
                  zita.data_ptr(), _chk(pack[0]).data_ptr(), _chk(pack[1]).data_ptr(), _pack_planes(pack),
                  int(prior_packed), int(bank), N, int(clips), Cc, V, P, L, int(T), float(tau), ws.data_ptr(), wsb,
                  _fault_ptr(x.device))
        return kappa, nu, zita
    if pack is not None:
        _lib.call('swem_memorize_packed_f32', _stream(), x.data_ptr(), v.data_ptr(), masks.data_ptr(),
                  kappa_prev.data_ptr(), nu_prev.data_ptr(), zita_prev.data_ptr(), kappa.data_ptr(), nu.data_ptr(),
                  zita.data_ptr(), _chk(pack[0]).data_ptr(), _chk(pack[1]).data_ptr(), _pack_planes(pack),
                  int(prior_packed), int(bank), N, Cc, V, P, L, int(T), float(tau), ws.data_ptr(), wsb, _fault_ptr(x.device))
        return kappa, nu, zita
    _lib.call('swem_memorize_f32', _stream(), x.data_ptr(), v.data_ptr(), masks.data_ptr(), kappa_prev.data_ptr(),
              nu_prev.data_ptr(), zita_prev.data_ptr(), kappa.data_ptr(), nu.data_ptr(), zita.data_ptr(), N, Cc, V,
              P, L, int(T), float(tau), ws.data_ptr(), wsb)
    return kappa, nu, zita


def memorize_keys(x, masks, kappa_prev, zita_prev, T, tau, pack, prior_packed=False, bank=1, out=None):
    """The part of memorize that does not read the value map (include/swem_hip.h, swem_memorize_packed_keys_f32): every E, W
    and key M step.  x (P,C); masks (N,2,P); kappa_prev (N,2,C,L); zita_prev (N,2,L) -> (kappa, zita, z); the pack's key half
    of bank `bank` is written.  out = (kappa, zita) tensors to write (not the priors)."""
    for t in (x, masks, kappa_prev, zita_prev):
        _chk(t)
    P, Cc = x.shape
    N, L = kappa_prev.shape[0], kappa_prev.shape[-1]
    if out is not None:
        kappa, zita = (_chk(t) for t in out)
        if kappa.data_ptr() == kappa_prev.data_ptr() or zita.data_ptr() == zita_prev.data_ptr():
            raise _lib.SwemHipError('memorize_keys: out must not alias the priors')
    else:
        kappa, zita = torch.empty_like(kappa_prev), torch.empty_like(zita_prev)
    z = torch.empty((N, em_pad(P), 2 * L), dtype=torch.float32, device=x.device)
    wsb = _lib.query('swem_memorize_workspace', N, Cc, 32, P, L)
    ws = workspace(wsb, x.device)
    _lib.call('swem_memorize_packed_keys_f32', _stream(), x.data_ptr(), masks.data_ptr(), kappa_prev.data_ptr(),
              zita_prev.data_ptr(), kappa.data_ptr(), zita.data_ptr(), _chk(pack[0]).data_ptr(), z.data_ptr(), int(prior_packed),
              int(bank), N, Cc, P, L, int(T), float(tau), ws.data_ptr(), wsb)
    return kappa, zita, z


def memorize_values(v, z, nu_prev, zita_prev, pack, bank=1, out=None):
    """The value update of memorize from the responsibilities `memorize_keys` left: v (N,P,V); nu_prev (N,2,V,L) -> nu; the
    pack's value half (and planes) of bank `bank` is written."""
    for t in (v, z, nu_prev, zita_prev):
        _chk(t)
    N, P, V = v.shape
    L = nu_prev.shape[-1]
    nu = _chk(out) if out is not None else torch.empty_like(nu_prev)
    if nu.data_ptr() == nu_prev.data_ptr():
        raise _lib.SwemHipError('memorize_values: out must not alias the prior')
    _lib.call('swem_memorize_packed_values_f32', _stream(), v.data_ptr(), z.data_ptr(), nu_prev.data_ptr(), zita_prev.data_ptr(),
              nu.data_ptr(), _chk(pack[1]).data_ptr(), _pack_planes(pack), int(bank), N, V, P, L, _fault_ptr(v.device))
    return nu


def _match_plan(key, launch, M, V, nkb):
    """Readout plan of matching: the book's, else under conv_math((m,)) the heuristic tile in math mode m, else tuned."""
    plan = BOOK.match.get(key + _PLAN_TAG, 0)
    if plan == 0 and len(_PLAN_TAG) == 2 and not AUTOTUNE:
        plan = _PLAN_TAG[1] << 16
    elif plan == 0 and not AUTOTUNE and (BOOK.fallback >> 16) & 3 == 3:
        plan = 3 << 16                             # a model's default: the pre-split (f16x3) readout on the heuristic tile
    if AUTOTUNE and plan == 0 and not torch.cuda.is_current_stream_capturing():
        # (the pre-split readout has ONE arithmetic, f16x3 on the pack's fp16 value planes: math field 3 selects it whatever
        # two-plane mode the convolutions run)
        modes = tuple(dict.fromkeys(3 if m == 7 else m for m in CONV_MATH_MODES))
        # (the readout is a batched GEMM with per-object filters: no 256-column tiles)
        plan = BOOK.match[key + _PLAN_TAG] = _autotune(launch, M, V, nkb, False, modes=modes, t256=False)
    return plan & ~(1 << 18)


def match(qk, kappa_first, nu_first, kappa_update, nu_update, topl, tau):
    """qk (P,C); banks (N,2,C,L)/(N,2,V,L) -> mem_out (N,P,V) (a view of a buffer with Pm >= P rows per object),
    S (N,P,2*topl)."""
    _chk(qk)
    _chk(kappa_first)
    _chk(nu_first)
    P, Cc = qk.shape
    N, _, V, L = nu_first.shape
    nb = 1
    if kappa_update is not None:
        _chk(kappa_update)
        _chk(nu_update)
        nb = 2
    Pm = _lib.query('swem_match_pad', P)
    mem_out = torch.empty((N, Pm, V), dtype=torch.float32, device=qk.device)
    S = torch.empty((N, P, 2 * topl), dtype=torch.float32, device=qk.device)

    def launch(plan):
        wsb = _lib.query('swem_match_workspace', N, Cc, V, P, L, nb, plan)
        ws = workspace(wsb, qk.device)
        _lib.call('swem_match_f32', _stream(), qk.data_ptr(), kappa_first.data_ptr(), nu_first.data_ptr(),
                  _ptr(kappa_update), _ptr(nu_update), mem_out.data_ptr(), S.data_ptr(), N, Cc, V, P, L, int(topl),
                  float(tau), plan, ws.data_ptr(), wsb)

    launch(_match_plan((N, Cc, V, P, L, nb), launch, N * Pm, V, 2 * nb * L // 32))
    return mem_out[:, :P], S


def new_pack(N, Cc, V, L, device):
    """Matching's persistent packed banks for N objects (include/swem_hip.h, swem_memorize_packed_f32): packed keys,
    packed values, and the values again as the fp16 pair (hi, mid) for the pre-split readout GEMM (f16x3 arithmetic)."""
    return (torch.zeros((2 * N, Cc // 4 + 1, 2 * L, 4), dtype=torch.float32, device=device),
            torch.zeros((N, V, 4 * L), dtype=torch.float32, device=device),
            torch.zeros((N, 2, 4 * L // 8, V, 8), dtype=torch.float16, device=device))


def value_planes_wanted():
    """Whether matching's readout may read the pack's fp16 value planes `mvq` under the CURRENT book / conv_math block (the
    pre-split f16x3 readout: _match_plan).  Where it cannot -- a book on the exact fp32 kernels (fallback 0), one that left the
    fp16 range (to_full_range), the exact-split block conv_math((0, 1)) with its tuned bf16x6 readout -- memorize neither
    writes nor range-checks them: value bases beyond 65520 are then no fault, nothing reads them as fp16.  SWEMCore stamps
    each bank of its pack with this flag and repacks a bank whose planes were left out once they are wanted again."""
    if BOOK.full_range:
        return False
    if AUTOTUNE:
        return True                        # (the tuner may choose the pre-split readout)
    # (the same order as _match_plan: a tuned plan of the current tag, else conv_math((m,))'s mode, else the book's fallback;
    # any shape's plan counts -- writing planes nobody reads costs a few microseconds, reading planes nobody wrote is wrong)
    if any((v >> 16) & 3 == 3 for k, v in BOOK.match.items() if tuple(k[6:]) == tuple(_PLAN_TAG)):
        return True
    if len(_PLAN_TAG) == 2:
        return _PLAN_TAG[1] & 3 == 3       # conv_math((m,)): the heuristic tile in math mode m (3 or 7: pre-split)
    return (BOOK.fallback >> 16) & 3 == 3


def _pack_planes(pack):
    if len(pack) < 3 or pack[2] is None or not value_planes_wanted():
        return None
    q = pack[2]
    if not (q.is_cuda and q.dtype == torch.float16 and q.is_contiguous()):
        raise _lib.SwemHipError('the value planes of a pack must be a contiguous fp16 device tensor')
    return q.data_ptr()


def pack_bank(kappa, nu, pack, bank):
    """bases (N,2,C,L) / (N,2,V,L) -> bank `bank` of a two-bank pack."""
    _chk(kappa)
    _chk(nu)
    N, _, Cc, L = kappa.shape
    _lib.call('swem_match_pack_bank_f32', _stream(), kappa.data_ptr(), nu.data_ptr(), pack[0].data_ptr(),
              pack[1].data_ptr(), _pack_planes(pack), int(bank), 2, N, Cc, nu.shape[2], L, _fault_ptr(kappa.device))


def match_packed(qk, pack, L, topl, tau, hw=None, clips=1):
    """qk (P,C); pack = (mkn (2N,C/4+1,2L,4), mvp (N,V,4L), mvq bf16 planes or None) -> mem_out (N,P,V) view, S (N,P,2*topl).
    hw = (H, W), H*W = P: the outputs come as the NHWC images (N,H,W,V) / (N,H,W,2*topl) the fusion conv consumes, and --
    once that conv has asked for their bf16 planes on an earlier frame (BOOK.hints) -- with the planes written by the
    matching kernels themselves (pre-split readout only)."""
    _chk(qk)
    mkn, mvp = _chk(pack[0]), _chk(pack[1])
    if clips > 1:        # the objects of `clips` clips, one query key map per clip: qk (clips,P,C) (swem_match_packed_clips_f32)
        if qk.dim() != 3 or qk.shape[0] != clips or mvp.shape[0] % clips:
            raise _lib.SwemHipError('match_packed: clips = %d needs qk (clips,P,C) and a multiple of clips objects' % clips)
        P, Cc = qk.shape[1:]
    else:
        P, Cc = qk.shape
    N, V = mvp.shape[0], mvp.shape[1]
    Pm = _lib.query('swem_match_pad', P)
    mem_out = torch.empty((N, Pm, V), dtype=torch.float32, device=qk.device)
    S = torch.empty((N, P, 2 * topl), dtype=torch.float32, device=qk.device)
    site_m, site_s = ('match_mem', N, P, V, L), ('match_S', N, P, topl, L)
    mvq = _pack_planes(pack)
    planes = {}

    def launch(plan):
        wsb = _lib.query('swem_match_packed_workspace', N, Cc, V, P, L, plan)
        ws = workspace(wsb, qk.device)
        args = (_stream(), qk.data_ptr(), mkn.data_ptr(), mvp.data_ptr(), mvq, mem_out.data_ptr(), S.data_ptr(), N, Cc, V, P, L,
                int(topl), float(tau), plan, ws.data_ptr(), wsb)
        want_m = BOOK.hints.get(site_m, {}).get(False) if (FUSE_SPLIT and hw and V % 8 == 0) else None
        want_s = BOOK.hints.get(site_s, {}).get(False) if (FUSE_SPLIT and hw and topl % 4 == 0) else None
        if clips > 1:
            args = args[:8] + (int(clips),) + args[8:]
        if (want_m or want_s) and mvq and (plan >> 16) & 3 == 3:
            pargs = []
            for key, want, numel in (('m', want_m, mem_out.numel()), ('s', want_s, S.numel())):
                if want and key not in planes:
                    planes[key] = (_new_planes(want, numel, qk.device), want)
                pargs += [planes[key][0].data_ptr(), planes[key][1]] if want else [0, 3]
            _lib.call('swem_match_packed_clips_f32' if clips > 1 else 'swem_match_packed_f32_planes', *args, *pargs,
                      _fault_ptr(qk.device))
        else:
            planes.clear()
            if clips > 1:
                _lib.call('swem_match_packed_clips_f32', *args, 0, 3, 0, 3, 0)
            else:
                _lib.call('swem_match_packed_f32', *args)

    launch(_match_plan((N, Cc, V, P, L, 2), launch, N * Pm, V, 4 * L // 32))
    if hw is None:
        return mem_out[:, :P], S
    mem_img, s_img = mem_out[:, :P].unflatten(1, hw), S.view(N, hw[0], hw[1], -1)
    for img, key, site in ((mem_img, 'm', site_m), (s_img, 's', site_s)):
        if key in planes:
            img.__dict__['_swem_split'] = {_pkey(False, planes[key][1]): planes[key]}
            img.__dict__['_swem_split_ver'] = img._version
        img.__dict__['_swem_site'] = site
    return mem_img, s_img
