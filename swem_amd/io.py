"""Input / output staging either side of the timed loop (reference methods/basic_modules/basic_evaluator.py:149-199,
utils/visualization.py:40-43).

* ``stage_sequence``: the evaluator's bicubic resize of the clip to 480x864 (basic_evaluator.py:160) on the device.
* ``IndexMapWriter``: predicted int64 index maps -> uint8 on the device (8x less PCIe traffic), asynchronous copy into
  pinned host memory on a side stream, palette-PNG encoding (``save_seg_mask``) on a small thread pool so that neither the
  copy nor the zlib work sits between two sequences.
* ``davis_sequence_u8`` / ``ytvos_sequence_u8``: the same staging FROM DECODED BYTES (include/swem_hip_io.h, csrc/stage.hip):
  uint8 RGB frames and palette-PNG index maps are uploaded as they are; b / 255, HWC -> CHW, the bicubic resize and the one-hot
  annotations (datasets/DAVIS_Test.py:40-49, datasets/YTVOS_Test.py:116-132) happen on the device.  The tables and the
  YouTube-VOS input size (YTVOS_Test.py:14-19, 75-91) are restated here; reading the files stays with the caller.
* ``IndexMapWriter`` also maps indices to object ids (basic_evaluator.py:202-206) and writes the overlay pictures of
  VAL.VISUALIZE (utils/visualization.py:46-72, basic_evaluator.py:185-196, 241-265), both on the device.
* ``IndexMapWriter(encode='device')`` encodes the palette PNGs on the device too (csrc/png.hip): the bytes
  that cross to the host are the files' bytes, and the thread pool only writes them out.  ``codes='dynamic'`` gives every segment
  a Huffman table of its own; ``overlay_encode='device'`` encodes the overlay pictures there as well (truecolour).
* ``png_decode`` / ``read_palette``: PNG files -- annotations, stage-0 masks, the palette file -- decoded on the device
  (csrc/png_decode.hip): the files' bytes are uploaded, inflate, unfilter and unpack run there, and the maps
  feed ``davis_sequence_u8``, ``metrics.JFMeter`` and ``augment.ClipAugmenter`` without the host touching a pixel.
Nothing here touches the model.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops


def stage_sequence(frames, masks, size=(480, 864)):
    """frames (1,T,3,H,W) fp32 in [0,1] on the device, masks (1,1,N+1,H,W) -> (in_frames (1,T,3,480,864), in_masks list
    with the first-frame mask), as basic_evaluator.py:157-163."""
    in_frames = ops.resize_planes(frames[0].float().contiguous(), tuple(size), 'bicubic').unsqueeze(0)
    in_masks = [None] * frames.shape[1]
    in_masks[0] = masks[:, 0].float()
    return in_frames, in_masks


def get_suit_size(size, ratio=16):
    """YTVOS_Test.py:14-19: to the nearer multiple of 16 (the reference adds 16, whatever `ratio`; it only ever passes 16)."""
    r = size % ratio
    size -= r
    if r > 7:
        size += 16
    return size


def ytvos_input_size(h, w, short_size=495):
    """YTVOS_Test.py:27, 75-91: the size a YouTube-VOS clip of h x w frames is fed at -- the shorter side at most
    get_suit_size(short_size) = 496, both sides multiples of 16.  720x1280 -> (496, 880)."""
    h, w = int(h), int(w)
    ssize = get_suit_size(int(short_size))
    if h < w:
        if h < ssize:
            return get_suit_size(h), get_suit_size(w)
        out_h = ssize
        return out_h, get_suit_size(get_suit_size(int(w * out_h / h)))
    if w < ssize:
        return get_suit_size(h), get_suit_size(w)
    out_w = ssize
    return get_suit_size(int(h * out_w / w)), out_w


def _labels_present(label_u8):
    """bool[256]: which labels a uint8 map holds (host array or device tensor; 256 flags come back, never the pixels)."""
    if isinstance(label_u8, torch.Tensor):
        if label_u8.dtype != torch.uint8:
            raise TypeError('label maps are uint8, got %s' % label_u8.dtype)
        return (torch.bincount(label_u8.reshape(-1).long(), minlength=256) > 0).cpu().numpy()
    a = np.asarray(label_u8)
    if a.dtype != np.uint8:
        raise TypeError('label maps are uint8, got %s' % a.dtype)
    return np.bincount(a.reshape(-1), minlength=256) > 0


def davis_table(first_label, single_obj=False):
    """The channel table of a DAVIS first-frame annotation and its channel count: (table uint8[256], obj_n).
    DAVIS_Test.py:43-48 -> data_utils.py:141-186 (to_onehot_tensor, shuffle=False): obj_n = largest label + 1 channels; the ids
    that are present take channels 1.. in ascending order (compacted: with labels {0,1,3} id 3 is channel 2 and channel 3 stays
    empty); every other label lands in channel 0, which the reference computes as 1 - sum.  single_obj: every label > 1 is label 1
    (DAVIS_Test.py:43-44)."""
    present = _labels_present(first_label).copy()
    if single_obj and present[2:].any():
        present[1] = True
        present[2:] = False
    ids = [int(i) for i in np.nonzero(present)[0] if i > 0]
    obj_n = (max(ids) if ids else 0) + 1
    if obj_n > 255:
        raise ValueError('davis_table: label 255 in the annotation would need 256 channels (255 at the most)')
    table = np.zeros(256, np.uint8)
    for k, i in enumerate(ids):
        table[i] = k + 1
    if single_obj:
        table[2:] = table[1]
    return table, obj_n


def ytvos_table(ids):
    """The channel table of a YouTube-VOS annotation frame that introduces the objects `ids` (YTVOS_Test.py:124-130): label 0 ->
    channel 0, ids[k] -> channel k + 1, every other label (an object annotated earlier) -> no channel (255)."""
    ids = [int(i) for i in ids]
    if len(ids) > 254 or len(set(ids)) != len(ids) or any(not 0 < i < 256 for i in ids):
        raise ValueError('ytvos_table: need at most 254 distinct object ids in 1..255, got %s' % (ids,))
    table = np.full(256, 255, np.uint8)
    table[0] = 0
    for k, i in enumerate(ids):
        table[i] = k + 1
    return table


def ytvos_id_table(ann):
    """obj_idx_list of YTVOS_Test.py:117-128 for ann = {frame_idx: (label_u8, ids)}: 0, then the ids in frame order and in
    list order within a frame -- index k of the evaluator's maps is object id table[k] (basic_evaluator.py:202-206)."""
    out = [0]
    for frame_idx in sorted(ann):
        out += [int(i) for i in ann[frame_idx][1]]
    if len(out) > 256 or any(not 0 <= i < 256 for i in out):
        raise ValueError('ytvos_id_table: object ids are bytes and at most 255 objects, got %s' % (out,))
    return np.asarray(out, np.uint8)


def _device_u8(x, device=None):
    """uint8 bytes on the device: a device tensor as it is, a numpy array / host tensor uploaded once from pinned memory."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        if x.dtype != torch.uint8:
            raise TypeError('decoded frames and label maps are uint8, got %s' % x.dtype)
        return x.contiguous()
    host = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if host.dtype != torch.uint8:
        raise TypeError('decoded frames and label maps are uint8, got %s' % host.dtype)
    pinned = torch.empty(host.shape, dtype=torch.uint8, pin_memory=True)
    pinned.copy_(host)
    return pinned.to('cuda' if device is None else device, non_blocking=True)


def davis_sequence_u8(frames_u8, first_label_u8, single_obj=False, size=(480, 864)):
    """DAVIS_Test.__getitem__ + basic_evaluator.py:157-163 from decoded bytes: frames_u8 (T,H,W,3) uint8 RGB, first_label_u8
    (H,W) uint8 palette indices -> (in_frames (1,T,3,480,864) fp32, in_masks with the (1,obj_n,H,W) fp32 first-frame mask,
    obj_n): what `evaluate_davis_seq` takes.  The mask stays at the source size, as in `stage_sequence`."""
    fr = _device_u8(frames_u8)
    lab = _device_u8(first_label_u8, fr.device)
    table, obj_n = davis_table(first_label_u8, single_obj)
    in_frames = ops.stage_frames_u8(fr, tuple(size)).unsqueeze(0)
    in_masks = [None] * fr.shape[0]
    in_masks[0] = ops.labels_onehot_u8(lab, table, obj_n).unsqueeze(0)
    return in_frames, in_masks, obj_n


def ytvos_sequence_u8(frames_u8, ann, short_size=495):
    """YTVOS_Test.__getitem__ from decoded bytes: frames_u8 (T,H,W,3) uint8 RGB from the first annotated frame on,
    ann = {frame_idx: (label_u8 (H,W), ids)} with the objects each annotation frame introduces -> (in_frames
    (1,T,3,out_h,out_w) fp32 at `ytvos_input_size`, init_masks with a (1,len(ids)+1,H,W) fp32 mask at every annotation frame,
    id_table): what `evaluate_ytvos_seq` takes (out_size = the frames' own H, W) and what `IndexMapWriter.submit(id_table=)`
    maps the results with."""
    if 0 not in ann:
        raise ValueError('ytvos_sequence_u8: the clip starts at its first annotated frame (ann[0] is missing)')
    fr = _device_u8(frames_u8)
    T, H, W = fr.shape[:3]
    id_table = ytvos_id_table(ann)
    in_frames = ops.stage_frames_u8(fr, ytvos_input_size(H, W, short_size)).unsqueeze(0)
    init_masks = [None] * T
    for frame_idx in sorted(ann):
        label, ids = ann[frame_idx]
        lab = _device_u8(label, fr.device)
        if tuple(lab.shape) != (H, W):
            raise ValueError('ytvos_sequence_u8: annotation %d is %s, the frames are %s' % (frame_idx, tuple(lab.shape), (H, W)))
        init_masks[frame_idx] = ops.labels_onehot_u8(lab, ytvos_table(ids), len(ids) + 1).unsqueeze(0)
    return in_frames, init_masks, id_table


def save_rgb(img, path):
    """(H,W,3) uint8 RGB -> PNG (the overlay pictures; the reference's cv2.imwrite of the BGR array)."""
    from PIL import Image
    Image.fromarray(img, 'RGB').save(path)


def save_seg_mask(pred, seg_path, palette):
    """utils/visualization.py:40-43: uint8 index map -> palette PNG."""
    from PIL import Image
    img = Image.fromarray(pred)
    if palette is not None:
        img.putpalette(palette)
    img.save(seg_path)


def default_palette(n=256):
    """DAVIS-style bit-interleaved colour map (the reference reads it from assets/davis_palette.png, not shipped here)."""
    pal = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        pal[i] = (r, g, b)
    return pal.flatten().tolist()


def png_capacity(H, W, channels=1):
    """swem_png_capacity / swem_png_capacity_px (include/swem_hip_io.h): the largest PNG file `ops.png_encode_u8` writes for an
    H x W map (channels=1) or an H x W x 3 picture (channels=3) -- every segment stored, plus the headers.  0 for a shape the
    encoder refuses."""
    from . import _lib
    if channels == 1:
        return int(_lib.query('swem_png_capacity', int(H), int(W)))
    return int(_lib.query('swem_png_capacity_px', int(H), int(W), int(channels)))


# SWEM_PNG_ST_* of include/swem_hip_io.h: the per-file status words of `png_decode`, by value
PNG_STATUS = ('OK', 'OFFSETS', 'SIGNATURE', 'CHUNK', 'CRC', 'IHDR', 'DIMENSIONS', 'UNSUPPORTED', 'METHOD', 'PLTE', 'IDAT', 'CRITICAL',
              'IEND', 'TRAILING', 'TOO_LARGE', 'ZLIB_CM', 'ZLIB_CINFO', 'ZLIB_FCHECK', 'ZLIB_FDICT', 'BLOCK_TYPE', 'STORED_LEN',
              'HLIT_HDIST', 'REPEAT', 'OVERSUBSCRIBED', 'INCOMPLETE', 'NO_EOB', 'BAD_SYMBOL', 'DISTANCE', 'NO_FINAL', 'TRUNCATED',
              'IDAT_LEFT', 'LENGTH', 'ADLER', 'FILTER', 'INDEX')


class PngDecodeError(ValueError):
    """`png_decode(check=True)` refused a file: `index` is its place in the list, `status` the word, `name` its name."""

    def __init__(self, index, status):
        self.index, self.status = int(index), int(status)
        self.name = PNG_STATUS[self.status] if 0 <= self.status < len(PNG_STATUS) else 'UNKNOWN'
        ValueError.__init__(self, 'png_decode: file %d refused: SWEM_PNG_ST_%s (%d)' % (self.index, self.name, self.status))


def _file_bytes(f):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    with open(f, 'rb') as fp:
        return fp.read()


def png_decode(files, slot_hw=None, channels=1, device=None, check=True):
    """PNG files -- a list of `bytes` or paths -- decoded on the device (csrc/png_decode.hip): the
    annotations of DAVIS and YouTube-VOS (palette PNGs), the stage-0 masks (grayscale), overlay pictures (channels=3).  The host
    concatenates the files and uploads their bytes; inflate, unfilter and unpack run on the device.
      slot_hw  : every file gets an (Hs, Ws) slot; None: the largest height and width among the files' IHDR fields (8 bytes a
                 file are read here; the kernel stays the authority on the header).  A file whose fields are 0 or past 65535
                 takes no part in the sizing -- with none left the slot is 1 x 1 -- and is then refused by the kernel
                 (DIMENSIONS, TOO_LARGE).
      channels : 1 for palette and grayscale files, 3 for truecolour; a file of the other kind is not sorted out here: the
                 kernel refuses it as UNSUPPORTED
      check    : True -- copy the status words back and raise `PngDecodeError` for the first refused file; False -- nothing waits
    Returns (pixels (T,Hs,Ws) or (T,Hs,Ws,3) uint8, sizes (T,2) int32, palettes (T,768) uint8, n_palette (T,) int32, status (T,)
    int32), all on the device.  pixels[t] feeds `metrics.JFMeter.add`, `davis_sequence_u8` and `augment.ClipAugmenter` as it is."""
    if channels not in (1, 3):
        raise ValueError('png_decode: channels is 1 or 3, got %r' % (channels,))
    data = [_file_bytes(f) for f in files]
    if not data:
        raise ValueError('png_decode: an empty list of files')
    if slot_hw is None:
        dims = [(int.from_bytes(d[20:24], 'big'), int.from_bytes(d[16:20], 'big')) for d in data if len(d) >= 24]
        slot_hw = (max([1] + [h for h, w in dims if 0 < h < 1 << 16 and 0 < w < 1 << 16]),
                   max([1] + [w for h, w in dims if 0 < h < 1 << 16 and 0 < w < 1 << 16]))
    offs = np.zeros(len(data) + 1, np.int64)
    np.cumsum([len(d) for d in data], out=offs[1:])
    blob = _device_u8(np.frombuffer(bytearray(b''.join(data) or b'\0'), np.uint8), device)
    offsets = torch.from_numpy(offs).to(blob.device, non_blocking=True)
    out = ops.png_decode_u8(blob, offsets, slot_hw, channels, want_palette=True)
    if check:
        status = out[4].cpu().numpy()
        bad = np.nonzero(status)[0]
        if bad.size:
            raise PngDecodeError(bad[0], status[bad[0]])
    return out


def read_palette(file):
    """The 768-byte palette of a palette PNG, zero-padded (numpy uint8): what VAL.DAVIS_PALETTE_DIR is read for."""
    data = _file_bytes(file)
    pal, n = png_decode([data])[2:4]
    if int(n[0]) < 1:
        raise ValueError('read_palette: the file carries no PLTE')
    return pal[0].cpu().numpy()


class IndexMapWriter:
    def __init__(self, out_dir, palette=None, workers=4, overlay_alpha=0.4, encode='host', codes='fixed', overlay_encode='host'):
        """encode='host': the index maps cross to the host as they are and PIL writes them on the thread pool.
        encode='device': `ops.png_encode_u8` makes the files on the device; only their bytes cross, and
        the pool writes them out unchanged.  The palette is then always written with 256 entries.
        codes='dynamic' (with encode='device'): a Huffman table per segment instead of the fixed codes -- smaller files.
        overlay_encode='host': the overlay pictures cross as pixels and PIL writes them.  overlay_encode='device': they are
        encoded on the device as truecolour PNGs (adaptive filters, dynamic tables) right after `ops.overlay_u8`; only file bytes
        cross."""
        if encode not in ('host', 'device'):
            raise ValueError("IndexMapWriter: encode is 'host' or 'device', got %r" % (encode,))
        if codes not in ('fixed', 'dynamic'):
            raise ValueError("IndexMapWriter: codes is 'fixed' or 'dynamic', got %r" % (codes,))
        if codes == 'dynamic' and encode != 'device':
            raise ValueError("IndexMapWriter: codes='dynamic' needs encode='device'")
        if overlay_encode not in ('host', 'device'):
            raise ValueError("IndexMapWriter: overlay_encode is 'host' or 'device', got %r" % (overlay_encode,))
        self.encode = encode
        self.codes = codes
        self.overlay_encode = overlay_encode
        self.out_dir = out_dir
        self.palette = default_palette() if palette is None else palette
        self.overlay_alpha = overlay_alpha
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.copy_stream = torch.cuda.Stream() if torch.cuda.is_available() else None
        self.pending = []

    def _palette768(self):
        pal = np.zeros(768, np.uint8)
        flat = np.asarray(self.palette, np.uint8).reshape(-1)[:768]
        pal[:flat.size] = flat
        return pal

    def _to_host(self, tensors):
        """Asynchronous copies into pinned memory on the copy stream; (host tensors, event)."""
        hosts = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in tensors]
        ev = torch.cuda.Event()
        self.copy_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.copy_stream):
            for h, t in zip(hosts, tensors):
                h.copy_(t, non_blocking=True)
            ev.record()
        for t in tensors:
            t.record_stream(self.copy_stream)
        return hosts, ev

    def _overlay(self, frames_u8, u8, device):
        fr = _device_u8(frames_u8, device)
        if tuple(fr.shape) != tuple(u8.shape) + (3,):
            raise ValueError('overlay frames are %s, the index maps %s' % (tuple(fr.shape), tuple(u8.shape)))
        return ops.overlay_u8(fr, u8, self._palette768(), self.overlay_alpha)

    def submit(self, seq_name, preds, first_index=1, id_table=None, names=None, keep=None, overlay_frames_u8=None):
        """preds: list of (1,H,W) int64 device index maps of one sequence (frames first_index, first_index+1, ...).
        Returns immediately; files appear as ``out_dir/seq_name/%05d.png``.
          id_table : index k is written as object id id_table[k] (basic_evaluator.py:202-206; `ytvos_id_table`)
          names    : the basenames of the sequence's frames, indexed by frame number: frame t is ``names[t].png``
          keep     : write only the index maps whose basename (or frame number, without `names`) is in it
                     (basename_to_save, basic_evaluator.py:258); overlays are written for every frame, as the reference does
          overlay_frames_u8 : the decoded (T,H,W,3) uint8 RGB frames of the whole sequence at the maps' size, indexed by frame
                     number (host or device): also writes ``out_dir/overlay/seq_name/<same name>.png``"""
        d = os.path.join(self.out_dir, seq_name)
        os.makedirs(d, exist_ok=True)
        stacked = torch.cat(preds, dim=0).contiguous()                 # (T-1,H,W) int64, device
        n = stacked.shape[0]
        u8 = ops.pack_u8(stacked) if id_table is None else ops.pack_u8_lut(stacked, id_table)
        device = self.encode == 'device'
        tensors, od, overlay_files = ([] if device else [u8]), None, None
        if overlay_frames_u8 is not None:
            od = os.path.join(self.out_dir, 'overlay', seq_name)
            os.makedirs(od, exist_ok=True)
            pictures = self._overlay(overlay_frames_u8[first_index:first_index + n], u8, u8.device)
            if self.overlay_encode == 'device':
                overlay_files = self._encode(list(range(n)), pictures)
            else:
                tensors.append(pictures)
        stems = [('%05d' % (first_index + t)) if names is None else names[first_index + t] for t in range(n)]
        kept = [keep is None or (stems[t] if names is not None else first_index + t) in keep for t in range(n)]
        files = None
        if device and any(kept):
            files = self._encode([t for t in range(n) if kept[t]], u8)
        hosts, ev = self._to_host(tensors)

        def write():
            for where, enc in ((d, files), (od, overlay_files)):
                if enc is not None:
                    for t, data in zip(enc[0], self._files_to_host(*enc[1:])):
                        with open(os.path.join(where, stems[t] + '.png'), 'wb') as f:
                            f.write(data)
            ev.synchronize()
            for t in range(n):
                if kept[t] and not device:
                    save_seg_mask(hosts[0].numpy()[t], os.path.join(d, stems[t] + '.png'), self.palette)
                if od is not None and overlay_files is None:
                    save_rgb(hosts[-1].numpy()[t], os.path.join(od, stems[t] + '.png'))
            return sum(kept)
        self.pending.append(self.pool.submit(write))

    def _encode(self, sel, u8):
        """The frames `sel` of u8 -- (n,H,W) index maps, or (n,H,W,3) overlay pictures -- as PNG files on the device, and the copy
        of their offsets under way on the copy stream: (sel, blob, offsets on the host, event).  Nothing here waits."""
        if len(sel) == u8.shape[0]:
            maps = u8
        elif sel == list(range(sel[0], sel[-1] + 1)):
            maps = u8[sel[0]:sel[-1] + 1]
        else:
            maps = torch.stack([u8[t] for t in sel])
        if u8.dim() == 4:
            blob, offsets = ops.png_encode_u8(maps, None, codes='dynamic')      # (fixed codes never beat the stored form here)
        else:
            blob, offsets = ops.png_encode_u8(maps, self._palette768(), codes=self.codes)
        (offs_host,), ev = self._to_host([offsets])
        blob.record_stream(self.copy_stream)
        return sel, blob, offs_host, ev

    def _files_to_host(self, blob, offs_host, ev):
        """Worker thread: wait for the offsets, copy blob[:total] on the copy stream -> the files' bytes."""
        ev.synchronize()
        offs = offs_host.tolist()
        host = torch.empty(offs[-1], dtype=torch.uint8, pin_memory=True)
        with torch.cuda.device(blob.device), torch.cuda.stream(self.copy_stream):
            host.copy_(blob[:offs[-1]], non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        done.synchronize()
        data = host.numpy()
        return [data[offs[k]:offs[k + 1]].tobytes() for k in range(len(offs) - 1)]

    def save_first(self, seq_name, mask_onehot, id_table=None, name=None, overlay_frame_u8=None):
        """Frame 0's given annotation (basic_evaluator.py:180-187, 238-244); `id_table`, `name` and the (H,W,3) uint8
        `overlay_frame_u8` as in `submit`."""
        d = os.path.join(self.out_dir, seq_name)
        os.makedirs(d, exist_ok=True)
        stem = '00000' if name is None else name
        idx, _ = ops.argmax_onehot(mask_onehot.float().contiguous(), want_onehot=False)
        u8 = ops.pack_u8(idx) if id_table is None else ops.pack_u8_lut(idx, id_table)
        if self.encode == 'device':
            blob, offsets = ops.png_encode_u8(u8, self._palette768(), codes=self.codes)
            with open(os.path.join(d, stem + '.png'), 'wb') as f:
                f.write(blob[:int(offsets[-1])].cpu().numpy().tobytes())
        else:
            save_seg_mask(u8.cpu().numpy()[0], os.path.join(d, stem + '.png'), self.palette)
        if overlay_frame_u8 is not None:
            od = os.path.join(self.out_dir, 'overlay', seq_name)
            os.makedirs(od, exist_ok=True)
            picture = self._overlay(overlay_frame_u8[None], u8, u8.device)
            if self.overlay_encode == 'device':
                (data,) = self._files_to_host(*self._encode([0], picture)[1:])
                with open(os.path.join(od, stem + '.png'), 'wb') as f:
                    f.write(data)
            else:
                save_rgb(picture.cpu().numpy()[0], os.path.join(od, stem + '.png'))

    def close(self):
        n = sum(f.result() for f in self.pending)
        self.pending = []
        self.pool.shutdown()
        return n
