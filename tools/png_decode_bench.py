"""PNG annotations decoded on the device (io.png_decode, csrc/png_decode.hip) beside the host path it replaces (PIL on four
threads, then the upload of the decoded maps).  One command, writes profiles/png_decode.json:

    python tools/png_decode_bench.py [--out profiles/png_decode.json] [--no-model] [--repeats 5]

  * the workload: 70 PIL-written 480x854 palette PNGs, the ragged discs of tools/png_bench.py (and a 70th frame of them);
  * per path, alternated host / device in ONE process, medians of `--repeats` runs:
      wall          time.perf_counter from the files' bytes in host memory to the 70 maps resident on the device (synchronised)
      host CPU      time.process_time across the same span (every thread of the process)
      bytes copied  host to device
    and the device's maps against PIL's: every map equal;
  * the decoder alone (`ops.png_decode_u8` on a resident blob, seven regions of >= 0.3 s) per frame, beside the model's frame
    time from `python bench.py` started as a child process BEFORE this process opens the GPU;
  * the same for the project's own truecolour overlay files (`ops.png_encode_u8(codes='dynamic')` of 8 noisy-gradient pictures):
    their streams are literal-heavy, the decoder's serial symbol loop at its worst.
No bar was fixed in advance; the record states what was measured, also where the device path loses."""
import argparse
import io as pyio
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.jf_bench import model_frame_ms, timed_regions  # noqa: E402
from tools.png_bench import H, T, W, synthetic_blobs  # noqa: E402


def annotation_files():
    import numpy as np
    from PIL import Image
    from swem_amd import io
    maps = synthetic_blobs()
    maps = np.concatenate([maps, maps[-1:]])              # 70 annotations
    files = []
    for m in maps:
        img = Image.fromarray(m, 'P')
        img.putpalette(io.default_palette())
        buf = pyio.BytesIO()
        img.save(buf, 'PNG')
        files.append(buf.getvalue())
    return maps, files


def host_path(files, pool):
    """PIL on four threads, one upload of the decoded maps from pinned memory."""
    import numpy as np
    import torch
    from PIL import Image
    maps = list(pool.map(lambda f: np.array(Image.open(pyio.BytesIO(f))), files))
    pinned = torch.empty((len(maps),) + maps[0].shape, dtype=torch.uint8, pin_memory=True)
    for t, m in enumerate(maps):
        pinned[t].copy_(torch.from_numpy(m))
    out = pinned.cuda(non_blocking=True)
    torch.cuda.synchronize()
    return out, out.numel()


def device_path(files, channels=1):
    import torch
    from swem_amd import io
    out = io.png_decode(files, slot_hw=(H, W), channels=channels, check=True)[0]     # (check=True waits for the status words)
    torch.cuda.synchronize()
    return out, sum(len(f) for f in files) + 8 * (len(files) + 1)


def measure(fn, repeats):
    fn()
    runs = []
    for _ in range(repeats):
        c0, t0 = time.process_time(), time.perf_counter()
        _out, nbytes = fn()
        t1, c1 = time.perf_counter(), time.process_time()
        runs.append({'wall_s': t1 - t0, 'cpu_s': c1 - c0, 'bytes': nbytes})
    return runs


def summary(runs, n):
    def med(key):
        v = sorted(r[key] for r in runs)
        return v[len(v) // 2]
    return {'wall_ms_bytes_to_resident_maps': round(1e3 * med('wall_s'), 2), 'wall_ms_all_runs': [round(1e3 * r['wall_s'], 2) for r in runs],
            'host_cpu_ms_per_frame': round(1e3 * med('cpu_s') / n, 3), 'bytes_host_to_device': int(runs[0]['bytes'])}


def decoder_alone(files, channels):
    import numpy as np
    import torch
    from swem_amd import ops
    blob = torch.from_numpy(np.frombuffer(bytearray(b''.join(files)), np.uint8)).cuda()
    offs = torch.from_numpy(np.cumsum([0] + [len(f) for f in files]).astype(np.int64)).cuda()
    reps, ms = timed_regions(lambda: ops.png_decode_u8(blob, offs, (H, W), channels), regions=7, min_s=0.3)
    return {'calls_per_region': reps, 'regions_ms_per_call': [round(v, 3) for v in ms], 'median_ms_per_call': round(ms[len(ms) // 2], 3),
            'median_us_per_frame': round(1e3 * ms[len(ms) // 2] / len(files), 1), 'files_per_call': len(files)}


def filtered_file(px, ftype):
    """An (H,W,3) picture as a truecolour PNG whose every scanline has filter type `ftype`, deflated at level 0 (stored blocks:
    inflate is a copy), so that the decode times of the five types differ by the unfilter alone."""
    import struct
    import zlib
    import numpy as np
    h, w = px.shape[:2]
    rows = px.reshape(h, -1).astype(np.int32)
    a, b, c = np.zeros_like(rows), np.zeros_like(rows), np.zeros_like(rows)
    a[:, 3:] = rows[:, :-3]
    b[1:] = rows[:-1]
    c[1:, 3:] = rows[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    pred = [np.zeros_like(rows), a, b, (a + b) >> 1, np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))][ftype]
    raw = np.concatenate([np.full((h, 1), ftype, np.uint8), ((rows - pred) & 255).astype(np.uint8)], 1).tobytes()

    def chunk(t, body):
        return struct.pack('>I', len(body)) + t + body + struct.pack('>I', zlib.crc32(t + body) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw, 0)) +
            chunk(b'IEND', b''))


def unfilter_cost(pictures):
    """The decoder alone on the same 8 pictures under each filter type, stored blocks: what the serial types 3 and 4 cost."""
    import numpy as np
    out = {}
    for ftype in range(5):
        files = [filtered_file(p, ftype) for p in pictures]
        assert np.array_equal(device_path(files, 3)[0].cpu().numpy(), pictures)
        out['type_%d' % ftype] = decoder_alone(files, 3)['median_ms_per_call']
    out['what'] = ('median ms per call of 8 files of %dx%dx3, every scanline of one filter type, deflate level 0; one wavefront per '
                   'file, so a call takes what one file takes' % (H, W))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_decode.json'))
    ap.add_argument('--no-model', action='store_true')
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    model = None if args.no_model else model_frame_ms()

    import numpy as np
    import torch
    from swem_amd import ops
    from tests.png_dyn_cases import make_picture
    maps, files = annotation_files()
    pool = ThreadPoolExecutor(4)
    runs = {'host': [], 'device': []}
    host_path(files, pool)
    device_path(files)
    for _ in range(args.repeats):                         # alternated: neither path gets the quiet half of the run
        runs['host'] += measure(lambda: host_path(files, pool), 1)
        runs['device'] += measure(lambda: device_path(files), 1)
    equal = int(sum(np.array_equal(a, b) for a, b in zip(device_path(files)[0].cpu().numpy(), maps)))
    rec = {'what': 'tools/png_decode_bench.py: %d PIL-written %dx%d palette PNG annotations, bytes in host memory -> maps resident on the '
                   'device; host = PIL on 4 threads + one upload, device = io.png_decode' % (T, H, W),
           'device_name': torch.cuda.get_device_name(0), 'frames': len(files), 'repeats': args.repeats,
           'file_bytes_per_frame': int(sum(len(f) for f in files) // len(files)), 'decoded_bytes_per_frame': H * W,
           'device_maps_equal_pil': '%d / %d' % (equal, len(files)),
           'host': summary(runs['host'], len(files)), 'device': summary(runs['device'], len(files)),
           'decoder_alone': decoder_alone(files, 1)}
    # the project's own truecolour overlay files: literal-heavy streams
    pictures = np.stack([make_picture('gradient', H, W, seed=k) for k in range(8)])
    blob, offsets = ops.png_encode_u8(torch.from_numpy(pictures).cuda(), None, codes='dynamic')
    offs = offsets.cpu().tolist()
    host_blob = blob[:offs[-1]].cpu().numpy().tobytes()
    overlay_files = [host_blob[offs[k]:offs[k + 1]] for k in range(len(pictures))]
    got = device_path(overlay_files, 3)[0].cpu().numpy()
    rec['overlay_truecolour'] = {'files': len(overlay_files), 'file_bytes_per_frame': int(offs[-1] // len(pictures)),
                                 'decoded_bytes_per_frame': 3 * H * W, 'device_pictures_equal_the_source': bool(np.array_equal(got, pictures)),
                                 'host': summary(measure(lambda: host_path(overlay_files, pool), args.repeats), len(overlay_files)),
                                 'device': summary(measure(lambda: device_path(overlay_files, 3), args.repeats), len(overlay_files)),
                                 'decoder_alone': decoder_alone(overlay_files, 3)}
    rec['unfilter_by_type'] = unfilter_cost(pictures)
    if model is not None:
        rec['model'] = model
        rec['decoder_alone']['share_of_model_frame_time'] = round(
            rec['decoder_alone']['median_us_per_frame'] / (1e3 * model['ms_per_frame']), 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
