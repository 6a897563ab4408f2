"""What the polygon tracer (config['tracks_polygons'], ops.mask_polygons) costs and what it sends to the host.

    python tools/polygons_bench.py [--frames 60] [--runs 3] [--reps 100] [--out FILE]

1. The tracer on its own: the seeded label maps of tools/tracks_bench.py (K ragged ellipses) at 480 x 854 and 1080 x 1920, K = 1 and
   5, B = 1 and 32; device events around `--reps` back-to-back `ops.mask_polygons(maps, K, wait=False)` calls (one launch sequence
   each: the labelling, the walks, the scans, the rounds of pointer jumping, the emit), nothing else running, three runs after a
   warm-up: median and spread, per call and per frame; next to it `ops.rle_encode` on the same maps in the same run, the corners
   and rings found, the launches of one call, the bytes of the record that travels and the bytes of it that are used.  The record
   of B = 1 is checked once against `polygons.record_host`.
2. `run_on_video` on files: one synthetic 480 x 854 clip of `--frames` JPEG frames (nothing outside the repository is read; the
   synthetic checkpoint), one network, `--runs` runs per mode alternating in one process after a warm-up run: save_tracks alone (the
   loop of the commit before the option) and save_tracks with tracks_polygons on top, with and without save_masks.  Each figure is a
   host clock around the whole call - preload, frame loop, writers joined - in frames per second.
`--only` picks parts.  No figure is asserted."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

MODES = (('save_tracks only (parent)', False, None), ('save_tracks only + polygons', False, True),
         ('save_masks + save_tracks (parent)', True, None), ('save_masks + save_tracks + polygons', True, True))


def launches_of_a_call(hw, capacity):
    """the labelling's 4 (3 when the map is one tile), the outer count, 2 row walks, the scan, the column walk, then one ranking launch
    (capacity <= 4096: in LDS) or the init, the rounds, the ring scan and the emit; the clear of the count tables is a memset"""
    most = min(capacity, 4 * (hw[0] + 1) * (hw[1] + 1))
    rounds = 0 if capacity <= 4096 else (most - 1).bit_length()
    return (4 if max(hw) > 32 else 3) + 1 + 2 + 1 + 1 + (1 if capacity <= 4096 else 1 + rounds + 1 + 1), rounds


def tracer_alone(emit, reps):
    import numpy as np
    import torch
    from tracks_bench import label_map
    from xmem2_amd import ops, polygons, rle

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / reps)
        return out
    emit(f'\n1. ops.mask_polygons on its own (us per call, median of 3 runs of {reps} calls with the spread; ops.rle_encode on the same maps '
         'next to it)')
    for hw in ((480, 854), (1080, 1920)):
        cap = polygons.default_capacity(*hw)
        n_launch, rounds = launches_of_a_call(hw, cap)
        for k in (1, 5):
            for b in (1, 32):
                maps = np.stack([label_map(hw, k, shift=1.5 * i) for i in range(b)])
                dev = torch.from_numpy(maps).cuda()
                meta, words = ops.mask_polygons(dev, k)
                want = polygons.record_host(maps[0], k)
                exact = bool((meta[0] == want[0]).all() and np.array_equal(words[0], want[1]))
                poly = timed(lambda: ops.mask_polygons(dev, k, wait=False))
                enc = timed(lambda: ops.rle_encode(dev, k, wait=False))
                total = int(meta[:, :, 0].sum(axis=1).max())
                sent, used = 4 * (k * polygons.META + cap), 4 * (k * polygons.META + total)
                emit(f'   {hw[0]:4d} x {hw[1]:4d}, K = {k}, B = {b:2d}: {statistics.median(poly):8.1f} us ({min(poly):.1f} .. {max(poly):.1f}), '
                     f'{statistics.median(poly) / b:7.1f} us per frame;  rle_encode {statistics.median(enc):7.1f} us ({min(enc):.1f} .. {max(enc):.1f});  '
                     f'{total} corners in {int(meta[0, :, 1].sum())} rings (frame 0: equal to record_host: {exact});  {n_launch} launches '
                     f'({rounds} rounds on global arrays);  record per frame {sent} B (used {used} B) against a mask of {hw[0] * hw[1]} B;  '
                     f'rle events of frame 0: {int(ops.rle_encode(dev[:1], k)[0][0, :, 0].sum())}')


def video(emit, frames, runs):
    import torch
    from session_bench import save_checkpoint
    from tracks_bench import write_clip
    from xmem2_amd import ops
    from xmem2_amd.network import XMem
    from xmem2_amd.run_on_video import run_on_video
    hw = (480, 854)
    with tempfile.TemporaryDirectory() as tmp:
        model = save_checkpoint(os.path.join(tmp, 'XMem_synth.pth'))
        net = XMem({'model': model, 'size': 480}, model).to('cuda').eval()
        imgs, msks = write_clip(os.path.join(tmp, 'clip'), frames, hw, 1)
        written = {}

        def run(masks, poly, n):
            out = os.path.join(tmp, f'out_{n}')
            config = {'model': model, 'size': 480, 'save_masks': masks, 'save_tracks': True}
            if poly is not None:
                config['tracks_polygons'] = poly
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_on_video(imgs, msks, out, frames_with_masks=[0], print_progress=False, save_overlay=False, network=net, overwrite_config=config)
            torch.cuda.synchronize()
            written[poly] = os.path.join(out, 'tracks.json')
            return frames / (time.perf_counter() - t0)
        run(True, True, 0)                                            # warm-up: graphs captured, both code paths loaded
        before = dict(ops.POLY_STATS)
        fps = {tag: [] for tag, _, _ in MODES}
        n = 1
        for _ in range(runs):
            for tag, masks, poly in MODES:
                fps[tag].append(run(masks, poly, n))
                n += 1
        emit(f'\n2. run_on_video on files, {frames} JPEG frames of {hw[0]} x {hw[1]}, one object, one reference; frames per second of the '
             f'whole call, {runs} runs per mode alternating')
        for tag, _, _ in MODES:
            emit(f'   {tag:38s} ' + ' '.join(f'{v:7.1f}' for v in fps[tag]) + f'   median {statistics.median(fps[tag]):7.1f}')
        for a, b in ((MODES[0][0], MODES[1][0]), (MODES[2][0], MODES[3][0])):
            spread = max(max(fps[t]) - min(fps[t]) for t in (a, b))
            diff = statistics.median(fps[b]) - statistics.median(fps[a])
            emit(f'   {b}: {diff:+.1f} frames/s against the parent\'s path, the spread of the runs is {spread:.1f}: '
                 + ('SLOWER by more than the spread' if diff < -spread else 'within the spread or faster'))
        doc, plain = json.load(open(written[True])), json.load(open(written[None]))
        corners = [sum(len(r) // 2 for r in s['polygons']) for a in doc['annotations'] for s in a['segmentations'] if s is not None]
        emit(f'   tracks.json: {os.path.getsize(written[None])} bytes without, {os.path.getsize(written[True])} bytes with polygons; corners per frame '
             f'of the PREDICTED masks (synthetic weights: ragged): min {min(corners)}, median {int(statistics.median(corners))}, max '
             f'{max(corners)}; counts unchanged: {[a["segmentations"][0]["counts"] for a in doc["annotations"]] == [a["segmentations"][0]["counts"] for a in plain["annotations"]]}')
        emit(f'   tracer calls in the timed runs: {ops.POLY_STATS["launches"] - before["launches"]} for {2 * runs * frames} frames; frames traced '
             f'again because their corners did not fit: {ops.POLY_STATS["retries"] - before["retries"]}')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=60)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=None, help='also append the report to this file')
    ap.add_argument('--only', default='tracer,video', help='comma-separated parts: tracer, video')
    args = ap.parse_args()
    import torch
    torch.set_grad_enabled(False)

    def emit(line):
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
    emit(f'tools/polygons_bench.py on {torch.cuda.get_device_name(0)}: polygon outlines of index masks, precision fp32')
    parts = set(args.only.split(','))
    if 'tracer' in parts:
        tracer_alone(emit, args.reps)
    if 'video' in parts:
        video(emit, args.frames, args.runs)


if __name__ == '__main__':
    main()
