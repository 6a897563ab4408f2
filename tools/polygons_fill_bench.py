"""What filling polygons back into masks (ops.fill_polygons, csrc/polygons_fill.hip) costs, next to the run-length decode.

    python tools/polygons_fill_bench.py [--frames 60] [--runs 3] [--reps 100] [--out FILE]

1. The launch sequence on its own: the seeded label maps of tools/tracks_bench.py (K ragged ellipses; a batch cycles through four
   shifted maps) at 480 x 854 and 1080 x 1920, K = 1 and 5, B = 1 and 32.  The rings are the tracer's (`ops.mask_polygons`), exact
   and simplified at tolerance 1.5; the edges are packed and uploaded before the clock starts.  Device events around `--reps`
   back-to-back calls of `xmem_polygons_fill` (the two clears, the edge launch, the resolve launch), nothing else running; three
   runs per case ALTERNATING between the exact rings, the simplified rings and `ops.rle_decode` of the same maps from their device
   record - the yardstick - after a warm-up: median and spread.  The exact fill is checked once against the maps.  Next to it the
   host's share of `ops.fill_polygons` (packing per vertex and the upload), one host clock around a whole call.
2. `metrics.compute_metrics` with the predictions read from a polygon-only tracks.json against the counts file of the same
   predictions, ground truth from PNGs: frames per second of the whole call, `--runs` runs per source alternating after a warm-up.
`--only` picks parts.  No figure is asserted."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def fill_alone(emit, reps):
    import numpy as np
    import torch
    from tracks_bench import label_map
    from xmem2_amd import _lib_raster, ops, polygons, rle
    lib = _lib_raster.load()

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def fmt(v):
        return f'{statistics.median(v):8.1f} us ({min(v):.1f} .. {max(v):.1f})'
    emit(f'\n1. xmem_polygons_fill on its own (us per call, median of 3 alternating runs of {reps} calls with the spread; ops.rle_decode of '
         'the same maps next to it)')
    for hw in ((480, 854), (1080, 1920)):
        cap = rle.default_capacity(*hw)
        for k in (1, 5):
            distinct = [label_map(hw, k, shift=1.5 * i) for i in range(4)]
            meta, words = ops.mask_polygons(torch.from_numpy(np.stack(distinct)).cuda(), k)
            exact4 = [polygons.label_rings(meta[i], words[i]) for i in range(4)]
            loose4 = [[[polygons.simplify(r, 1.5) for r in rings] for rings in rows] for rows in exact4]
            for b in (1, 32):
                dev = torch.from_numpy(np.stack([distinct[i % 4] for i in range(b)])).cuda()
                rec = ops.rle_encode(dev, k, cap, wait=False)
                out = torch.empty((b,) + hw, dtype=torch.uint8, device='cuda')
                status = torch.empty(2, dtype=torch.int32, device='cuda')
                ws = torch.empty(lib.xmem_polygons_fill_workspace_bytes(b, *hw, k), dtype=torch.uint8, device='cuda')
                calls, n_edges, host_ms = {}, {}, {}
                for tag, four in (('exact', exact4), ('tolerance 1.5', loose4)):
                    frames = [four[i % 4] for i in range(b)]
                    t0 = time.perf_counter()
                    got = ops.fill_polygons(frames, *hw)
                    host_ms[tag] = (time.perf_counter() - t0) * 1e3                 # packing, upload, launches and the status read
                    if tag == 'exact' and not torch.equal(got, dev):
                        raise SystemExit(f'the exact fill of {hw}, K = {k}, B = {b} is not the map')
                    e, p = (torch.from_numpy(a).cuda() for a in polygons.pack_edges(frames, k))
                    n_edges[tag] = len(p)
                    calls[tag] = (lambda e=e, p=p: lib.xmem_polygons_fill(
                        ctypes.c_void_p(e.data_ptr()), ctypes.c_void_p(p.data_ptr()), len(p), b, hw[0], hw[1], k, 8, None, 0,
                        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                        _lib_raster.stream_ptr()))
                calls['rle_decode'] = lambda: ops.rle_decode(rec, *hw, k, cap, out=out, check=False)
                for fn in calls.values():
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                us = {tag: [] for tag in calls}
                for _ in range(3):
                    for tag, fn in calls.items():
                        us[tag].append(run(fn))
                ratio = statistics.median(us['exact']) / statistics.median(us['rle_decode'])
                emit(f'   {hw[0]:4d} x {hw[1]:4d}, K = {k}, B = {b:2d}: exact rings ({n_edges["exact"]} edges) {fmt(us["exact"])};  tolerance 1.5 '
                     f'({n_edges["tolerance 1.5"]} edges) {fmt(us["tolerance 1.5"])};  rle_decode {fmt(us["rle_decode"])};  exact fill / decode = '
                     f'{ratio:.2f};  workspace {ws.numel()} B;  whole ops.fill_polygons call on the host clock: exact {host_ms["exact"]:.1f} ms, '
                     f'tolerance 1.5 {host_ms["tolerance 1.5"]:.1f} ms')


def evaluate(emit, frames, runs):
    import torch
    from PIL import Image
    from tracks_bench import label_map
    from xmem2_amd.metrics import compute_metrics
    from xmem2_amd.rle import TrackWriter
    hw = (480, 854)
    pal = [0, 0, 0, 200, 0, 0, 0, 200, 0, 0, 0, 200] + [0] * (256 * 3 - 12)
    with tempfile.TemporaryDirectory() as tmp:
        gt, trk, ply = (os.path.join(tmp, d, 'clip') for d in ('gt', 'tracks', 'polygons'))
        for d in (gt, trk, ply):
            os.makedirs(d)
        writer = TrackWriter(*hw, polygons=True)
        for i in range(frames):
            truth = label_map(hw, 1, shift=1.5 * i - 0.75 * frames)
            im = Image.fromarray(truth)
            im.putpalette(pal)
            im.save(os.path.join(gt, f'{i:05d}.png'), compress_level=1)
            writer.add_mask(f'{i:05d}.png', label_map(hw, 1, seed=4, shift=1.5 * i - 0.75 * frames + 3))
        doc = writer.to_dict()
        only = json.loads(json.dumps(doc))
        for ann in only['annotations']:
            for seg in ann['segmentations']:
                if seg is not None:
                    del seg['counts']
            ann['bboxes'] = ann['areas'] = [None] * frames
        for ann in doc['annotations']:
            for seg in ann['segmentations']:
                if seg is not None:
                    del seg['polygons']
        for d, content in ((trk, doc), (ply, only)):
            with open(os.path.join(d, 'tracks.json'), 'w') as f:
                json.dump(content, f, separators=(',', ':'))
        sources = {'from tracks.json, counts': os.path.join(tmp, 'tracks'), 'from tracks.json, polygons only': os.path.join(tmp, 'polygons')}
        tables = {tag: compute_metrics(os.path.join(tmp, 'gt'), d) for tag, d in sources.items()}      # warm-up, and the check
        same = tables['from tracks.json, counts'].equals(tables['from tracks.json, polygons only'])
        fps = {tag: [] for tag in sources}
        for _ in range(runs):
            for tag, d in sources.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                compute_metrics(os.path.join(tmp, 'gt'), d)
                fps[tag].append(frames / (time.perf_counter() - t0))
        emit(f'\n2. metrics.compute_metrics, one video of {frames} frames of {hw[0]} x {hw[1]}, one object, ground truth from PNGs; frames per '
             f'second of the whole call, {runs} runs per source alternating; the tables are equal: {same}')
        for tag in sources:
            emit(f'   {tag:34s} ' + ' '.join(f'{v:7.1f}' for v in fps[tag]) + f'   median {statistics.median(fps[tag]):7.1f}')
        emit(f'   counts file {os.path.getsize(os.path.join(trk, "tracks.json"))} bytes, polygon-only file '
             f'{os.path.getsize(os.path.join(ply, "tracks.json"))} bytes')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=60)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=None, help='also append the report to this file')
    ap.add_argument('--only', default='fill,evaluate', help='comma-separated parts: fill, evaluate')
    args = ap.parse_args()
    import torch
    torch.set_grad_enabled(False)

    def emit(line):
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
    emit(f'tools/polygons_fill_bench.py on {torch.cuda.get_device_name(0)}: polygons filled back into index masks')
    parts = set(args.only.split(','))
    if 'fill' in parts:
        fill_alone(emit, args.reps)
    if 'evaluate' in parts:
        evaluate(emit, args.frames, args.runs)


if __name__ == '__main__':
    main()
