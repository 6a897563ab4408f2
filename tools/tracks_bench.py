"""What the run-length track export (config['save_tracks'], ops.rle_encode) costs and what it sends to the host.

    python tools/tracks_bench.py [--frames 60] [--runs 3] [--reps 200] [--counts {list,compressed}] [--out FILE]

1. The encode on its own: seeded label maps of K ragged ellipses at 480 x 854 and 1080 x 1920, K = 1 and 5; device events around
   `--reps` back-to-back `ops.rle_encode(map, K, wait=False)` calls (the three launches and two clears of one frame), nothing else
   running; next to it the events found, the bytes of the record that travels (meta + the default capacity), the bytes of it that
   are used, and H * W, the mask it stands for.
2. `run_on_video` on files: one synthetic 480 x 854 clip of `--frames` JPEG frames (nothing outside the repository is read; the
   synthetic checkpoint), one network, `--runs` runs per mode alternating in one process after a warm-up run: save_masks only and
   neither (with save_tracks off the loop is the parent commit's), both, tracks only.  Each figure is a host clock around the whole
   call - preload, frame loop, writers joined - in frames per second.
3. The decode on its own (`ops.rle_decode`, one launch), at the sizes of part 1: device events around `--reps` back-to-back decodes
   of the device record `ops.rle_encode(map, K, wait=False)` left, checked once against the map.
4. `metrics.compute_metrics` on one synthetic 480 x 854 video of `--frames` frames whose predictions exist twice, as the palette
   PNGs `run_on_video` writes and as tracks.json: frames per second of the whole call from each, `--runs` runs alternating after a
   warm-up.  The PNG row is the parent commit's code path.
5. `--counts compressed` (config['tracks_counts']): the compressed COCO strings next to the list form in the same run - parts 2 and 4
   get a compressed row per tracks row (and both files' sizes), and part 5 times `ops.rle_compress` and `ops.rle_decompress` on their
   own at the sizes of part 1 (three runs of `--reps` launch sequences each: median and spread) and prints the bytes of the record
   that travels in both forms.
`--only` picks parts.  No figure is asserted."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

MODES = (('save_masks only (parent)', True, False, 'list'), ('neither (parent, save_masks=False)', False, False, 'list'),
         ('save_masks + save_tracks', True, True, 'list'), ('save_tracks only', False, True, 'list'))
COMPRESSED_MODES = (('save_masks + save_tracks, compressed', True, True, 'compressed'),
                    ('save_tracks only, compressed', False, True, 'compressed'))


def label_map(hw, k, seed=3, shift=0.0):
    """uint8 H x W: k ellipses with a ragged rim (a seeded radial wobble), labels 1..k."""
    import numpy as np
    h, w = hw
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros(hw, np.uint8)
    for o in range(k):
        cx, cy = w * (o + 1) / (k + 1) + shift, h * (0.5 + 0.12 * (o - (k - 1) / 2))
        ang = np.arctan2(yy - cy, xx - cx)
        wobble = 1 + 0.08 * np.sin(ang * rng.integers(5, 12) + rng.random() * 6) + 0.03 * np.sin(ang * rng.integers(20, 40))
        out[(((yy - cy) / (h / 6)) ** 2 + ((xx - cx) / (w / (2.5 * (k + 1)))) ** 2) <= wobble ** 2] = o + 1
    return out


def encode_alone(emit, reps):
    import torch
    from xmem2_amd import ops, rle
    emit('\n1. ops.rle_encode on its own (us per frame: count, scan, emit and the two clears)')
    for hw in ((480, 854), (1080, 1920)):
        for k in (1, 5):
            dev = torch.from_numpy(label_map(hw, k)).cuda()
            meta, events = ops.rle_encode(dev, k)
            cap = rle.default_capacity(*hw)
            for _ in range(5):
                ops.rle_encode(dev, k, wait=False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.rle_encode(dev, k, wait=False)
            e1.record()
            torch.cuda.synchronize()
            total = int(meta[0, :, 0].sum())
            sent, used = 4 * (k * rle.META + cap), 4 * (k * rle.META + total)
            emit(f'   {hw[0]:4d} x {hw[1]:4d}, K = {k}: {e0.elapsed_time(e1) * 1e3 / reps:7.1f} us;  {total:5d} events;  record {sent} B '
                 f'(used {used} B) against a mask of {hw[0] * hw[1]} B: {hw[0] * hw[1] / sent:.1f}x ({hw[0] * hw[1] / used:.1f}x) fewer')


def write_clip(root, t, hw, k):
    from PIL import Image
    from resize_ingest_bench import seeded_frame
    imgs, msks = os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations')
    os.makedirs(imgs); os.makedirs(msks)
    pal = [0, 0, 0, 200, 0, 0, 0, 200, 0, 0, 0, 200] + [0] * (256 * 3 - 12)
    for i in range(t):
        Image.fromarray(seeded_frame(hw, 5, shift=2 * i)).save(os.path.join(imgs, f'{i:05d}.jpg'), quality=90)
        im = Image.fromarray(label_map(hw, k, shift=1.5 * i - 0.75 * t))
        im.putpalette(pal)
        im.save(os.path.join(msks, f'{i:05d}.png'))
    return imgs, msks


def strings_alone(emit, reps):
    import statistics as st
    import torch
    from xmem2_amd import ops, rle
    emit('\n5. ops.rle_compress / ops.rle_decompress on their own (us per frame: the three launches of each and the clear of the output; '
         f'median of 3 runs of {reps} with the spread), from / to the device record of ops.rle_encode')
    for hw in ((480, 854), (1080, 1920)):
        for k in (1, 5):
            dev = torch.from_numpy(label_map(hw, k)).cuda()
            cap, ccap = rle.default_capacity(*hw), rle.default_char_capacity(*hw)
            rec = ops.rle_encode(dev, k, cap, wait=False)
            srec = ops.rle_compress(rec, *hw, k, cap, ccap, wait=False)
            pair = ops.rle_string_offsets(srec, 1, k, ccap)

            def timed(fn):
                for _ in range(5):
                    fn()
                out = []
                for _ in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    out.append(e0.elapsed_time(e1) * 1e3 / reps)
                return f'{st.median(out):7.1f} us ({min(out):.1f} .. {max(out):.1f})'
            comp = timed(lambda: ops.rle_compress(rec, *hw, k, cap, ccap, wait=False))
            dec = timed(lambda: ops.rle_decompress(pair, *hw, k, cap, check=False))
            back, status = ops.rle_decompress(pair, *hw, k, cap, check=False)
            str_len, _ = rle.split_string_record(srec.cpu().numpy(), 1, k, ccap)
            total = int(rec[:k * rle.META].view(k, rle.META)[:, 0].sum())
            exact = bool(not status.any() and torch.equal(back[k * rle.META:k * rle.META + total], rec[k * rle.META:k * rle.META + total]))
            listed, sent, used = 4 * (k * rle.META + cap), 4 * k * (rle.META + 1) + ccap, 4 * k * (rle.META + 1) + int(str_len.sum())
            emit(f'   {hw[0]:4d} x {hw[1]:4d}, K = {k}: compress {comp};  decompress {dec};  events back exactly: {exact};  {total} events, '
                 f'{int(str_len.sum())} characters;  record per frame: list {listed} B (used {4 * (k * rle.META + total)} B), compressed '
                 f'{sent} B (used {used} B)')


def video(emit, frames, runs, counts='list'):
    import torch
    from session_bench import save_checkpoint
    from xmem2_amd.network import XMem
    from xmem2_amd.run_on_video import run_on_video
    hw = (480, 854)
    with tempfile.TemporaryDirectory() as tmp:
        model = save_checkpoint(os.path.join(tmp, 'XMem_synth.pth'))
        net = XMem({'model': model, 'size': 480}, model).to('cuda').eval()
        imgs, msks = write_clip(os.path.join(tmp, 'clip'), frames, hw, 1)

        modes = MODES + (COMPRESSED_MODES if counts == 'compressed' else ())

        def run(tag, masks, tracks, n, form='list'):
            out = os.path.join(tmp, f'out_{n}')
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_on_video(imgs, msks, out, frames_with_masks=[0], print_progress=False, save_overlay=False, network=net,
                         overwrite_config={'model': model, 'size': 480, 'save_masks': masks, 'save_tracks': tracks, 'tracks_counts': form})
            torch.cuda.synchronize()
            if tracks:
                written[form] = os.path.join(out, 'tracks.json')
            return frames / (time.perf_counter() - t0)
        written = {}
        from xmem2_amd import ops
        run('warm-up', True, True, 0)
        if counts == 'compressed':
            run('warm-up', True, True, 0, 'compressed')
        before, before_strings = dict(ops.RLE_STATS), dict(ops.RLE_STRING_STATS)
        fps = {tag: [] for tag, _, _, _ in modes}
        n = 1
        for _ in range(runs):
            for tag, masks, tracks, form in modes:
                fps[tag].append(run(tag, masks, tracks, n, form))
                n += 1
        emit(f'\n2. run_on_video on files, {frames} JPEG frames of {hw[0]} x {hw[1]}, one object, one reference; frames per second of the '
             f'whole call, {runs} runs per mode alternating')
        for tag, _, _, _ in modes:
            emit(f'   {tag:36s} ' + ' '.join(f'{v:7.1f}' for v in fps[tag]) + f'   median {statistics.median(fps[tag]):7.1f}')
        import json
        path = written['list']
        doc = json.load(open(path))
        per_frame = [len(s['counts']) - 1 for a in doc['annotations'] for s in a['segmentations'] if s is not None]
        emit(f'   tracks.json of the clip: {os.path.getsize(path)} bytes; events per frame of the PREDICTED masks (synthetic weights: ragged): '
             f'min {min(per_frame)}, median {int(statistics.median(per_frame))}, max {max(per_frame)}; default capacity '
             f'{__import__("xmem2_amd.rle", fromlist=["rle"]).default_capacity(*hw)}')
        emit(f'   encode calls in the timed runs: {ops.RLE_STATS["launches"] - before["launches"]} for '
             f'{sum(t for _, _, t, _ in modes) * runs * frames} frames; frames '
             f'encoded again because their events did not fit: {ops.RLE_STATS["retries"] - before["retries"]}')
        if counts == 'compressed':
            text = open(written['compressed']).read()
            same = json.loads(open(path).read()) == __import__('xmem2_amd.rle', fromlist=['rle']).recode_tracks(json.loads(text), 'list')
            emit(f'   tracks.json with compressed counts: {len(text)} bytes against {os.path.getsize(path)} as lists; recoded to lists it is '
                 f'the list file: {same}; compress calls in the timed runs: '
                 f'{ops.RLE_STRING_STATS["launches"] - before_strings["launches"]}; frames compressed again because their characters did '
                 f'not fit: {ops.RLE_STRING_STATS["retries"] - before_strings["retries"]}')
            for a, b in (('save_masks + save_tracks', 'save_masks + save_tracks, compressed'), ('save_tracks only', 'save_tracks only, compressed')):
                spread = max(max(fps[t]) - min(fps[t]) for t in (a, b))
                diff = statistics.median(fps[b]) - statistics.median(fps[a])
                emit(f'   {b}: {diff:+.1f} frames/s against the list form, the spread of the runs is {spread:.1f}: '
                     + ('SLOWER than the list form by more than the spread' if diff < -spread else 'within the spread or faster'))


def decode_alone(emit, reps):
    import torch
    from xmem2_amd import ops, rle
    emit('\n3. ops.rle_decode on its own (us per frame: one launch, from the device record of ops.rle_encode)')
    for hw in ((480, 854), (1080, 1920)):
        for k in (1, 5):
            dev = torch.from_numpy(label_map(hw, k)).cuda()
            cap = rle.default_capacity(*hw)
            rec = ops.rle_encode(dev, k, cap, wait=False)
            out = torch.empty((1,) + hw, dtype=torch.uint8, device='cuda')
            for _ in range(5):
                ops.rle_decode(rec, *hw, k, cap, out=out, check=False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.rle_decode(rec, *hw, k, cap, out=out, check=False)
            e1.record()
            torch.cuda.synchronize()
            exact = bool(torch.equal(ops.rle_decode(rec, *hw, k, cap)[0], dev))
            emit(f'   {hw[0]:4d} x {hw[1]:4d}, K = {k}: {e0.elapsed_time(e1) * 1e3 / reps:7.1f} us;  equal to the encoded map: {exact}')


def evaluate(emit, frames, runs, counts='list'):
    import torch
    from PIL import Image
    from xmem2_amd.metrics import compute_metrics
    from xmem2_amd.rle import TrackWriter
    hw = (480, 854)
    pal = [0, 0, 0, 200, 0, 0, 0, 200, 0, 0, 0, 200] + [0] * (256 * 3 - 12)
    with tempfile.TemporaryDirectory() as tmp:
        gt, png, trk, ctrk = (os.path.join(tmp, d, 'clip') for d in ('gt', 'png', 'tracks', 'ctracks'))
        os.makedirs(gt); os.makedirs(os.path.join(png, 'masks')); os.makedirs(trk)
        writer, cwriter = TrackWriter(*hw), TrackWriter(*hw)
        for i in range(frames):
            truth = label_map(hw, 1, shift=1.5 * i - 0.75 * frames)
            pred = label_map(hw, 1, seed=4, shift=1.5 * i - 0.75 * frames + 3)
            for d, m in ((gt, truth), (os.path.join(png, 'masks'), pred)):
                im = Image.fromarray(m)
                im.putpalette(pal)
                im.save(os.path.join(d, f'{i:05d}.png'), compress_level=1)       # as the writers of run_on_video save them
            writer.add_mask(f'{i:05d}.png', pred)
            if counts == 'compressed':
                cwriter.add_mask(f'{i:05d}.png', pred, counts='compressed')
        writer.write(trk)
        frames_of = {'from PNGs (parent)': os.path.join(tmp, 'png'), 'from tracks.json': os.path.join(tmp, 'tracks')}
        if counts == 'compressed':
            cwriter.write(ctrk)
            frames_of['from tracks.json, compressed'] = os.path.join(tmp, 'ctracks')
        tables = {tag: compute_metrics(os.path.join(tmp, 'gt'), d) for tag, d in frames_of.items()}      # warm-up, and the check
        same = all(t.equals(tables['from PNGs (parent)']) for t in tables.values())
        fps = {tag: [] for tag in frames_of}
        for _ in range(runs):
            for tag, d in frames_of.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                compute_metrics(os.path.join(tmp, 'gt'), d)
                fps[tag].append(frames / (time.perf_counter() - t0))
        emit(f'\n4. metrics.compute_metrics, one video of {frames} frames of {hw[0]} x {hw[1]}, one object, ground truth from PNGs (8 decode '
             f'threads); frames per second of the whole call, {runs} runs per source alternating; the tables are equal: {same}')
        for tag in frames_of:
            emit(f'   {tag:36s} ' + ' '.join(f'{v:7.1f}' for v in fps[tag]) + f'   median {statistics.median(fps[tag]):7.1f}')
        emit(f'   tracks.json: {os.path.getsize(os.path.join(trk, "tracks.json"))} bytes; the prediction PNGs: '
             f'{sum(os.path.getsize(os.path.join(png, "masks", f)) for f in os.listdir(os.path.join(png, "masks")))} bytes')
        if counts == 'compressed':
            emit(f'   tracks.json with compressed counts: {os.path.getsize(os.path.join(ctrk, "tracks.json"))} bytes')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=60)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None, help='also append the report to this file')
    ap.add_argument('--counts', default='list', choices=('list', 'compressed'),
                    help="compressed: config['tracks_counts'] = 'compressed' next to the list form in parts 2 and 4, and part 5")
    ap.add_argument('--only', default='encode,video,decode,evaluate,strings',
                    help='comma-separated parts: encode, video, decode, evaluate, strings (the last with --counts compressed)')
    args = ap.parse_args()
    import torch
    torch.set_grad_enabled(False)

    def emit(line):
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
    emit(f'tools/tracks_bench.py on {torch.cuda.get_device_name(0)}: run-length track export, precision fp32')
    parts = set(args.only.split(','))
    if 'encode' in parts:
        encode_alone(emit, args.reps)
    if 'video' in parts:
        video(emit, args.frames, args.runs, args.counts)
    if 'decode' in parts:
        decode_alone(emit, args.reps)
    if 'evaluate' in parts:
        evaluate(emit, args.frames, args.runs, args.counts)
    if 'strings' in parts and args.counts == 'compressed':
        strings_alone(emit, args.reps)


if __name__ == '__main__':
    main()
