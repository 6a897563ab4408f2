"""What building the PNG files on the device (config['png_on_device'], ops.png_encode) costs, and what it replaces.

    python tools/png_bench.py [--frames 60] [--runs 4] [--reps 20] [--only 1,2,3,4] [--out FILE]

1. One `ops.png_encode(..., wait=False)` launch sequence at 480 x 854 and 1080 x 1920 per mode, one plane per call and 32 per call, on
   an empty mask, a smooth one (three ellipses) and a ragged one (the ellipses of tools/tracks_bench.py with 2 % of the pixels flipped).
   Device events around `--reps` back-to-back calls, 7 such windows after a warm-up: median and spread, in us per call and per frame.
2. The host path it replaces, on this machine's CPUs, per frame on one thread: `quantize(palette)`, `.convert('RGB')` and `save` at
   compress_level=1 into memory, the same three masks.  Median of `--reps` frames after a warm-up, with the spread.
3. The bytes that travel per frame (the record: meta and the starting capacity) against the mask plane, and the files' sizes against
   Pillow's at compress_level=1 for the same planes.
4. `run_on_video` on one synthetic 480 x 854 clip of `--frames` JPEG frames (the synthetic checkpoint, one network), save_overlay off,
   the option off and on in alternating runs after a warm-up of each: the loop's own clock and a host clock round the whole call, which
   includes the writers.  The same with mattes and a trimap.  The option-off path is the parent commit's code.
No figure is asserted."""
import argparse
import contextlib
import io
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SIZES = ((480, 854), (1080, 1920))
MODES = ('rgb', 'palette', 'grey')
KINDS = ('empty', 'smooth', 'ragged')
BATCHES = (1, 32)
PALETTE = [0, 0, 0, 200, 0, 0, 0, 200, 0, 0, 0, 200] + [0] * (256 * 3 - 12)


def mask_of(hw, kind, shift=0.0):
    import numpy as np
    from tracks_bench import label_map
    if kind == 'empty':
        return np.zeros(hw, np.uint8)
    out = label_map(hw, 3, shift=shift)
    if kind == 'ragged':
        rng = np.random.default_rng(int(shift * 10) + 1)
        flip = rng.random(hw) < 0.02
        out[flip] = rng.integers(0, 4, int(flip.sum())).astype(np.uint8)
    return out


def tables_of(mode):
    import numpy as np
    pal = np.array(PALETTE, np.uint8).reshape(256, 3)
    ident = np.arange(256, dtype=np.uint8)
    return {'rgb': (pal, None), 'palette': (ident, pal), 'grey': (None, None)}[mode]


def windows(fn, reps, n=7):
    import torch
    for _ in range(3):
        fn()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def alone(emit, reps):
    import numpy as np
    import torch
    from xmem2_amd import ops, png
    emit(f'\n1. one ops.png_encode(wait=False) launch sequence (median of 7 windows of {reps} calls, with the spread), default capacity')
    for hw in SIZES:
        for mode in MODES:
            table, palette = (None if t is None else torch.from_numpy(t).cuda() for t in tables_of(mode))
            for kind in KINDS:
                for n in BATCHES:
                    dev = torch.from_numpy(np.stack([mask_of(hw, kind, 1.5 * i) for i in range(n)])).cuda()
                    capacity = png.default_capacity(*hw, mode)
                    med, lo, hi = windows(lambda: ops.png_encode(dev, mode, table, palette, capacity=capacity, wait=False), max(2, reps // n))
                    meta, _ = png.split_record(ops.png_encode(dev, mode, table, palette, capacity=capacity, wait=False).cpu().numpy(), n, capacity)
                    emit(f'   {hw[0]:4d} x {hw[1]:4d} {mode:7s} {kind:6s} batch {n:2d}: {med:9.1f} us per call ({lo:.1f} .. {hi:.1f}), {med / n:8.1f} us per frame;   '
                         f'file {int(meta[:, 0].mean()):8d} bytes, capacity {capacity}' + ('  DOES NOT FIT' if (meta[:, 0] > capacity).any() else ''))
                    del dev


def host(emit, reps):
    from PIL import Image
    emit(f'\n2. the host path per frame on one thread: quantize(palette) + convert(RGB) + save(compress_level=1) (median of {reps} frames, spread)')
    ref = Image.new('P', (1, 1))
    ref.putpalette(PALETTE)
    for hw in SIZES:
        for kind in KINDS:
            masks = [mask_of(hw, kind, 1.5 * i) for i in range(4)]
            took = []
            for i in range(reps + 2):
                t0 = time.perf_counter()
                img = Image.fromarray(masks[i % 4]).quantize(palette=ref, dither=Image.Dither.NONE).convert('RGB')
                img.save(io.BytesIO(), format='PNG', compress_level=1)
                took.append((time.perf_counter() - t0) * 1e3)
            took = took[2:]
            emit(f'   {hw[0]:4d} x {hw[1]:4d} {kind:6s}  {statistics.median(took):7.2f} ms per frame ({min(took):.2f} .. {max(took):.2f})')


def sizes(emit):
    from PIL import Image
    from xmem2_amd import png
    emit('\n3. bytes per frame that travel (record = meta + starting capacity) against the plane, and file sizes against Pillow at compress_level=1')
    ref = Image.new('P', (1, 1))
    ref.putpalette(PALETTE)
    for hw in SIZES:
        for mode in MODES:
            cap = png.default_capacity(*hw, mode)
            emit(f'   {hw[0]:4d} x {hw[1]:4d} {mode:7s} record {4 * png.META + cap:8d} bytes; the mask plane {hw[0] * hw[1]} bytes')
            for kind in KINDS:
                m = mask_of(hw, kind)
                ours = len(png.encode_host(m, mode, *tables_of(mode)))
                img = Image.fromarray(m)
                if mode == 'rgb':
                    img = img.quantize(palette=ref, dither=Image.Dither.NONE).convert('RGB')
                elif mode == 'palette':
                    img.putpalette(PALETTE)
                buf = io.BytesIO()
                img.save(buf, format='PNG', compress_level=1)
                emit(f'        {kind:6s} this rule {ours:8d} bytes, Pillow {buf.tell():8d} bytes, ratio {ours / buf.tell():.2f}')


def video(emit, frames, runs):
    import torch
    from session_bench import save_checkpoint
    from tracks_bench import write_clip
    from xmem2_amd.network import XMem
    from xmem2_amd.run_on_video import run_on_video
    with tempfile.TemporaryDirectory() as tmp:
        model = save_checkpoint(os.path.join(tmp, 'XMem_synth.pth'))
        net = XMem({'model': model, 'size': 480}, model).to('cuda').eval()
        imgs, msks = write_clip(os.path.join(tmp, 'clip'), frames, (480, 854), 1)

        def run(extra, n):
            over = dict({'model': model, 'size': 480}, **extra)
            text = io.StringIO()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(text):
                run_on_video(imgs, msks, os.path.join(tmp, f'out_{n}'), frames_with_masks=[0], print_progress=False, save_overlay=False,
                             network=net, overwrite_config=over, print_fps=True)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            return float(re.search(r'TOTAL PROCESSING TIME: ([0-9.]+)s', text.getvalue()).group(1)), wall

        for title, base in (('masks only', {}), ('with mattes and a trimap', {'mattes': {'feather': 3, 'trimap': 2}})):
            modes = {'off (parent)': dict(base), 'on, rgb': dict(base, png_on_device=True), 'on, palette': dict(base, png_on_device={'mode': 'palette'})}
            for tag, extra in modes.items():
                run(extra, 'warm')
            rows = {tag: [] for tag in modes}
            for r in range(runs):
                for tag, extra in modes.items():
                    rows[tag].append(run(extra, f'{len(base)}{tag[:6].strip()}{r}'))
            emit(f'\n4. run_on_video, 480 x 854, {frames} frames, one object, save_overlay=False, {title}: {runs} alternating runs per mode')
            for tag, v in rows.items():
                loops, walls = [a for a, _ in v], [b for _, b in v]
                emit(f'   {tag:13s} frame loop ms/frame: ' + '  '.join(f'{1e3 * a / frames:6.3f}' for a in loops) +
                     f'   median {1e3 * statistics.median(loops) / frames:6.3f};   whole call frames/s: ' +
                     '  '.join(f'{frames / b:6.1f}' for b in walls) + f'   median {frames / statistics.median(walls):6.1f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=60)
    ap.add_argument('--runs', type=int, default=4)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', default='1,2,3,4')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool measures on the MI355X'
    from xmem2_amd import build
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f'PNG files built on the device, on {torch.cuda.get_device_name(0)}; {os.cpu_count()} CPUs visible; build digest {build.source_digest()}')
    if '1' in args.only:
        alone(emit, args.reps)
    if '2' in args.only:
        host(emit, args.reps)
    if '3' in args.only:
        sizes(emit)
    if '4' in args.only:
        video(emit, args.frames, args.runs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
