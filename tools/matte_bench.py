"""What the on-device mattes (config['mattes'], ops.mask_mattes / ops.signed_edt_sq / ops.grow_masks) cost.

    python tools/matte_bench.py [--frames 60] [--runs 4] [--reps 50] [--out FILE]

1. The launch sequences on their own at 480 x 854 and 1080 x 1920 on the ragged ellipses of tools/tracks_bench.py: K = 1 and 3
   objects, N = 1 and 32 frames per call, feather 4 (R = 2) and 32 (R = 16), one table and two (a matte and a trimap from one
   distance pass); grow and shrink by 4 and 16 pixels.  Device events around `--reps` back-to-back calls, 7 such windows after a
   warm-up: median and spread, in us per FRAME (the call's time over N).
2. `run_on_video` on one synthetic 480 x 854 clip of `--frames` JPEG frames (the synthetic checkpoint, one network), the option off
   and on in alternating runs after a warm-up of each: the loop's own clock (TOTAL PROCESSING TIME) and a host clock around the whole
   call, which includes the PNG writers.  The option-off path is the parent commit's code.
3. For scale: the same planes through `matte.signed_d2_host` (scipy's transform, both sides of the edge) on this machine's host, per
   object, the copy of the mask to the host included.
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
FEATHERS = (4, 32)
SPEC = {'feather': 4, 'trimap': 2}


def frames_of(hw, k, n):
    import numpy as np
    from tracks_bench import label_map
    distinct = [label_map(hw, k, shift=0.5 * i) for i in range(min(n, 4))]          # N = 32: four frames, eight times
    return np.stack([distinct[i % len(distinct)] for i in range(n)])


def windows(fn, reps, per=1, n=7):
    import torch
    for _ in range(5):
        fn()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps / per)
    return f'{statistics.median(out):9.1f} us ({min(out):.1f} .. {max(out):.1f})'


def alone(emit, reps):
    import numpy as np
    import torch
    from xmem2_amd import matte, ops
    emit(f'\n1. the launch sequences on their own (us per frame; median of 7 windows of {reps} calls, with the spread)')
    for hw in SIZES:
        for k in (1, 3):
            for n in (1, 32):
                dev = torch.from_numpy(frames_of(hw, k, n)).cuda()
                emit(f'   {hw[0]:4d} x {hw[1]:4d}, K = {k}, N = {n:2d}')
                r = max(1, reps // n)
                for w in FEATHERS:
                    one, radius = matte.feather_table(feather=w)
                    two = np.stack([one, matte.trimap_table(band=2, R=radius)[0]])
                    t1, t2 = torch.from_numpy(one[None]).cuda(), torch.from_numpy(two).cuda()
                    emit(f'        mattes, feather {w:2d} (R = {radius:2d}), 1 table   ' + windows(lambda: ops.mask_mattes(dev, k, t1, radius), r, n))
                    emit(f'        mattes, feather {w:2d} (R = {radius:2d}), 2 tables  ' + windows(lambda: ops.mask_mattes(dev, k, t2, radius), r, n))
                    emit(f'        signed_edt_sq, R = {radius:2d}                 ' + windows(lambda: ops.signed_edt_sq(dev, k, radius), r, n))
                out = torch.empty_like(dev)
                for rad in (4, 16):
                    emit(f'        grow {rad:2d}                               ' + windows(lambda: ops.grow_masks(dev, rad, out=out), r, n))
                    emit(f'        shrink {rad:2d}                             ' + windows(lambda: ops.grow_masks(dev, -rad, out=out), r, n))
                del dev, out
                torch.cuda.empty_cache()


def host(emit):
    import torch
    from xmem2_amd import matte
    emit('\n3. matte.signed_d2_host on this machine\'s host, per object, the copy of the mask to the host included (ms; median of 5)')
    for hw in SIZES:
        for w in FEATHERS:
            radius = matte.feather_radius(w)
            dev = torch.from_numpy(frames_of(hw, 1, 1)[0]).cuda()
            took = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                matte.signed_d2_host(dev.cpu().numpy(), 1, radius)
                took.append((time.perf_counter() - t0) * 1e3)
            emit(f'   {hw[0]:4d} x {hw[1]:4d}, R = {radius:2d}  {statistics.median(took):9.2f} ms ({min(took):.2f} .. {max(took):.2f})')


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

        def run(spec, n):
            over = {'model': model, 'size': 480}
            if spec is not None:
                over['mattes'] = dict(spec)
            text = io.StringIO()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(text):
                run_on_video(imgs, msks, os.path.join(tmp, f'out_{n}'), frames_with_masks=[0], print_progress=False, save_overlay=False,
                             network=net, overwrite_config=over, print_fps=True)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            return float(re.search(r'TOTAL PROCESSING TIME: ([0-9.]+)s', text.getvalue()).group(1)), wall

        run(None, 'w0'), run(SPEC, 'w1')
        rows = {'off (parent)': [], 'on': []}
        for r in range(runs):
            rows['off (parent)'].append(run(None, f'off{r}'))
            rows['on'].append(run(SPEC, f'on{r}'))
        emit(f'\n2. run_on_video, 480 x 854, {frames} frames, one object, mask PNGs written, mattes = {SPEC}: {runs} alternating runs per mode')
        med = {}
        for tag, v in rows.items():
            loops, walls = [a for a, _ in v], [b for _, b in v]
            med[tag] = statistics.median(loops)
            emit(f'   {tag:13s} frame loop ms/frame: ' + '  '.join(f'{1e3 * a / frames:6.3f}' for a in loops) +
                 f'   median {1e3 * med[tag] / frames:6.3f} ({frames / med[tag]:6.1f} frames/s);   whole call frames/s: ' +
                 '  '.join(f'{frames / b:6.1f}' for b in walls) + f'   median {frames / statistics.median(walls):6.1f}')
        emit(f'   difference of the medians: {1e6 * (med["on"] - med["off (parent)"]) / frames:.1f} us per frame')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=60)
    ap.add_argument('--runs', type=int, default=4)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--only', default='1,2,3')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this tool measures on the MI355X'
    from xmem2_amd import build
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f'mattes on {torch.cuda.get_device_name(0)}; build digest {build.source_digest()}')
    if '1' in args.only:
        alone(emit, args.reps)
    if '2' in args.only:
        video(emit, args.frames, args.runs)
    if '3' in args.only:
        host(emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
