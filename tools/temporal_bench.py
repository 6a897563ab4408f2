"""What temporal mask smoothing (config['temporal_smooth'], ops.temporal_mode / ops.temporal_mode_ring) costs.

    python tools/temporal_bench.py [--frames 60] [--runs 4] [--reps 50] [--out FILE]

1. The launch on its own at 480 x 854 and 1080 x 1920, r = 1, 2 and 7: one frame per call from a ring of 2 r + 1 slots, as the frame
   loop calls it, and 32 frames per call with their halo.  Two inputs: the ragged ellipses of tools/tracks_bench.py drifting from
   frame to frame with 0.2 % of the pixels flipped ('masks': what the option is for - most threads see a constant window and skip the
   vote), and four labels drawn at random per pixel and frame ('noise': every thread votes - the arithmetic bound).  Device events
   around `--reps` back-to-back calls, 7 such windows after a warm-up: median and spread, in us per launch and per frame, next to
   the bytes the launch must move (every frame of the window read once, every output frame written once) over 6.3 TB/s, the rate a
   streaming kernel reaches on this part.  At these sizes the window is resident in the caches between calls, so that floor is a
   bound on the kernel, not on what the launch costs.
2. `run_on_video` on one synthetic 480 x 854 clip of `--frames` JPEG frames (the synthetic checkpoint, one network), the option off
   and on (radius 2) in alternating runs after a warm-up of each: the loop's own clock (TOTAL PROCESSING TIME) and a host clock round
   the whole call, which includes the PNG writers.  The option-off path is the parent commit's code.
3. For scale, the user's alternative: `temporal.mode_host` on this machine's host, the copy of the masks to the host included.
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
RADII = (1, 2, 7)
BATCHES = (1, 32)
HBM_STREAM = 6.3e12                   # bytes per second


def clip_of(hw, n, kind):
    import numpy as np
    rng = np.random.default_rng(n)
    if kind == 'noise':
        return rng.integers(0, 4, (n,) + hw).astype(np.uint8)
    from tracks_bench import label_map
    distinct = [label_map(hw, 3, shift=1.5 * i) for i in range(min(n, 8))]
    out = np.stack([distinct[i % len(distinct)] for i in range(n)])
    flip = rng.random(out.shape) < 0.002
    out[flip] = rng.integers(0, 4, int(flip.sum())).astype(np.uint8)
    return out


def windows(fn, reps, n=7):
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
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def alone(emit, reps):
    import torch
    from xmem2_amd import ops
    emit(f'\n1. the launch on its own (median of 7 windows of {reps} calls, with the spread; floor = bytes the launch must move / 6.3 TB/s)')
    for hw in SIZES:
        for kind in ('masks', 'noise'):
            emit(f'   {hw[0]:4d} x {hw[1]:4d}, {kind}')
            for n in BATCHES:
                for r in RADII:
                    T = n + 2 * r
                    dev = torch.from_numpy(clip_of(hw, T, kind)).cuda()
                    flags = torch.ones(T, dtype=torch.uint8, device='cuda')
                    out = torch.empty((n,) + hw, dtype=torch.uint8, device='cuda')
                    changed = torch.empty(n, dtype=torch.int32, device='cuda')
                    med, lo, hi = windows(lambda: ops.temporal_mode_ring(dev, T, r, n, r, flags, out=out, changed=changed), max(1, reps // n))
                    moved = (T + n) * hw[0] * hw[1]
                    emit(f'        batch {n:2d}, r = {r}: {med:9.1f} us per launch ({lo:.1f} .. {hi:.1f}), {med / n:8.1f} us per frame;   '
                         f'{moved / 1e6:7.2f} MB, floor {1e6 * moved / HBM_STREAM:7.1f} us;   pixels changed per frame '
                         f'{int(changed.sum()) // n}')
                    del dev, out
                    torch.cuda.empty_cache()


def host(emit):
    import torch
    from xmem2_amd import temporal
    emit('\n3. temporal.mode_host on this machine\'s host, the copy of the masks to the host included (ms per frame; one run each)')
    for hw in SIZES:
        for r in RADII:
            n = 16 if hw == SIZES[0] else 8
            dev = torch.from_numpy(clip_of(hw, n, 'masks')).cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            temporal.mode_host(dev.cpu().numpy(), r)
            took = (time.perf_counter() - t0) * 1e3
            emit(f'   {hw[0]:4d} x {hw[1]:4d}, r = {r}, {n:2d} frames  {took / n:9.2f} ms per frame')


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

        def run(radius, n):
            over = {'model': model, 'size': 480}
            if radius is not None:
                over['temporal_smooth'] = radius
            text = io.StringIO()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(text):
                run_on_video(imgs, msks, os.path.join(tmp, f'out_{n}'), frames_with_masks=[0], print_progress=False, save_overlay=False,
                             network=net, overwrite_config=over, print_fps=True)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            said = re.search(r'TEMPORAL SMOOTHING: [^\n]*', text.getvalue())
            return float(re.search(r'TOTAL PROCESSING TIME: ([0-9.]+)s', text.getvalue()).group(1)), wall, said.group(0) if said else ''

        run(None, 'w0'), run(2, 'w1')
        rows = {'off (parent)': [], 'on': []}
        for r in range(runs):
            rows['off (parent)'].append(run(None, f'off{r}'))
            rows['on'].append(run(2, f'on{r}'))
        emit(f'\n2. run_on_video, 480 x 854, {frames} frames, one object, mask PNGs written, temporal_smooth = 2: {runs} alternating runs per mode')
        med = {}
        for tag, v in rows.items():
            loops, walls = [a for a, _, _ in v], [b for _, b, _ in v]
            med[tag] = statistics.median(loops)
            emit(f'   {tag:13s} frame loop ms/frame: ' + '  '.join(f'{1e3 * a / frames:6.3f}' for a in loops) +
                 f'   median {1e3 * med[tag] / frames:6.3f} ({frames / med[tag]:6.1f} frames/s);   whole call frames/s: ' +
                 '  '.join(f'{frames / b:6.1f}' for b in walls) + f'   median {frames / statistics.median(walls):6.1f}')
        emit(f'   difference of the medians: {1e6 * (med["on"] - med["off (parent)"]) / frames:.1f} us per frame')
        emit('   ' + rows['on'][-1][2])


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
    emit(f'temporal smoothing on {torch.cuda.get_device_name(0)}; build digest {build.source_digest()}')
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
