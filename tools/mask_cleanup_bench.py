"""What the on-device mask clean-up (config['mask_cleanup'], ops.components / ops.clean_masks) costs.

    python tools/mask_cleanup_bench.py [--frames 60] [--runs 4] [--reps 50] [--out FILE]

1. The launch sequences on their own at 480 x 854 and 1080 x 1920: a smooth one-object mask, a five-object mask (the ragged ellipses
   of tools/tracks_bench.py) and p = 0.5 noise of one label, the worst case of the union phase.  Device events around `--reps`
   back-to-back calls into preallocated outputs, 7 such windows after a warm-up: median and spread, in us per call.
   components: connectivity 8.  clean: min_area = max_hole = 16, without and with keep_largest (two labellings either way).
2. `run_on_video` on one synthetic 480 x 854 clip of `--frames` JPEG frames (the synthetic checkpoint, one network, tracks only so
   that no PNG writer runs), the option off and on in alternating runs after a warm-up of each: the loop's own clock (TOTAL
   PROCESSING TIME) and a host clock around the whole call.  The option-off path is the parent commit's code.
3. For scale: the same rules with scipy.ndimage on the host per frame, the device-to-host copy included.
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
SPEC = {'min_area': 16, 'max_hole': 16}


def masks_of(hw):
    import numpy as np
    from tracks_bench import label_map
    rng = np.random.default_rng(0)
    return (('smooth, 1 object', label_map(hw, 1)), ('smooth, 5 objects', label_map(hw, 5)),
            ('noise p = 0.5', (rng.random(hw) < 0.5).astype(np.uint8)))


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
    return f'{statistics.median(out):8.1f} us ({min(out):.1f} .. {max(out):.1f})'


def alone(emit, reps):
    import torch
    from xmem2_amd import ops
    emit(f'\n1. the launch sequences on their own (us per call; median of 7 windows of {reps} calls, with the spread)')
    for hw in SIZES:
        for name, m in masks_of(hw):
            dev = torch.from_numpy(m).cuda()
            root, area = ops.components(dev, 8)
            out = torch.empty_like(dev)
            _, stats = ops.clean_masks(dev, **SPEC, out=out)
            n_comp = int((root.view(-1) == torch.arange(root.numel(), device=root.device, dtype=torch.int32)).sum())
            emit(f'   {hw[0]:4d} x {hw[1]:4d}, {name:18s} ({n_comp:7d} components; clean: {stats.cpu().tolist()})')
            emit('        components(8)               ' + windows(lambda: ops.components(dev, 8), reps))
            emit('        clean(16, 16)               ' + windows(lambda: ops.clean_masks(dev, **SPEC, out=out), reps))
            emit('        clean(16, 16, keep_largest) ' + windows(lambda: ops.clean_masks(dev, keep_largest=True, **SPEC, out=out), reps))


def scipy_clean(m, min_area, max_hole):
    import numpy as np
    from scipy import ndimage
    out = m.copy()
    for k in np.unique(m):
        if k == 0:
            continue
        lab, n = ndimage.label(m == k, structure=np.ones((3, 3), int))
        size = ndimage.sum(np.ones_like(m), lab, np.arange(1, n + 1))
        out[np.isin(lab, 1 + np.nonzero(size < min_area)[0])] = 0
    lab, n = ndimage.label(out == 0)
    size = ndimage.sum(np.ones_like(m), lab, np.arange(1, n + 1))
    edge = np.unique(np.concatenate((lab[0], lab[-1], lab[:, 0], lab[:, -1])))
    small = np.setdiff1d(1 + np.nonzero(size <= max_hole)[0], edge)
    hole = np.isin(lab, small)
    grown = ndimage.grey_dilation(out, footprint=ndimage.generate_binary_structure(2, 1))
    out[hole] = grown[hole]                                          # one pass: right for the holes one pixel wide that an argmax has
    return out


def host(emit):
    import torch
    emit('\n3. scipy.ndimage on the host, per frame, the copy of the mask to the host included (ms; median of 5)')
    for hw in SIZES:
        for name, m in masks_of(hw):
            dev = torch.from_numpy(m).cuda()
            took = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                scipy_clean(dev.cpu().numpy(), **SPEC)
                took.append((time.perf_counter() - t0) * 1e3)
            emit(f'   {hw[0]:4d} x {hw[1]:4d}, {name:18s} {statistics.median(took):9.2f} ms ({min(took):.2f} .. {max(took):.2f})')


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
            over = {'model': model, 'size': 480, 'save_masks': False, 'save_tracks': True}
            if spec is not None:
                over['mask_cleanup'] = dict(spec)
            text = io.StringIO()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(text):
                df = run_on_video(imgs, msks, os.path.join(tmp, f'out_{n}'), frames_with_masks=[0], print_progress=False, save_overlay=False,
                                  network=net, overwrite_config=over, print_fps=True)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            loop = float(re.search(r'TOTAL PROCESSING TIME: ([0-9.]+)s', text.getvalue()).group(1))
            return loop, wall, df.attrs.get('cleanup')

        run(None, 'w0'), run(SPEC, 'w1')
        rows = {'off (parent)': [], 'on': []}
        totals = None
        for r in range(runs):
            rows['off (parent)'].append(run(None, f'off{r}')[:2])
            loop, wall, totals = run(SPEC, f'on{r}')
            rows['on'].append((loop, wall))
        emit(f'\n2. run_on_video, 480 x 854, {frames} frames, tracks only, mask_cleanup = {SPEC}: {runs} alternating runs per mode')
        emit(f'   totals of one run with the option on: {totals}')
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
    emit(f'mask clean-up on {torch.cuda.get_device_name(0)}; build digest {build.source_digest()}')
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
