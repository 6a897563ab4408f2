"""What the block-motion search and the motion-compensated vote (config['temporal_smooth'] with 'motion') cost.

    python tools/motion_bench.py [--frames 60] [--runs 3] [--reps 20] [--only 1,2,3,4] [--out FILE]

1. One `ops.block_motion` pair at 480 x 854 and 1080 x 1920 for search 8, 16 and 32, on a smooth texture that pans by (2, -3) with a
   little noise: device events around `--reps` back-to-back calls, 7 such windows after a warm-up (tools/temporal_bench.py's
   `windows`): median and spread, next to the byte differences the search takes (every in-bounds candidate of every block) and the
   time their pure v_sad_u8 issue would take at an ASSUMED full rate: 4 bytes per lane and instruction, 64 lanes, 4 SIMDs on each of
   256 CUs at 2.4 GHz, one instruction per cycle.  The instruction's real rate is not measured.
2. `ops.temporal_mode_mc_ring` - `motion_window` plus the vote - per frame for r = 1, 2 and 3 at 480 x 854, search 16: one frame per
   call from a ring of 2 r + 1 slots, as the frame loop calls it, and 32 frames per call.
3. `run_on_video` on one synthetic 480 x 854 clip of `--frames` frames at the source size (the synthetic checkpoint, one network):
   the key off, the plain vote (radius 1) and the compensated vote (radius 1) in alternating runs after a warm-up of each.
4. For scale: `temporal.mode_mc_host` on this machine's host, 480 x 854, r = 1, search 16, three frames.
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

from temporal_bench import SIZES, clip_of, windows      # noqa: E402

SEARCHES = (8, 16, 32)
RADII = (1, 2, 3)
SAD_BYTES_PER_SECOND = 4 * 64 * 4 * 256 * 2.4e9      # ASSUMES v_sad_u8 issues every cycle on every SIMD; its rate is not measured


def panning_lumas(hw, n):
    """uint8 [n,H,W]: a smooth texture that pans by (2, -3) a frame, with noise of +-2"""
    import numpy as np
    from xmem2_amd.synth import _smooth_field
    H, W = hw
    rng = np.random.default_rng(n)
    field = _smooth_field(H + 2 * n, W + 3 * n, 7, passes=2, radius=3)
    field = (255 * (field - field.min()) / (field.max() - field.min())).astype(np.int32)
    out = np.stack([field[2 * (n - 1 - t):2 * (n - 1 - t) + H, 3 * t:3 * t + W] for t in range(n)])
    return (out + rng.integers(-2, 3, out.shape)).clip(0, 255).astype(np.uint8)


def candidates(hw, S):
    """byte differences of one pair: over the blocks, pixels times in-bounds candidates - a product of a sum over the block rows and
    one over the block columns"""
    import numpy as np

    def along(n):
        starts = np.arange(0, n, 16)
        ends = np.minimum(starts + 16, n)
        return int(((ends - starts) * (np.minimum(S, starts) + np.minimum(S, n - ends) + 1)).sum())
    return along(hw[0]) * along(hw[1])


def pairs(emit, reps):
    import torch
    from xmem2_amd import ops
    emit(f'\n1. one block_motion pair (median of 7 windows of {reps} calls, with the spread; issue = byte differences / v_sad_u8 rate)')
    for hw in SIZES:
        lumas = torch.from_numpy(panning_lumas(hw, 2)).cuda()
        for S in SEARCHES:
            vec, sad = ops.block_motion(lumas[0], lumas[1], S, 1)
            med, lo, hi = windows(lambda: ops.block_motion(lumas[0], lumas[1], S, 1, vec=vec, sad=sad), reps)
            work = candidates(hw, S)
            moving = float((vec != 0).any(-1).float().mean())
            emit(f'   {hw[0]:4d} x {hw[1]:4d}, search {S:2d}: {med:9.1f} us ({lo:.1f} .. {hi:.1f});   {work / 1e6:9.1f} M byte differences, '
                 f'issue {1e6 * work / SAD_BYTES_PER_SECOND:6.1f} us;   blocks that move {100 * moving:.0f} %')


def votes(emit, reps):
    import torch
    from xmem2_amd import ops
    hw = SIZES[0]
    emit(f'\n2. motion_window + vote at {hw[0]} x {hw[1]}, search 16 (median of 7 windows, with the spread)')
    for n in (1, 32):
        for r in RADII:
            T = n + 2 * r
            lumas = torch.from_numpy(panning_lumas(hw, T)).cuda()
            masks = torch.from_numpy(clip_of(hw, T, 'masks')).cuda()
            flags = torch.ones(T, dtype=torch.uint8, device='cuda')
            out = torch.empty((n,) + hw, dtype=torch.uint8, device='cuda')
            changed = torch.empty(n, dtype=torch.int32, device='cuda')
            vec, sad = ops.motion_window(lumas, T, r, n, r, flags)
            both = lambda: ops.temporal_mode_mc_ring(masks, lumas, T, r, n, r, flags, out=out, changed=changed, vec=vec, sad=sad)
            search = lambda: ops.motion_window(lumas, T, r, n, r, flags, vec=vec, sad=sad)
            med, lo, hi = windows(both, max(1, reps // n))
            only, _, _ = windows(search, max(1, reps // n))
            emit(f'        batch {n:2d}, r = {r}: {med:9.1f} us per call ({lo:.1f} .. {hi:.1f}), {med / n:8.1f} us per frame, of which the '
                 f'search {only / n:8.1f};   pixels changed per frame {int(changed.sum()) // n}')
            del lumas, masks, out
            torch.cuda.empty_cache()


def host(emit):
    from xmem2_amd import temporal
    hw = SIZES[0]
    lumas, masks = panning_lumas(hw, 3), clip_of(hw, 3, 'masks')
    t0 = time.perf_counter()
    temporal.mode_mc_host(masks, lumas, 1)
    emit(f'\n4. temporal.mode_mc_host on this machine\'s host, {hw[0]} x {hw[1]}, r = 1, search 16, 3 frames (4 pairs): '
         f'{(time.perf_counter() - t0) / 3:.2f} s per frame')


def video(emit, frames, runs):
    import torch
    from session_bench import save_checkpoint
    from tracks_bench import write_clip
    from xmem2_amd.network import XMem
    from xmem2_amd.run_on_video import run_on_video
    modes = {'off (parent)': None, 'plain vote': 1, 'compensated': {'radius': 1, 'motion': True}}
    with tempfile.TemporaryDirectory() as tmp:
        model = save_checkpoint(os.path.join(tmp, 'XMem_synth.pth'))
        net = XMem({'model': model, 'size': -1}, model).to('cuda').eval()
        imgs, msks = write_clip(os.path.join(tmp, 'clip'), frames, (480, 854), 1)

        def run(smooth, n):
            over = {'model': model, 'size': -1}
            if smooth is not None:
                over['temporal_smooth'] = smooth
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

        for i, smooth in enumerate(modes.values()):
            run(smooth, f'w{i}')
        rows = {tag: [] for tag in modes}
        for r in range(runs):
            for tag, smooth in modes.items():
                rows[tag].append(run(smooth, f'{list(modes).index(tag)}_{r}'))
        emit(f'\n3. run_on_video, 480 x 854 at the source size, {frames} frames, one object, mask PNGs written: {runs} alternating runs per mode')
        med = {}
        for tag, v in rows.items():
            loops, walls = [a for a, _, _ in v], [b for _, b, _ in v]
            med[tag] = statistics.median(loops)
            emit(f'   {tag:13s} frame loop ms/frame: ' + '  '.join(f'{1e3 * a / frames:6.3f}' for a in loops) +
                 f'   median {1e3 * med[tag] / frames:6.3f} ({frames / med[tag]:6.1f} frames/s);   whole call frames/s median '
                 f'{frames / statistics.median(walls):6.1f}')
        for tag in ('plain vote', 'compensated'):
            emit(f'   {tag} - off, difference of the medians: {1e6 * (med[tag] - med["off (parent)"]) / frames:.1f} us per frame')
            emit('   ' + rows[tag][-1][2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=60)
    ap.add_argument('--runs', type=int, default=3)
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
    emit(f'block motion and the compensated vote on {torch.cuda.get_device_name(0)}; build digest {build.source_digest()}')
    for key, part in (('1', lambda: pairs(emit, args.reps)), ('2', lambda: votes(emit, args.reps)),
                      ('3', lambda: video(emit, args.frames, args.runs)), ('4', lambda: host(emit))):
        if key in args.only.split(','):
            part()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
