"""What confidence and uncertainty maps (config['confidence'], ops.confidence_stats) cost.

    python tools/confidence_bench.py [--frames 60] [--runs 3] [--reps 200] [--only 1,2,3] [--out FILE]

1. The call on its own at 480 x 854 with C = 2 and 4 and at 1080 x 1920 with C = 6, next to `ops.argmax_u8` of the same tensor - the
   kernel it replaces in the frame loop, which reads the same bytes.  Scores: a softmax over ragged ellipses (tools/tracks_bench.py)
   blurred at their borders, so that most waves lie inside one label and the borders are unsure, as a decoder's output is.  Both
   calls are timed in the same process in alternating windows: device events around `--reps` back-to-back calls, 7 windows each after
   a warm-up, median and spread in us per call, next to the bytes the call must move over 6.3 TB/s, the rate a streaming kernel
   reaches on this part.  At these sizes the scores are resident in the caches between calls, so that floor is a bound on the kernel,
   not on what the call costs.  With and without the plane.
2. `run_on_video` on one synthetic 480 x 854 clip of `--frames` JPEG frames (the synthetic checkpoint, one network), the option off
   and on in alternating runs after a warm-up of each: the loop's own clock (TOTAL PROCESSING TIME) and a host clock round the whole
   call, which includes the PNG writers.  The option-off path is the parent commit's code.
3. `python -m xmem2_amd.session`'s loop on a clip with ground truth (--clip-images / --clip-masks; default: tests/golden/chair)
   with both --review-by rules: J&F of every round.  With synthetic weights this records that the plumbing works; it says nothing
   about which rule picks better frames.
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

CASES = (((480, 854), 2), ((480, 854), 4), ((1080, 1920), 6))
HBM_STREAM = 6.3e12                   # bytes per second


def scores_of(hw, C, seed=0):
    """float32 [C,H,W] on the device: a softmax whose winner is a ragged label map and whose borders are soft"""
    import numpy as np
    import torch
    from tracks_bench import label_map
    labels = torch.from_numpy(label_map(hw, C - 1).astype(np.int64)).cuda()
    onehot = torch.nn.functional.one_hot(labels, C).permute(2, 0, 1).float()[None]
    soft = torch.nn.functional.avg_pool2d(onehot, 9, stride=1, padding=4, count_include_pad=False)[0]
    noise = torch.rand((C,) + hw, device='cuda', generator=torch.Generator('cuda').manual_seed(seed)) * 0.05
    return torch.softmax(6.0 * soft + noise, 0).contiguous()


def window(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternating(fns, reps, n=7):
    """{name: (median, min, max)} in us per call: after a warm-up of each, n rounds of one window per function"""
    for fn in fns.values():
        for _ in range(10):
            fn()
    got = {name: [] for name in fns}
    for _ in range(n):
        for name, fn in fns.items():
            got[name].append(window(fn, reps))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def alone(emit, reps):
    import torch
    from xmem2_amd import ops
    emit(f'\n1. the call on its own (median of 7 alternating windows of {reps} calls, with the spread; floor = bytes moved / 6.3 TB/s)')
    for hw, C in CASES:
        prob = scores_of(hw, C)
        P = hw[0] * hw[1]
        record = torch.empty((C, 4), dtype=torch.int64, device='cuda')
        mask, plane = torch.empty(hw, dtype=torch.uint8, device='cuda'), torch.empty(hw, dtype=torch.uint8, device='cuda')
        res = alternating({
            'argmax_u8 (parent)': lambda: ops.argmax_u8(prob),
            'confidence_stats': lambda: ops.confidence_stats(prob, 64, record=record, mask=mask),
            'confidence_stats + plane': lambda: ops.confidence_stats(prob, 64, record=record, mask=mask, plane=plane)}, reps)
        assert torch.equal(mask, ops.argmax_u8(prob))
        rec = record.cpu().numpy()
        emit(f'   {hw[0]:4d} x {hw[1]:4d}, C = {C}: scores {4 * C * P / 1e6:6.2f} MB;  low pixels {int(rec[:, 2].sum())} of {P}')
        for name, (med, lo, hi) in res.items():
            moved = 4 * C * P + P * (2 if name.endswith('plane') else 1)
            emit(f'        {name:26s} {med:8.2f} us per call ({lo:.2f} .. {hi:.2f});   floor {1e6 * moved / HBM_STREAM:6.2f} us')
        del prob
        torch.cuda.empty_cache()


def _clip(tmp, frames):
    from session_bench import save_checkpoint
    from tracks_bench import write_clip
    model = save_checkpoint(os.path.join(tmp, 'XMem_synth.pth'))
    imgs, msks = write_clip(os.path.join(tmp, 'clip'), frames, (480, 854), 1)
    return model, imgs, msks


def video(emit, frames, runs):
    import torch
    from xmem2_amd.network import XMem
    from xmem2_amd.run_on_video import run_on_video
    with tempfile.TemporaryDirectory() as tmp:
        model, imgs, msks = _clip(tmp, frames)
        net = XMem({'model': model, 'size': 480}, model).to('cuda').eval()

        def run(option, n):
            over = {'model': model, 'size': 480}
            if option is not None:
                over['confidence'] = option
            text = io.StringIO()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(text):
                df = run_on_video(imgs, msks, os.path.join(tmp, f'out_{n}'), frames_with_masks=[0], print_progress=False, save_overlay=False,
                                  network=net, overwrite_config=over, print_fps=True)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            return float(re.search(r'TOTAL PROCESSING TIME: ([0-9.]+)s', text.getvalue()).group(1)), wall, df

        modes = {'off (parent)': None, 'on': True, 'on + maps': {'maps': True}}
        for i, option in enumerate(modes.values()):
            run(option, f'w{i}')
        rows = {tag: [] for tag in modes}
        for r in range(runs):
            for tag, option in modes.items():
                rows[tag].append(run(option, f'{len(rows[tag])}_{r}_{list(modes).index(tag)}'))
        emit(f'\n2. run_on_video, 480 x 854, {frames} frames, one object, mask PNGs written: {runs} alternating runs per mode')
        for tag, v in rows.items():
            loops, walls = [1e3 * a / frames for a, _, _ in v], [frames / b for _, b, _ in v]
            emit(f'   {tag:13s} frame loop ms/frame: ' + '  '.join(f'{a:6.3f}' for a in loops) +
                 f'   median {statistics.median(loops):6.3f} ({min(loops):.3f} .. {max(loops):.3f});   whole call frames/s: ' +
                 '  '.join(f'{b:6.1f}' for b in walls) + f'   median {statistics.median(walls):6.1f} ({min(walls):.1f} .. {max(walls):.1f})')
        conf = rows['on'][-1][2]['confidence'].to_numpy()
        emit(f'   frame confidence of the last run: min {float(conf[1:].min()):.4f}, median {float(statistics.median(conf[1:])):.4f}')


def review(emit, rounds, k, images, masks):
    """the loop of `python -m xmem2_amd.session --rounds N --review-by ...`, with J&F of every round"""
    import torch
    from session_bench import save_checkpoint
    from xmem2_amd.session import VideoSession
    with tempfile.TemporaryDirectory() as tmp:
        over = {'model': save_checkpoint(os.path.join(tmp, 'XMem_synth.pth')), 'size': 480}
        if images is None:                                           # the chair files: 10 frames at 480 x 720, every one annotated
            chair = os.path.join(ROOT, 'tests', 'golden', 'chair')
            images, masks = os.path.join(chair, 'JPEGImages'), os.path.join(chair, 'Annotations')
        emit(f'\n3. the session loop on {images}, {rounds} rounds of k = {k}: mean J and F per round.  Synthetic weights: a record that '
             'the plumbing works, not a claim about quality')
        for rule in ('dissimilarity', 'confidence'):
            s = VideoSession(images, masks, overwrite_config=dict(over, **({'confidence': True} if rule == 'confidence' else {})))
            s.save_reference(0)
            chosen = []
            for r in range(rounds):
                for t in sorted(chosen):
                    if s.frames[t].mask is not None:
                        s.save_reference(t)
                s.full_propagation()
                torch.cuda.synchronize()                             # the scorer's buffers are allocated now: nothing of the propagation may still be in flight
                df = s.stats(compute_jf=True)
                with contextlib.redirect_stdout(io.StringIO()):
                    chosen = s.review_queue(k=k) if rule == 'confidence' else s.candidates(k=k)
                emit(f'   --review-by {rule:13s} round {r}: references {s.references}  J {float(df["J"].mean()):.4f}  F {float(df["F"].mean()):.4f}  '
                     f'next {chosen}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=60)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--k', type=int, default=2)
    ap.add_argument('--clip-images', default=None)
    ap.add_argument('--clip-masks', default=None)
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
    emit(f'confidence and uncertainty maps on {torch.cuda.get_device_name(0)}; build digest {build.source_digest()}')
    if '1' in args.only:
        alone(emit, args.reps)
    if '2' in args.only:
        video(emit, args.frames, args.runs)
    if '3' in args.only:
        review(emit, args.rounds, args.k, args.clip_images, args.clip_masks)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
