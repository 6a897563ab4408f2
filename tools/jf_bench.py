"""Cost of DAVIS J&F scoring (xmem_jf_counts, xmem2_amd.metrics, run_on_video(compute_jf=True)).

    python tools/jf_bench.py [--iters 200] [--videos 30] [--video-frames 20] [--clip-frames 120] [--repeat 2]
    python tools/jf_bench.py --kernel-only            # launches only: run it under rocprofv3 --kernel-trace --stats
    python tools/jf_bench.py --kernel-stats <rocprofv3 kernel_stats.csv>

1. kernel: one xmem_jf_counts launch per frame (B = 1, the in-loop form) at 480 x 854 (radius 8) and 1080 x 1920 (radius 18) with 1, 3
   and 10 objects, timed with device events over `--iters` back-to-back launches (microseconds per frame);
2. compute_metrics over a synthetic dataset of `--videos` videos x `--video-frames` 480p frames written to PNG files (wall seconds,
   and the share spent decoding);
3. run_on_video frames/s (its own print_fps clock: the frame loop without decode, preload and writing) on one synthetic 480 x 854 clip
   with every frame annotated on disk, compute_jf off and on alternated in one process, best of `--repeat` calls each.
"""
import argparse
import contextlib
import csv
import io
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {'480p': (480, 854), '1080p': (1080, 1920)}
OBJECTS = (1, 3, 10)


def label_maps(hw, n_obj, seed):
    """A ground truth of n_obj ellipses and a prediction shifted by a few pixels."""
    rng = np.random.default_rng(seed)
    H, W = hw
    yy, xx = np.mgrid[:H, :W]
    gt = np.zeros(hw, np.uint8)
    for k in range(1, n_obj + 1):
        cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
        ry, rx = rng.uniform(0.05, 0.25) * H, rng.uniform(0.05, 0.25) * W
        gt[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = k
    return gt, np.roll(gt, (3, -4), axis=(0, 1))


def kernel_times(iters):
    import torch
    from xmem2_amd import ops
    from xmem2_amd.metrics import bound_pix
    rows = []
    for name, hw in SIZES.items():
        r = bound_pix(0.008, hw)
        for n in OBJECTS:
            gt, pred = label_maps(hw, n, 0)
            g, p = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
            out = torch.empty((1, 256, 7), dtype=torch.int32, device='cuda')
            for _ in range(10):
                ops.jf_counts(g, p, r, out=out)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                ops.jf_counts(g, p, r, out=out)
            b.record()
            b.synchronize()
            rows.append((name, hw, r, n, a.elapsed_time(b) * 1e3 / iters))
    return rows


def write_dataset(root, videos, frames, hw=(480, 854), n_obj=3):
    from PIL import Image
    pal = [0, 0, 0, 128, 0, 0, 0, 128, 0, 128, 128, 0, 0, 0, 128] + [0] * (256 * 3 - 15)
    for v in range(videos):
        gdir, pdir = os.path.join(root, 'gt', f'v{v:03d}'), os.path.join(root, 'pred', f'v{v:03d}', 'masks')
        os.makedirs(gdir); os.makedirs(pdir)
        for t in range(frames):
            gt, pred = label_maps(hw, n_obj, 1000 * v + t)
            for a, d in ((gt, gdir), (pred, pdir)):
                im = Image.fromarray(a, mode='P')
                im.putpalette(pal)
                im.save(os.path.join(d, f'{t:05d}.png'))


def metrics_wall(root):
    from concurrent.futures import ThreadPoolExecutor
    import torch
    from xmem2_amd.metrics import compute_metrics, load_video
    compute_metrics(os.path.join(root, 'gt'), os.path.join(root, 'pred'))      # warm: imports, first launch, PNG caches
    t0 = time.perf_counter()
    df = compute_metrics(os.path.join(root, 'gt'), os.path.join(root, 'pred'))
    wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(8) as pool:
        for v in sorted(os.listdir(os.path.join(root, 'pred'))):
            load_video(os.path.join(root, 'gt', v), os.path.join(root, 'pred', v, 'masks'), pool)
    decode = time.perf_counter() - t0
    torch.cuda.synchronize()
    return df, wall, decode


def write_clip(root, t, hw=(480, 854)):
    """Synthetic 480p frames with every frame's 2-object ground truth on disk (so compute_jf scores all of them)."""
    from PIL import Image
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    imgs, msks = os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations')
    os.makedirs(imgs); os.makedirs(msks)
    frames, masks = synthetic_frames(t, *hw), synthetic_masks(t, 2, *hw)
    for i in range(t):
        rgb = np.clip((frames[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(imgs, f'{i:05d}.jpg'), quality=95)
        idx = np.zeros(hw, np.uint8)
        idx[masks[i, 0] > 0.5] = 1
        idx[masks[i, 1] > 0.5] = 2
        im = Image.fromarray(idx, mode='P')
        im.putpalette([0, 0, 0, 200, 0, 0, 0, 200, 0] + [0] * (256 * 3 - 9))
        im.save(os.path.join(msks, f'{i:05d}.png'))
    return imgs, msks


def loop_fps(imgs, msks, out, model, compute_jf):
    from xmem2_amd.run_on_video import run_on_video
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        df = run_on_video(imgs, msks, out, frames_with_masks=[0], print_progress=False, print_fps=True, compute_jf=compute_jf,
                          overwrite_config={'model': model})
    return float(re.search(r'TOTAL PROCESSING FPS: ([0-9.]+)', buf.getvalue()).group(1)), df


def kernel_report(path):
    rows = [r for r in csv.DictReader(open(path)) if 'jf_counts' in r['Name']]
    if not rows:
        print(f'no jf_counts launches in {path}')
        return
    for r in rows:
        print(f'   {r["Name"].split("(")[0].replace("void ", "")[:40]:40s} calls {int(r["Calls"]):6d}  avg {float(r["AverageNs"]) / 1e3:7.2f} us'
              f'  min {float(r["MinNs"]) / 1e3:7.2f}  max {float(r["MaxNs"]) / 1e3:7.2f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--videos', type=int, default=30)
    ap.add_argument('--video-frames', type=int, default=20)
    ap.add_argument('--clip-frames', type=int, default=120)
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_report(args.kernel_stats)
        return
    import torch
    torch.set_grad_enabled(False)
    print(f'device {torch.cuda.get_device_name(0)}')
    print(f'\n1. xmem_jf_counts, one frame per launch, {args.iters} back-to-back launches (device events):')
    for name, hw, r, n, us in kernel_times(args.iters):
        print(f'   {name:6s} {hw[0]}x{hw[1]} radius {r:2d}  {n:2d} object(s)  {us:8.2f} us per frame', flush=True)
    if args.kernel_only:
        return
    with tempfile.TemporaryDirectory() as tmp:
        write_dataset(os.path.join(tmp, 'ds'), args.videos, args.video_frames)
        df, wall, decode = metrics_wall(os.path.join(tmp, 'ds'))
        n = args.videos * args.video_frames
        print(f'\n2. compute_metrics over {args.videos} videos x {args.video_frames} frames 480x854 (3 objects), PNG files: {wall:.3f} s '
              f'({n / wall:.1f} frames/s); decoding alone {decode:.3f} s = {100 * decode / wall:.0f} %; mean J {df["iou"].mean():.4f} '
              f'F {df["f"].mean():.4f}', flush=True)
        from xmem2_amd.synth import synthetic_state_dict
        model = os.path.join(tmp, 'XMem_synth.pth')
        torch.save(synthetic_state_dict(0), model)
        imgs, msks = write_clip(os.path.join(tmp, 'clip'), args.clip_frames)
        fps = {False: [], True: []}
        for i in range(args.repeat):
            for flag in (False, True):
                f, df = loop_fps(imgs, msks, os.path.join(tmp, f'out{i}{int(flag)}'), model, flag)
                fps[flag].append(f)
        off, on = max(fps[False]), max(fps[True])
        print(f'\n3. run_on_video, synthetic 480x854 clip, {args.clip_frames} frames, every frame with a ground truth; processing frames/s '
              f'(alternated off/on, best of {args.repeat}): off {off:.1f} (all {", ".join(f"{x:.1f}" for x in fps[False])}), '
              f'on {on:.1f} (all {", ".join(f"{x:.1f}" for x in fps[True])}) -> on / off {on / off:.3f}; '
              f'in-loop mean J {np.nanmean(df["J"]):.4f} F {np.nanmean(df["F"]):.4f}')


if __name__ == '__main__':
    main()
