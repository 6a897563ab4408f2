"""Frame rate of the test-time ensemble (xmem2_amd.run_on_video.run_on_video_ensemble) against its passes run alone.

    python tools/ensemble_fps.py [--frames 120] [--repeat 2] [--only NAME ...]
    python tools/ensemble_fps.py --kernel-stats <rocprofv3 kernel_stats.csv> --passes-frames N

On the chair files (tests/golden/chair, 10 frames at 480 x 720) and on a longer synthetic 480 x 854 clip written to JPEG files, it times
with the harness's own clock (`print_fps`: the frame loop without decode, preload and writing) each of

    single    run_on_video at size 480 (the usual single pass)
    s480 / s600 / s480f / s600f    each pass of the 4-pass ensemble run alone (run_on_video_ensemble with that one pass)
    ens2      the default flip ensemble [[480, no flip], [480, flip]]
    ens4      {480, 600} x {no flip, flip}

and prints frames/s, the sum-of-passes expectation (1 / sum of 1/fps of the passes alone) and the ratio.  Every call builds its own
network, so the first frames of every call include its graph captures; `--repeat` keeps the best of several calls.

Under `rocprofv3 --kernel-trace --stats -- python tools/ensemble_fps.py --only ens4 --repeat 1`, the merge kernel's launches are in the
kernel_stats.csv; `--kernel-stats` turns that file into microseconds per pass per frame.
"""
import argparse
import contextlib
import csv
import io
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PASSES = {'s480': [[480, False]], 's480f': [[480, True]], 's600': [[600, False]], 's600f': [[600, True]],
          'ens2': [[480, False], [480, True]], 'ens4': [[480, False], [480, True], [600, False], [600, True]]}
ALONE = {'ens2': ['s480', 's480f'], 'ens4': ['s480', 's480f', 's600', 's600f']}


def write_synthetic_clip(root, t, hw=(480, 854)):
    import numpy as np
    from PIL import Image
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    imgs, msks = os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations')
    os.makedirs(imgs); os.makedirs(msks)
    frames, masks = synthetic_frames(t, *hw), synthetic_masks(1, 2, *hw)
    for i in range(t):
        rgb = np.clip((frames[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(imgs, f'{i:05d}.jpg'), quality=95)
    idx = (masks[0, 0] * 1 + masks[0, 1] * 2).astype(np.uint8)
    im = Image.fromarray(idx, mode='P')
    im.putpalette([0, 0, 0, 200, 0, 0, 0, 200, 0] + [0] * (256 * 3 - 9))
    im.save(os.path.join(msks, '00000.png'))
    return imgs, msks


def timed(name, imgs, msks, out, model):
    """Processing frames/s of one call (the harness's print_fps line)."""
    from xmem2_amd.run_on_video import run_on_video, run_on_video_ensemble
    over = {'model': model}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        if name == 'single':
            run_on_video(imgs, msks, out, frames_with_masks=[0], print_progress=False, print_fps=True, overwrite_config=over)
        else:
            run_on_video_ensemble(imgs, msks, out, frames_with_masks=[0], print_progress=False, print_fps=True,
                                  overwrite_config=dict(over, ensemble=PASSES[name]))
    m = re.search(r'TOTAL PROCESSING FPS: ([0-9.]+)', buf.getvalue())
    return float(m.group(1))


def kernel_report(path, frames_passes):
    rows = [r for r in csv.DictReader(open(path)) if 'ensemble_accumulate' in r['Name']]
    if not rows:
        print(f'no ensemble_accumulate launches in {path}')
        return
    n = sum(int(r['Calls']) for r in rows)
    tot = sum(int(r['Calls']) * float(r['AverageNs']) for r in rows)
    print(f'merge kernel (ensemble_accumulate_kernel): {n} launches, {tot / n / 1e3:.2f} us per launch (= per pass per frame) on average'
          + (f'; expected launches {frames_passes}' if frames_passes else ''))
    for r in rows:
        short = r['Name'].split('(')[0].replace('void ', '')
        print(f'   {short[:60]:60s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:7.2f} us  '
              f'min {float(r["MinNs"]) / 1e3:7.2f}  max {float(r["MaxNs"]) / 1e3:7.2f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=120, help='length of the synthetic 480p clip')
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--only', nargs='*', default=None)
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--passes-frames', type=int, default=0)
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_report(args.kernel_stats, args.passes_frames)
        return
    import torch
    from xmem2_amd.synth import synthetic_state_dict
    torch.set_grad_enabled(False)
    names = args.only or ['single', 's480', 's480f', 's600', 's600f', 'ens2', 'ens4']
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, 'XMem_synth.pth')
        torch.save(synthetic_state_dict(0), model)
        chair = os.path.join(ROOT, 'tests', 'golden', 'chair')
        clips = [('chair 480x720, 10 frames', os.path.join(chair, 'JPEGImages'), os.path.join(chair, 'Annotations'))]
        clips.append((f'synthetic 480x854, {args.frames} frames',) + write_synthetic_clip(os.path.join(tmp, 'synth'), args.frames))
        print(f'device {torch.cuda.get_device_name(0)}; processing frames/s (frame loop, no decode / preload / writing), '
              f'best of {args.repeat} calls')
        for title, imgs, msks in clips:
            fps = {}
            for n in names:
                fps[n] = max(timed(n, imgs, msks, os.path.join(tmp, 'out', n), model) for _ in range(args.repeat))
            print(f'\n{title}')
            for n in names:
                line = f'   {n:8s} {len(PASSES.get(n, [0])):2d} pass(es)  {fps[n]:8.1f} frames/s'
                if n in ALONE and all(a in fps for a in ALONE[n]):
                    expect = 1.0 / sum(1.0 / fps[a] for a in ALONE[n])
                    line += f'   sum of its passes alone {expect:7.1f} frames/s -> ensemble / sum {fps[n] / expect:.3f}'
                print(line, flush=True)


if __name__ == '__main__':
    main()
