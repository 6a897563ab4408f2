"""Frame ingest: what the device resize (`ops.resize_u8`, config['resize_on_device']) costs and what it replaces.

    python tools/resize_ingest_bench.py stage [--case 1080p|2160p|ensemble ...] [--reps 50]
    python tools/resize_ingest_bench.py video [--frames 200] [--runs 3] [--cpus 8]
    python tools/resize_ingest_bench.py --kernel-stats <rocprofv3 kernel_stats.csv>

Every input is generated from a seed, written as JPEG files and decoded again (nothing outside the repository is read).

stage   per case (1080 x 1920 -> 480 x 853, 2160 x 3840 -> 480 x 853, and the four ensemble variants {480, 600} x {plain, flip} of
        one 1080p frame): the H2D copy of the pinned source frame and the resize launches between HIP events on one stream (back to
        back, so launch gaps are included), and the single-thread host time of the Pillow resize (+ numpy mirror) they replace.
        The kernels' own durations come from a run of their own:
            rocprofv3 --kernel-trace --stats -- python tools/resize_ingest_bench.py stage --case 1080p
        (one case per run: the stats file groups by kernel name, so the `ensemble` case's figures are averages over its 480- and
        600-row variants), summarised by `--kernel-stats`.
video   `run_on_video` and `run_on_video_ensemble` ({480, 600} x flip) on a 1080p JPEG clip at decode_workers=8 with the process
        confined to `--cpus` CPUs (what launch.pin_rank leaves a rank), option off and on alternating in one call, `--runs` each:
        the harness's own 'WALL-CLOCK FPS of the frame loop incl. decode' and 'TOTAL PROCESSING FPS' lines.
"""
import argparse
import contextlib
import csv
import functools
import io
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {'1080p': ((1080, 1920), [((480, 853), False)]),
         '2160p': ((2160, 3840), [((480, 853), False)]),
         'ensemble': ((1080, 1920), [((480, 853), False), ((480, 853), True), ((600, 1066), False), ((600, 1066), True)])}
ENSEMBLE = [[480, False], [480, True], [600, False], [600, True]]


@functools.lru_cache(maxsize=2)
def _texture(hw, seed):
    import numpy as np
    from PIL import Image
    h, w = hw
    coarse = np.random.default_rng(seed).integers(0, 256, size=(h // 40 + 2, w // 40 + 8, 3), dtype=np.uint8)
    return np.array(Image.fromarray(coarse).resize((w + 320, h), Image.BICUBIC), dtype=np.int16)


def seeded_frame(hw, seed, shift=0):
    """A smooth seeded texture (blow-up of a coarse random grid) shifted by `shift` px, plus seeded pixel noise: uint8 H x W x 3."""
    import numpy as np
    h, w = hw
    big = _texture(tuple(hw), seed)
    noise = np.random.default_rng(seed * 7919 + shift).integers(-12, 13, size=(h, w, 3), dtype=np.int16)
    return np.clip(big[:, shift % 320:shift % 320 + w] + noise, 0, 255).astype(np.uint8)


def write_clip(root, t, hw, seed=7):
    import numpy as np
    from PIL import Image
    imgs, msks = os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations')
    os.makedirs(imgs); os.makedirs(msks)
    for i in range(t):
        Image.fromarray(seeded_frame(hw, seed, shift=i)).save(os.path.join(imgs, f'{i:05d}.jpg'), quality=90)
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]]
    idx = ((((yy - hw[0] / 2) / (hw[0] / 5)) ** 2 + ((xx - hw[1] / 2) / (hw[1] / 6)) ** 2) <= 1).astype(np.uint8)
    im = Image.fromarray(idx, mode='P')
    im.putpalette([0, 0, 0, 200, 0, 0] + [0] * (256 * 3 - 6))
    im.save(os.path.join(msks, '00000.png'))
    return imgs, msks


def stage(cases, reps):
    import numpy as np
    import torch
    from PIL import Image
    from xmem2_amd import ops
    torch.set_num_threads(1)
    print(f'device {torch.cuda.get_device_name(0)}; {reps} repetitions per figure; Pillow {Image.__version__}')
    with tempfile.TemporaryDirectory() as tmp:
        for name in cases:
            src_hw, variants = CASES[name]
            path = os.path.join(tmp, name + '.jpg')
            Image.fromarray(seeded_frame(src_hw, 3)).save(path, quality=90)
            pil = Image.open(path).convert('RGB')
            host = torch.from_numpy(np.array(pil, dtype=np.uint8)).pin_memory()
            dev = host.to('cuda')
            outs = [torch.empty(hw + (3,), dtype=torch.uint8, device='cuda') for hw, _ in variants]
            for (hw, f), o in zip(variants, outs):                     # tables uploaded, allocator warm; the result is the host's
                ops.resize_u8(dev, hw, flip=f, out=o)
                want = np.array(pil.resize((hw[1], hw[0]), Image.BILINEAR), dtype=np.uint8)
                assert np.array_equal(o.cpu().numpy(), want[:, ::-1] if f else want), 'device resize differs from Pillow'

            def events(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / reps * 1e3

            copy_us = events(lambda: dev.copy_(host, non_blocking=True))
            resize_us = events(lambda: [ops.resize_u8(dev, hw, flip=f, out=o) for (hw, f), o in zip(variants, outs)])
            n_host = max(3, reps // 5)
            t0 = time.perf_counter()
            for _ in range(n_host):
                by_size = {}
                for hw, f in variants:                                   # as EnsembleFramePrefetcher: one resize per size, numpy mirror
                    if hw not in by_size:
                        by_size[hw] = np.array(pil.resize((hw[1], hw[0]), Image.BILINEAR), dtype=np.uint8)
                    if f:
                        np.ascontiguousarray(by_size[hw][:, ::-1])
            host_us = (time.perf_counter() - t0) / n_host * 1e6
            mb = host.numel() / 1e6
            print(f'{name:9s} source {src_hw[0]} x {src_hw[1]} ({mb:.1f} MB) -> ' + ', '.join(f'{hw[0]} x {hw[1]}' + (' flip' if f else '')
                                                                                               for hw, f in variants))
            print(f'   H2D copy of the pinned source frame      {copy_us:9.1f} us  ({mb / copy_us * 1e3:.1f} GB/s)')
            print(f'   resize launches, back to back (events)   {resize_us:9.1f} us  for {len(variants)} variant(s)')
            print(f'   Pillow resize (+ mirror), one host thread {host_us:8.1f} us', flush=True)


def kernel_report(path):
    rows = [r for r in csv.DictReader(open(path)) if re.search(r'resize_[hv]_kernel|copy_mirror_kernel', r['Name'])]
    if not rows:
        print(f'no resize launches in {path}')
        return
    for r in rows:
        short = re.search(r'resize_[hv]_kernel|copy_mirror_kernel', r['Name']).group(0)
        print(f'   {short:20s} calls {int(r["Calls"]):5d}  avg {float(r["AverageNs"]) / 1e3:7.2f} us  min {float(r["MinNs"]) / 1e3:7.2f}  '
              f'max {float(r["MaxNs"]) / 1e3:7.2f}')


def video(frames, runs, cpus):
    import torch
    from xmem2_amd.run_on_video import run_on_video, run_on_video_ensemble
    from xmem2_amd.synth import synthetic_state_dict
    if hasattr(os, 'sched_setaffinity'):
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:cpus])
    torch.set_num_threads(min(cpus, 8))
    torch.set_grad_enabled(False)
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, 'XMem_synth.pth')
        torch.save(synthetic_state_dict(0), model)
        imgs, msks = write_clip(os.path.join(tmp, 'clip'), frames, (1080, 1920))
        print(f'device {torch.cuda.get_device_name(0)}; {frames} JPEG frames of 1080 x 1920, working size 480; decode_workers 8, '
              f'{len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else "?"} CPUs; masks are not written', flush=True)
        for title, fn, extra in (('run_on_video', run_on_video, {}),
                                 ('run_on_video_ensemble {480, 600} x flip', run_on_video_ensemble, {'ensemble': ENSEMBLE})):
            res = {False: [], True: []}
            for r in range(runs):
                for on in (False, True):
                    buf = io.StringIO()
                    with contextlib.redirect_stdout(buf):
                        fn(imgs, msks, os.path.join(tmp, 'out'), frames_with_masks=[0], print_progress=False, print_fps=True,
                           save_overlay=False, overwrite_config=dict(extra, model=model, size=480, decode_workers=8, save_masks=False,
                                                                     resize_on_device=on))
                    txt = buf.getvalue()
                    res[on].append((float(re.search(r'incl\. decode: ([0-9.]+)', txt).group(1)),
                                    float(re.search(r'TOTAL PROCESSING FPS: ([0-9.]+)', txt).group(1))))
            print(f'\n{title}')
            for on in (False, True):
                wall, proc = [a for a, _ in res[on]], [b for _, b in res[on]]
                print(f'   resize_on_device {"on " if on else "off"}  wall-clock frames/s incl. decode: ' + ' '.join(f'{v:7.1f}' for v in wall)
                      + f'  (min {min(wall):.1f} max {max(wall):.1f})   TOTAL PROCESSING FPS: ' + ' '.join(f'{v:7.1f}' for v in proc)
                      + f'  (min {min(proc):.1f} max {max(proc):.1f})', flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('mode', nargs='?', choices=['stage', 'video'])
    ap.add_argument('--case', nargs='*', default=None, choices=sorted(CASES))
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--cpus', type=int, default=8)
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_report(args.kernel_stats)
    elif args.mode == 'stage':
        stage(args.case or ['1080p', '2160p', 'ensemble'], args.reps)
    elif args.mode == 'video':
        video(args.frames, args.runs, args.cpus)
    else:
        ap.error('choose a mode: stage, video or --kernel-stats FILE')


if __name__ == '__main__':
    main()
