"""What a network that outlives a call, and a session that keeps a video on the device, save.

    python tools/session_bench.py launch [--clips 30] [--long-frames 400] [--runs 2]
    python tools/session_bench.py rounds [--frames 100] [--rounds 3] [--k 3] [--runs 3]

Every input is generated from a seed and written as JPEG files (nothing outside the repository is read); the checkpoint is the synthetic
one, saved to a file so that every process loads the same weights.

launch  seconds per video through `python -m xmem2_amd.launch --gpus 1`, with and without `--fresh-network-per-video` (the behaviour
        before the network was shared), alternating, `--runs` each: on ONE synthetic 480p clip of `--long-frames` frames and on
        `--clips` clips of 50-100 frames.  The per-video seconds are the launcher's own (summary.json); the wall time of the whole
        command (process start, torch import, network build included) is printed next to them.
rounds  seconds per annotate -> propagate -> select round on one 480p clip: through `VideoSession` (save_reference, full_propagation,
        candidates) and through the file API the parent commit offers for the same round - `run_on_video` (masks written, no
        overlays) + `select_k_next_best_annotation_candidates(use_previously_predicted_masks=True)`, each call building its own
        network as it did there.  The two alternate within a run; every figure is a host clock around work that ends in a device
        synchronise or in files on disk.  The session's one-off cost (decode + upload of the clip, its first captures) is printed
        separately: it is paid once per video, not per round.  The file API with a shared network (`network=net`) is timed too.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HW = (480, 854)


def write_clip(root, t, seed):
    """`t` JPEG frames of a seeded moving texture and a palette annotation for EVERY frame (an ellipse that moves with it)."""
    import numpy as np
    from PIL import Image
    from resize_ingest_bench import seeded_frame
    imgs, msks = os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations')
    os.makedirs(imgs); os.makedirs(msks)
    yy, xx = np.mgrid[0:HW[0], 0:HW[1]]
    for i in range(t):
        Image.fromarray(seeded_frame(HW, seed, shift=2 * i)).save(os.path.join(imgs, f'{i:05d}.jpg'), quality=90)
        cx = HW[1] / 2 + 1.5 * i - 0.75 * t
        idx = ((((yy - HW[0] / 2) / (HW[0] / 5)) ** 2 + ((xx - cx) / (HW[1] / 6)) ** 2) <= 1).astype(np.uint8)
        im = Image.fromarray(idx, mode='P')
        im.putpalette([0, 0, 0, 200, 0, 0] + [0] * (256 * 3 - 6))
        im.save(os.path.join(msks, f'{i:05d}.png'))
    return imgs, msks


def save_checkpoint(path):
    import torch
    from xmem2_amd.synth import synthetic_state_dict
    torch.save(synthetic_state_dict(0), path)
    return path


def _launch(videos, masks, out, model, fresh):
    cmd = [sys.executable, '-m', 'xmem2_amd.launch', '--gpus', '1', '--videos', videos, '--masks', masks, '--out', out,
           '--frames-with-masks', '0', '--config', json.dumps({'model': model, 'size': 480})]
    if fresh:
        cmd.append('--fresh-network-per-video')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, env=env, cwd=ROOT, stdout=subprocess.DEVNULL)
    wall = time.perf_counter() - t0
    summ = json.load(open(os.path.join(out, 'summary.json')))
    return wall, [v['seconds'] for v in summ['videos']], summ['total_frames']


def launch_mode(n_clips, long_frames, runs):
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        model = save_checkpoint(os.path.join(tmp, 'XMem_synth.pth'))
        lengths = [int(v) for v in np.random.default_rng(3).integers(50, 101, size=n_clips)]
        sets = {}
        for name, lens in ((f'one clip of {long_frames} frames', [long_frames]), (f'{n_clips} clips of 50-100 frames', lengths)):
            root = os.path.join(tmp, 'set%d' % len(sets))
            for i, n in enumerate(lens):
                imgs, msks = write_clip(os.path.join(root, 'tmp%d' % i), n, seed=11 + i)
                for sub, src in (('JPEGImages', imgs), ('Annotations', msks)):
                    os.makedirs(os.path.join(root, sub), exist_ok=True)
                    os.rename(src, os.path.join(root, sub, f'vid{i:02d}'))
            sets[name] = root
        print('python -m xmem2_amd.launch --gpus 1, 480p JPEG clips, masks written (no overlays are part of the launcher); '
              'seconds per video are the launcher\'s own', flush=True)
        for name, root in sets.items():
            res = {False: [], True: []}
            for r in range(runs):
                for fresh in (True, False):
                    res[fresh].append(_launch(os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations'),
                                              os.path.join(tmp, f'out_{len(res[fresh])}_{int(fresh)}'), model, fresh))
            print(f'\n{name}')
            for fresh in (True, False):
                label = '--fresh-network-per-video (a network per video, as before)' if fresh else 'one network per rank (default)              '
                for wall, secs, frames in res[fresh]:
                    print(f'   {label}  mean {sum(secs) / len(secs):6.3f} s/video  (min {min(secs):.3f} max {max(secs):.3f}, first '
                          f'{secs[0]:.3f})  sum {sum(secs):7.2f} s for {frames} frames; whole command {wall:7.2f} s', flush=True)


def rounds_mode(frames, rounds, k, runs):
    import torch
    from xmem2_amd.network import XMem
    from xmem2_amd.run_on_video import run_on_video, select_k_next_best_annotation_candidates
    from xmem2_amd.session import VideoSession
    torch.set_grad_enabled(False)
    with tempfile.TemporaryDirectory() as tmp:
        model = save_checkpoint(os.path.join(tmp, 'XMem_synth.pth'))
        imgs, msks = write_clip(os.path.join(tmp, 'clip'), frames, seed=5)
        cfg = {'model': model, 'size': 480}
        print(f'device {torch.cuda.get_device_name(0)}; one 480p JPEG clip of {frames} frames, {rounds} rounds of annotate -> propagate '
              f'-> select (k = {k}) per run, {runs} runs, the two paths alternating; seconds per round', flush=True)

        def file_round(refs, out, network):
            t0 = time.perf_counter()
            run_on_video(imgs, msks, out, frames_with_masks=refs, print_progress=False, save_overlay=False, overwrite_config=dict(cfg),
                         network=network)
            new = select_k_next_best_annotation_candidates(imgs, msks, out, k=k, print_progress=False, previously_chosen_candidates=refs,
                                                           use_previously_predicted_masks=True, overwrite_config=dict(cfg), network=network)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, new

        shared = XMem(dict(cfg), model).to('cuda').eval()
        for r in range(runs):
            # the file API, a network per call (the parent commit's only way)
            refs, times_files = [0], []
            for i in range(rounds):
                dt, new = file_round(refs, os.path.join(tmp, f'files_{r}_{i}'), None)
                times_files.append(dt); refs = sorted(set(refs) | set(new))
            chosen_files = refs
            # the file API on one network
            refs, times_shared = [0], []
            for i in range(rounds):
                dt, new = file_round(refs, os.path.join(tmp, f'shared_{r}_{i}'), shared)
                times_shared.append(dt); refs = sorted(set(refs) | set(new))
            # the session
            t0 = time.perf_counter()
            s = VideoSession(imgs, msks, overwrite_config=dict(cfg), network=shared)
            torch.cuda.synchronize()
            setup = time.perf_counter() - t0
            new, times_session = [0], []
            for i in range(rounds):
                t0 = time.perf_counter()
                for t in sorted(new):
                    s.save_reference(t)
                s.full_propagation()
                new = s.candidates(k=k, mask_form='files')
                torch.cuda.synchronize()
                times_session.append(time.perf_counter() - t0)
            chosen_session = sorted(set(s.references) | set(new))
            t0 = time.perf_counter()
            s.save(os.path.join(tmp, f'session_{r}'), save_overlay=False)
            save = time.perf_counter() - t0
            fmt = lambda ts: ' '.join(f'{v:7.3f}' for v in ts)
            print(f'\nrun {r}')
            print(f'   run_on_video + select_k_next_best..., a network per call   {fmt(times_files)}')
            print(f'   the same on one network (network=net)                      {fmt(times_shared)}')
            print(f'   VideoSession (save_reference, full_propagation, candidates) {fmt(times_session)}   '
                  f'once per video: construction {setup:.3f} s, save() of {frames} masks {save:.3f} s')
            print(f'   frames chosen after {rounds} rounds: files {chosen_files}, session {chosen_session}', flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('mode', choices=['launch', 'rounds'])
    ap.add_argument('--clips', type=int, default=30)
    ap.add_argument('--long-frames', type=int, default=400)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--runs', type=int, default=2)
    args = ap.parse_args()
    if args.mode == 'launch':
        launch_mode(args.clips, args.long_frames, args.runs)
    else:
        rounds_mode(args.frames, args.rounds, args.k, args.runs)


if __name__ == '__main__':
    main()
