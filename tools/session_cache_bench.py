"""What the session's feature cache (config['session_feature_cache_bytes']) saves per re-propagation.

    python tools/session_cache_bench.py [--frames 100] [--rounds 6] [--objects 1,3] [--out FILE]

Per object count one synthetic 480p clip (seeded JPEG frames, nothing outside the repository is read; the synthetic checkpoint) and two
`VideoSession`s on ONE network: cache off - the parent commit's re-propagation, the yardstick - and cache on with a budget for the whole
clip.  Round 1 of both (captures, the cache being filled) is printed but not compared.  Rounds 2.. alternate off / on in one process;
each figure is a host clock around `full_propagation()` ending in a device synchronise.  Then the masks of the two sessions are
compared, and the copy launches are timed on their own (device events around `--reps` back-to-back launches of one frame's entry,
nothing else running): restore = entry -> buffers shaped like the key stage's outputs, save = the way back.  No figure is asserted."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HW = (480, 854)


def write_clip(root, t, seed, n_obj):
    """`t` JPEG frames of a seeded moving texture and a palette annotation of `n_obj` ellipses that move with it."""
    import numpy as np
    from PIL import Image
    from resize_ingest_bench import seeded_frame
    imgs, msks = os.path.join(root, 'JPEGImages'), os.path.join(root, 'Annotations')
    os.makedirs(imgs); os.makedirs(msks)
    yy, xx = np.mgrid[0:HW[0], 0:HW[1]]
    pal = [0, 0, 0, 200, 0, 0, 0, 200, 0, 0, 0, 200] + [0] * (256 * 3 - 12)
    for i in range(t):
        Image.fromarray(seeded_frame(HW, seed, shift=2 * i)).save(os.path.join(imgs, f'{i:05d}.jpg'), quality=90)
        idx = np.zeros(HW, np.uint8)
        for o in range(n_obj):
            cx = HW[1] * (o + 1) / (n_obj + 1) + 1.5 * i - 0.75 * t
            cy = HW[0] * (0.5 + 0.15 * (o - (n_obj - 1) / 2))
            idx[(((yy - cy) / (HW[0] / 7)) ** 2 + ((xx - cx) / (HW[1] / 12)) ** 2) <= 1] = o + 1
        im = Image.fromarray(idx, mode='P')
        im.putpalette(pal)
        im.save(os.path.join(msks, f'{i:05d}.png'))
    return imgs, msks


def timed_round(s):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.full_propagation()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def copy_launch_us(entry, reps):
    """(restore, save) microseconds per launch of one frame's entry, and the bytes one launch moves (read + written)."""
    import torch
    from xmem2_amd import ops
    bufs = [torch.empty_like(t) for t in entry]
    out = []
    for pairs in (list(zip(entry, bufs)), list(zip(bufs, entry))):
        for _ in range(3):
            ops.copy_segments(pairs)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.copy_segments(pairs)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return out[0], out[1], 2 * sum(t.numel() * t.element_size() for t in entry)


def bench(n_obj, frames, rounds, reps, model, tmp, net, emit):
    import torch
    from xmem2_amd.session import VideoSession
    imgs, msks = write_clip(os.path.join(tmp, f'clip{n_obj}'), frames, seed=5, n_obj=n_obj)
    cfg = {'model': model, 'size': 480}
    off = VideoSession(imgs, msks, overwrite_config=dict(cfg), network=net)
    on = VideoSession(imgs, msks, overwrite_config=dict(cfg, session_feature_cache_bytes=64 << 30), network=net)
    for s in (off, on):
        s.save_reference(0)
    first = {name: timed_round(s) for name, s in (('off', off), ('on', on))}
    times = {'off': [], 'on': []}
    for _ in range(rounds):
        for name, s in (('off', off), ('on', on)):
            times[name].append(timed_round(s))
    same = bool(torch.equal(off.masks, on.masks) and torch.equal(off.key, on.key) and torch.equal(off.selection, on.selection))
    info = on.cache_info()
    fc = on._fcache
    restore, save, moved = copy_launch_us(fc._entry(fc._slot[0]), reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    fmt = lambda ts: ' '.join(f'{v:7.4f}' for v in ts)
    emit(f'\n{n_obj} object(s), {frames} frames of {HW[0]} x {HW[1]}, key_batch {on.key_batch}, one reference (frame 0); seconds per full_propagation()')
    emit(f'   round 1 (captures; the cache is filled)   cache off {first["off"]:7.4f}   cache on {first["on"]:7.4f}')
    emit(f'   rounds 2..{rounds + 1}, cache off (the parent commit)  {fmt(times["off"])}   median {med["off"]:.4f}  '
         f'({1e3 * med["off"] / frames:.3f} ms per frame)')
    emit(f'   rounds 2..{rounds + 1}, cache on                       {fmt(times["on"])}   median {med["on"]:.4f}  '
         f'({1e3 * med["on"] / frames:.3f} ms per frame)')
    emit(f'   cache off / cache on (medians) = {med["off"] / med["on"]:.3f}x;  min / min = {min(times["off"]) / min(times["on"]):.3f}x')
    emit(f'   masks, keys and selections of the two sessions equal: {same}')
    emit(f'   cache: {info["frames"]} frames, entry {info["entry_bytes"] / 1e6:.2f} MB, arena {info["bytes"] / 1e9:.3f} GB, '
         f'hits {info["hits"]}, misses {info["misses"]}')
    emit(f'   copy launch on its own ({reps} back to back): restore {restore:.1f} us, save {save:.1f} us per frame '
         f'({moved / 1e6:.1f} MB read + written: {moved / restore / 1e6:.2f} / {moved / save / 1e6:.2f} TB/s)')
    del off, on
    return med['off'] / med['on']


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=6, help='timed rounds per session after the first')
    ap.add_argument('--objects', default='1,3')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None, help='also append the report to this file')
    args = ap.parse_args()
    import torch
    from session_bench import save_checkpoint
    from xmem2_amd.network import XMem
    torch.set_grad_enabled(False)
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
    with tempfile.TemporaryDirectory() as tmp:
        model = save_checkpoint(os.path.join(tmp, 'XMem_synth.pth'))
        net = XMem({'model': model, 'size': 480}, model).to('cuda').eval()
        emit(f'tools/session_cache_bench.py on {torch.cuda.get_device_name(0)}: VideoSession re-propagation with the feature cache off and on, '
             'alternating in one process, precision fp32')
        for n_obj in (int(v) for v in args.objects.split(',')):
            bench(n_obj, args.frames, args.rounds, args.reps, model, tmp, net, emit)


if __name__ == '__main__':
    main()
