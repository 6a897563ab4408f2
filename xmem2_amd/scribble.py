"""Scribbles -> annotation masks from the command line (the S2M step of the interactive demo, without the GUI).

    python -m xmem2_amd.scribble --images DIR --scribbles DIR --out DIR [--prev-masks DIR] [--model s2m.pth | --synthetic-seed N]
                                 [--num-objects K] [--ignore-class 255]

Files are paired by the first integer in their names (as process_video.py pairs frames and masks).  A scribble PNG is an
indexed map: k = a stroke for object k, 0 = a background stroke, 255 (--ignore-class) = no stroke.  For every frame with a
scribble map, the S2M network turns image, previous mask (optional, indexed) and strokes into aggregate_wbg(., keep_bg=True,
hard=True) and its argmax is written as a palette PNG named after the frame (`<frame stem>.png`), so the output directory
serves as the masks directory of run_on_video / process_video.  One network and one captured graph serve every frame.
"""
import argparse
import os
import re
import sys

import numpy as np

IMAGE_EXT = ('.jpg', '.jpeg', '.png', '.bmp')
IM_MEAN = np.array((0.485, 0.456, 0.406), np.float32)       # dataset/range_transform.py:5-8
IM_STD = np.array((0.229, 0.224, 0.225), np.float32)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m xmem2_amd.scribble', description=__doc__.split('\n\n')[0])
    ap.add_argument('--images', required=True, help='directory of frames')
    ap.add_argument('--scribbles', required=True, help='directory of indexed scribble PNGs (k = object, 0 = background, 255 = none)')
    ap.add_argument('--out', required=True, help='output directory for the palette masks')
    ap.add_argument('--prev-masks', default=None, help='directory of indexed previous masks (default: none)')
    src = ap.add_mutually_exclusive_group()
    src.add_argument('--model', default=None, help='S2M checkpoint (saves/s2m.pth)')
    src.add_argument('--synthetic-seed', type=int, default=None, help='conditioned synthetic weights instead of a checkpoint')
    ap.add_argument('--num-objects', type=int, default=None, help='objects (default: the largest label in scribbles / masks)')
    ap.add_argument('--ignore-class', type=int, default=255)
    args = ap.parse_args(argv)
    if args.model is None and args.synthetic_seed is None:
        ap.error('one of --model or --synthetic-seed is required')
    if args.model is not None and not os.path.isfile(args.model):
        ap.error(f'--model: no such file: {args.model}')
    if args.num_objects is not None and not 1 <= args.num_objects <= 254:
        ap.error('--num-objects must be in [1, 254]')
    if not 0 <= args.ignore_class <= 255:
        ap.error('--ignore-class must be in [0, 255]')
    return args


def frame_number(name):
    m = re.search(r'\d+', os.path.splitext(os.path.basename(name))[0])
    return int(m.group()) if m else None


def index_dir(path, exts=IMAGE_EXT):
    """{frame number: file name} of a directory; files without a number are skipped, a repeated number is an error."""
    out = {}
    if path is None:
        return out
    if not os.path.isdir(path):
        raise FileNotFoundError(f'not a directory: {path}')
    for f in sorted(os.listdir(path)):
        if not f.lower().endswith(exts):
            continue
        n = frame_number(f)
        if n is None:
            continue
        if n in out:
            raise ValueError(f'{path}: frames {out[n]} and {f} share the number {n}')
        out[n] = f
    return out


def pair_files(images, scribbles, prev_masks=None):
    """[(frame number, image file, scribble file, previous-mask file or None)] for every scribble map with a frame."""
    imgs, scrs, prevs = index_dir(images), index_dir(scribbles, ('.png',)), index_dir(prev_masks, ('.png',))
    missing = sorted(set(scrs) - set(imgs))
    if missing:
        raise FileNotFoundError(f'scribbles without a frame: numbers {missing[:10]}')
    return [(n, imgs[n], scrs[n], prevs.get(n)) for n in sorted(scrs)]


def _palette():
    """The DAVIS palette (bit-interleaved colour map), as the reference's masks use."""
    pal = np.zeros((256, 3), np.uint8)
    for i in range(256):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        pal[i] = (r, g, b)
    return pal.reshape(-1).tolist()


def _load_index(path):
    from PIL import Image
    im = Image.open(path)
    if im.mode not in ('P', 'L'):
        raise ValueError(f'{path}: expected an indexed (P) or grey (L) PNG, got mode {im.mode}')
    return np.array(im, dtype=np.uint8)


def main(argv=None):
    args = parse_args(argv)
    import torch
    from PIL import Image
    from .s2m import S2M, S2MController
    torch.set_grad_enabled(False)
    pairs = pair_files(args.images, args.scribbles, args.prev_masks)
    if not pairs:
        print('no scribble maps found', file=sys.stderr)
        return 1
    loaded = []
    k_max = 0
    for n, fi, fs, fp in pairs:
        img = np.array(Image.open(os.path.join(args.images, fi)).convert('RGB'), dtype=np.uint8)
        scr = _load_index(os.path.join(args.scribbles, fs))
        prev = _load_index(os.path.join(args.prev_masks, fp)) if fp else np.zeros(scr.shape, np.uint8)
        if scr.shape != img.shape[:2] or prev.shape != img.shape[:2]:
            raise ValueError(f'frame {n}: image {img.shape[:2]}, scribbles {scr.shape} and previous mask {prev.shape} differ in size')
        labels = set(np.unique(scr).tolist()) | set(np.unique(prev).tolist())
        labels -= {0, args.ignore_class}
        k_max = max([k_max] + list(labels))
        loaded.append((fi, img, scr, prev))
    K = args.num_objects or k_max
    if K < 1:
        print('no object strokes or masks found: nothing to segment', file=sys.stderr)
        return 1
    device = torch.device('cuda', torch.cuda.current_device())
    net = S2M(device=device)
    if args.model:
        net.load_weights(args.model)
    else:
        from .synth import synthetic_s2m_state_dict
        net.load_state_dict(synthetic_s2m_state_dict(args.synthetic_seed))
    ctl = S2MController(net, K, args.ignore_class, device=device)
    os.makedirs(args.out, exist_ok=True)
    pal = _palette()
    for fi, img, scr, prev in loaded:
        image = torch.from_numpy(((img.astype(np.float32) / 255.0 - IM_MEAN) / IM_STD).transpose(2, 0, 1).copy())[None]
        _, mask = ctl.predict(image.to(device), torch.from_numpy(prev).to(device), scr)
        out = Image.fromarray(mask.cpu().numpy(), mode='P')
        out.putpalette(pal)
        out.save(os.path.join(args.out, os.path.splitext(fi)[0] + '.png'))
    print(f'wrote {len(loaded)} mask(s) for {K} object(s) to {args.out} ({net.captures} graph capture(s))')
    return 0


if __name__ == '__main__':
    sys.exit(main())
