"""Feathered mattes, trimaps, grow and shrink of index masks: the definition, on the host, in numpy - and the command line.

This module is what `ops.signed_edt_sq` / `ops.mask_mattes` / `ops.grow_masks` (csrc/matte.hip, include/xmem_hip_matte.h) are tested
against byte for byte; the product path calls its tables and its parser, never its transforms.  Everything is integer but the tables,
which are made once per option in float64.

`m` is a uint8 index map [H, W], `k` a label in 1..255, `R` an integer in 1..127, cap2 = (R + 1)^2.  Distances run between pixel
centres and NOTHING exists outside the image: an object that touches the border has no edge there (`ops.edt_sq`, the click robot's
transform, puts a ring of zeros round the image; this one does not).

signed_d2_host(m, k, R) -> int32 [H, W]
    +min(cap2, min over q with m(q) != k of |p - q|^2)  where m(p) == k,
    -min(cap2, min over q with m(q) == k of |p - q|^2)  elsewhere;  a minimum over no pixel at all is cap2.

Every per-object product is table[s2 + cap2] with `table` uint8 of length 2 cap2 + 1 (`lookup`):
feather_table(feather=w, offset=o, falloff) -> (table, R), R = max(1, ceil(w / 2 + |o|)).  For index i: s2 = i - cap2, d = sqrt(|s2|),
    s = sign(s2) (d - 1/2) - the edge lies half-way between the nearest opposite centres - and +-inf where |s2| == cap2;
    a = clip(1/2 + (s + o) / w, 0, 1), for w == 0 the step s + o > 0; 'smooth' maps a -> a a (3 - 2 a); value = rint(255 a).
    The choice of R makes everything at the cap saturate, so the cap never shows.
trimap_table(band=t) -> (table, R), R = max(1, ceil(t)): 255 where s2 > t^2, 0 where s2 < -t^2, 128 between.

grow_host(m, r), r2 = floor(r r):
    r > 0, grow:   out(p) = m(p) where m(p) != 0 (objects never eat one another); else the label of the object pixel q with
                   |p - q|^2 <= r2 that minimises (|p - q|^2, m(q)) lexicographically - ties go to the smaller label -, 0 without one.
    r < 0, shrink: out(p) = 0 where m(p) != 0 and some q with m(q) != m(p) has |p - q|^2 <= r2; else m(p).

parse_mattes(spec): config['mattes'] -> None or {'feather', 'offset', 'falloff', 'trimap'}.

`python -m xmem2_amd.matte --tracks F | --masks DIR [--palette-from PNG] --out DIR [--feather W] [--offset O] [--falloff F]
[--trimap T]` makes the planes of results that already exist, on the device (tracks are decoded there: no mask plane reaches the host
before the matte does).
"""
import argparse
import json
import math
import os

import numpy as np

MAX_R = 127
KEYS = ('feather', 'offset', 'falloff', 'trimap')
FALLOFFS = ('linear', 'smooth')
DEFAULT_FEATHER = 2
OUTPUTS = ('mattes', 'trimaps')                 # the directories under masks_out_path, in the order of the tables


def _mask2d(m):
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype != np.uint8 or m.size == 0:
        raise ValueError(f'mask: expected a non-empty uint8 [H,W] array, got {m.dtype} {m.shape}')
    return m


def _check_radius(R):
    if isinstance(R, (bool, np.bool_)) or not isinstance(R, (int, np.integer)) or not 1 <= int(R) <= MAX_R:
        raise ValueError(f'R = {R!r} must be an integer in 1..{MAX_R}')
    return int(R)


def _d2_to(where):
    """int64 [H, W]: the squared distance of every pixel to the nearest pixel of `where`, None when `where` is empty.  scipy's
    transform is exact here: d is the float64 square root of an integer below 2^53, and rint(d d) gives the integer back."""
    from scipy.ndimage import distance_transform_edt
    if not where.any():
        return None
    d = distance_transform_edt(~where)
    return np.rint(d * d).astype(np.int64)


def signed_d2_host(m, k, R):
    m, R = _mask2d(m), _check_radius(R)
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 255:
        raise ValueError(f'k = {k!r} must be a label in 1..255')
    cap2 = (R + 1) ** 2
    inside = m == k
    out = np.empty(m.shape, np.int64)
    for side, sign in ((inside, 1), (~inside, -1)):                  # the pixels of `side` look for the nearest pixel outside it
        d2 = _d2_to(~side)
        out[side] = sign * (cap2 if d2 is None else np.minimum(d2[side], cap2))
    return out.astype(np.int32)


def radius2(r):
    """r -> (r2 = floor(r r), shrink); |r| <= 127"""
    if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, float, np.integer, np.floating)) or not math.isfinite(r):
        raise ValueError(f'grow: r = {r!r} must be a finite number')
    if abs(r) > MAX_R:
        raise ValueError(f'grow: |r| = {abs(r)} must be at most {MAX_R}')
    return int(math.floor(float(r) * float(r))), r < 0


def grow_host(m, r):
    m = _mask2d(m)
    r2, shrink = radius2(r)
    out = m.copy()
    labels = [int(v) for v in np.unique(m) if v]                     # ascending: argmin takes the first, the smaller label
    if r2 == 0:
        return out
    if shrink:
        for c in labels:
            d2 = _d2_to(m != c)
            if d2 is not None:
                out[(m == c) & (d2 <= r2)] = 0
        return out
    if not labels:
        return out
    d2 = np.stack([_d2_to(m == c) for c in labels])
    first = d2.argmin(0)
    near = np.take_along_axis(d2, first[None], 0)[0] <= r2
    grown = np.asarray(labels, np.uint8)[first]
    free = m == 0
    out[free & near] = grown[free & near]
    return out


# ---- tables ---------------------------------------------------------------------------------------------------------------------------

def _number(name, v, lo=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f'mattes: {name} = {v!r} must be a finite number')
    if lo is not None and v < lo:
        raise ValueError(f'mattes: {name} = {v!r} must be at least {lo}')
    return float(v)


def _table_radius(name, least, R):
    if least > MAX_R:
        raise ValueError(f'mattes: {name} needs a reach of {least} pixels, more than {MAX_R}')
    if R is None:
        return least
    R = _check_radius(R)
    if R < least:
        raise ValueError(f'mattes: {name} needs R >= {least}, got {R}')
    return R


def feather_radius(feather=DEFAULT_FEATHER, offset=0):
    return max(1, int(math.ceil(_number('feather', feather, 0) / 2 + abs(_number('offset', offset)))))


def trimap_radius(band):
    return max(1, int(math.ceil(_number('trimap', band, 0))))


def feather_table(feather=DEFAULT_FEATHER, offset=0, falloff='linear', R=None):
    """-> (uint8 [2 cap2 + 1], R).  `R`: a larger reach than the table needs (one distance pass serves several tables)."""
    w, o = _number('feather', feather, 0), _number('offset', offset)
    if falloff not in FALLOFFS:
        raise ValueError(f'mattes: falloff = {falloff!r}, known: {FALLOFFS}')
    R = _table_radius('feather', feather_radius(w, o), R)
    cap2 = (R + 1) ** 2
    s2 = np.arange(2 * cap2 + 1, dtype=np.int64) - cap2
    s = np.sign(s2) * (np.sqrt(np.abs(s2).astype(np.float64)) - 0.5)
    s[0], s[-1] = -np.inf, np.inf
    if w == 0:
        a = (s + o > 0).astype(np.float64)
    else:
        a = np.clip(0.5 + (s + o) / w, 0.0, 1.0)
    if falloff == 'smooth':
        a = a * a * (3.0 - 2.0 * a)
    return np.rint(255.0 * a).astype(np.uint8), R


def trimap_table(band=1, R=None):
    t = _number('trimap', band, 0)
    R = _table_radius('trimap', trimap_radius(t), R)
    cap2 = (R + 1) ** 2
    s2 = np.arange(2 * cap2 + 1, dtype=np.int64) - cap2
    table = np.full(2 * cap2 + 1, 128, np.uint8)
    table[s2 > t * t] = 255
    table[s2 < -(t * t)] = 0
    return table, R


def lookup(table, s2, R):
    """table[s2 + cap2]: the product of one object from its signed squared distance"""
    return np.asarray(table)[np.asarray(s2, np.int64) + (int(R) + 1) ** 2]


def parse_mattes(spec):
    """config['mattes'] -> None (off) or {'feather': w or None, 'offset': o, 'falloff': f, 'trimap': t or None} with the defaults
    filled in.  Accepts None, True ({'feather': 2}) or a dict with any of those keys; `'feather': None` together with `trimap` gives
    trimaps only.  Unknown keys, values that are no numbers, negative widths, an unknown falloff, a reach beyond 127 pixels and a
    dict that asks for nothing raise ValueError."""
    if spec is None:
        return None
    if spec is True:
        spec = {}
    if not isinstance(spec, dict):
        raise ValueError(f'mattes: expected None, True or a dict with any of {KEYS}, got {type(spec).__name__}')
    unknown = sorted(set(spec) - set(KEYS), key=str)
    if unknown:
        raise ValueError(f'mattes: unknown keys {unknown} (known: {KEYS})')
    out = {'feather': spec.get('feather', DEFAULT_FEATHER), 'offset': spec.get('offset', 0), 'falloff': spec.get('falloff', 'linear'),
           'trimap': spec.get('trimap')}
    out['offset'] = _number('offset', out['offset'])
    if out['falloff'] not in FALLOFFS:
        raise ValueError(f'mattes: falloff = {out["falloff"]!r}, known: {FALLOFFS}')
    if out['feather'] is not None:
        out['feather'] = _number('feather', out['feather'], 0)
        _table_radius('feather', feather_radius(out['feather'], out['offset']), None)
    if out['trimap'] is not None:
        out['trimap'] = _number('trimap', out['trimap'], 0)
        _table_radius('trimap', trimap_radius(out['trimap']), None)
    if out['feather'] is None and out['trimap'] is None:
        raise ValueError('mattes: feather = None without a trimap asks for nothing')
    return out


def tables_of(spec):
    """What a parsed spec asks of one distance pass -> (names: the output directories, tables uint8 [T, 2 cap2 + 1], R)"""
    R = max(feather_radius(spec['feather'], spec['offset']) if spec['feather'] is not None else 1,
            trimap_radius(spec['trimap']) if spec['trimap'] is not None else 1)
    names, tables = [], []
    if spec['feather'] is not None:
        names.append(OUTPUTS[0])
        tables.append(feather_table(spec['feather'], spec['offset'], spec['falloff'], R=R)[0])
    if spec['trimap'] is not None:
        names.append(OUTPUTS[1])
        tables.append(trimap_table(spec['trimap'], R=R)[0])
    return names, np.stack(tables), R


def planes_host(m, K, spec):
    """{name: uint8 [K, H, W]} of the dense index map `m`: what the loop writes, by the definitions above"""
    names, tables, R = tables_of(spec)
    s2 = np.stack([signed_d2_host(m, k, R) for k in range(1, K + 1)])
    return {name: lookup(table, s2, R) for name, table in zip(names, tables)}


# ---- the writer of the planes (the frame loops, VideoSession.save_mattes and the command line) ------------------------------------------

def plane_job(names, labels, planes, stem):
    """The `_AsyncSaver` job that writes planes uint8 [T, K, H, W] as <names[t]>/<labels[j]>/<stem>.png, 8-bit mode L."""
    def job():
        from PIL import Image
        for t, sub in enumerate(names):
            for j, lab in enumerate(labels):
                yield Image.fromarray(np.ascontiguousarray(planes[t, j])), os.path.join(sub, str(lab)), stem + '.png'
    return job


def write_mattes(masks_of, n_frames, stems, labels, out_dir, spec, batch=32, png_on_device=False):
    """`ops.mask_mattes` over `n_frames` frames in launches of at most `batch`, written under `out_dir`.  masks_of(frames) ->
    (uint8 device tensor [len(frames), H, W] of dense ids 1..len(labels), present bool per frame); a frame that is not present gets
    no file.  `png_on_device`: the planes of a launch are encoded as 'grey' PNGs on the device in one `ops.png_encode` call and the
    files' bytes reach the host, not the planes.  Returns the number of files."""
    import torch
    from . import ops
    from .rle import batches
    from .frame_outputs import _AsyncSaver
    names, tables, R = tables_of(spec)
    k, written = len(labels), 0
    saver, tables_dev = _AsyncSaver(str(out_dir), ''), None
    try:
        for frames in batches(range(n_frames if k else 0), batch):
            dense, present = masks_of(frames)
            if not any(present):
                continue
            if tables_dev is None:
                tables_dev = torch.from_numpy(tables).to(dense.device)
            planes = ops.mask_mattes(dense, k, tables_dev, R)                       # [T, N, K, H, W]
            if png_on_device:
                from .png import bytes_job, plane_files
                files = ops.png_encode(planes.reshape((-1,) + tuple(planes.shape[-2:])), 'grey')
                n = len(frames)
            else:
                planes = planes.cpu().numpy()
            for j, t in enumerate(frames):
                if present[j]:
                    if png_on_device:
                        mine = [files[(i * n + j) * k + c] for i in range(len(names)) for c in range(k)]
                        saver.submit(bytes_job(plane_files(names, labels, mine, stems[t])))
                    else:
                        saver.submit(plane_job(names, labels, planes[:, j], stems[t]))
                    written += len(names) * k
    finally:
        saver.close()
    return written


def matte_tracks(tracks, out_dir, spec, batch=32, png_on_device=False):
    """The planes of every entry of a tracks file, decoded on the device (`TrackReader.masks_device`): <label> is the track's label."""
    from .rle import TrackReader
    reader = TrackReader(tracks)
    reader.require_unique_labels('matte_tracks')
    stems = [os.path.splitext(n)[0] for n in reader.frame_names()]

    def masks_of(frames):
        return reader.masks_device(frames, values='dense', batch=max(1, int(batch)))
    return write_mattes(masks_of, len(reader), stems, list(reader.labels), out_dir, spec, batch, png_on_device)


def _colour_keys(rgb):
    rgb = np.asarray(rgb, np.uint32)
    return rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]


def matte_pngs(mask_dir, out_dir, spec, batch=32, palette_from=None, png_on_device=False):
    """The planes of a directory of mask PNGs; <label> runs over the labels that occur in any of them, in ascending order.  Index
    PNGs (mode P or L, as `python -m xmem2_amd.rle --out DIR` writes them): the pixel values are the labels.  Colour PNGs (mode RGB,
    as run_on_video writes them): `palette_from` names a palette PNG - an annotation - and a colour is the first index that has it;
    a colour the palette does not hold is a ValueError."""
    import torch
    from PIL import Image
    files = sorted(f for f in os.listdir(mask_dir) if f.lower().endswith('.png'))
    if not files:
        raise ValueError(f'{mask_dir}: no PNG')
    pal_keys = None
    if palette_from is not None:
        pal = np.asarray(Image.open(palette_from).convert('P').getpalette(), np.uint8).reshape(-1, 3)
        pal_keys, first = np.unique(_colour_keys(pal), return_index=True)                # sorted keys, the first index of each

    def read(f):
        img = Image.open(os.path.join(mask_dir, f))
        if img.mode in ('P', 'L'):
            return np.asarray(img, np.uint8)
        if img.mode not in ('RGB', 'RGBA'):
            raise ValueError(f'{f}: mode {img.mode}, a mask PNG is mode P, L or RGB')
        if pal_keys is None:
            raise ValueError(f'{f}: a colour PNG needs --palette-from (an annotation PNG) to name its labels')
        keys = _colour_keys(np.asarray(img.convert('RGB')))
        at = np.minimum(np.searchsorted(pal_keys, keys), len(pal_keys) - 1)
        if (pal_keys[at] != keys).any():
            raise ValueError(f'{f}: a colour that the palette of {palette_from} does not hold')
        return first[at].astype(np.uint8)
    masks = [read(f) for f in files]
    if len({m.shape for m in masks}) != 1:
        raise ValueError(f'{mask_dir}: the PNGs differ in size')
    labels = sorted({int(v) for m in masks for v in np.unique(m) if v})
    lut = np.zeros(256, np.uint8)
    lut[labels] = np.arange(1, len(labels) + 1, dtype=np.uint8)
    device = torch.device('cuda', torch.cuda.current_device())

    def masks_of(frames):
        return torch.from_numpy(np.stack([lut[masks[t]] for t in frames])).to(device), [True] * len(frames)
    return write_mattes(masks_of, len(files), [os.path.splitext(f)[0] for f in files], labels, out_dir, spec, batch, png_on_device)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m xmem2_amd.matte',
                                 description='feathered mattes and trimaps of masks that already exist, made on the device: '
                                             '<out>/mattes/<label>/<frame>.png and, with --trimap, <out>/trimaps/<label>/<frame>.png')
    ap.add_argument('--tracks', default=None, help='a tracks.json; its masks are decoded on the device')
    ap.add_argument('--masks', default=None, metavar='DIR', help='a directory of mask PNGs: index PNGs (mode P or L, as `python -m xmem2_amd.rle '
                                                                 '--out` writes them) or, with --palette-from, the colour PNGs of run_on_video')
    ap.add_argument('--palette-from', default=None, metavar='PNG', help='with --masks: the palette PNG (an annotation) whose indices name the '
                                                                        'colours of RGB masks')
    ap.add_argument('--out', required=True, metavar='DIR', help='the directory the planes are written under')
    ap.add_argument('--feather', default=None, metavar='W', help=f'width of the soft edge in pixels (default {DEFAULT_FEATHER}); '
                                                                 '"none" together with --trimap writes trimaps only')
    ap.add_argument('--offset', type=float, default=0.0, metavar='O', help='moves the edge outwards (> 0, spread) or inwards (< 0, choke)')
    ap.add_argument('--falloff', default='linear', choices=FALLOFFS)
    ap.add_argument('--trimap', type=float, default=None, metavar='T', help='also write trimaps with an unknown band of T pixels either side')
    ap.add_argument('--png-on-device', action='store_true', help='build the PNG files on the device: their bytes reach the host, not the planes')
    args = ap.parse_args(argv)
    if (args.tracks is None) == (args.masks is None):
        ap.error('exactly one of --tracks and --masks is needed')
    spec = {'offset': args.offset, 'falloff': args.falloff, 'trimap': args.trimap}
    if args.feather is not None:
        try:
            spec['feather'] = None if args.feather.lower() == 'none' else float(args.feather)
        except ValueError:
            ap.error(f'--feather: {args.feather!r} is neither a number nor "none"')
    try:
        args.spec = parse_mattes(spec)
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.tracks is not None:
        written = matte_tracks(args.tracks, args.out, args.spec, png_on_device=args.png_on_device)
    else:
        written = matte_pngs(args.masks, args.out, args.spec, palette_from=args.palette_from, png_on_device=args.png_on_device)
    print(json.dumps({'files': written, 'out': args.out}))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
