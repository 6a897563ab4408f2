"""DAVIS-style mask evaluation: region similarity J and boundary accuracy F (util/metrics.py and the `compute_metrics` driver of
inference/run_experiments.py:376-410), with the per-pixel work on the device.

    from xmem2_amd.metrics import batched_jaccard, batched_f_measure, jf, compute_metrics

One `xmem_jf_counts` launch turns a batch of (gt, pred) label maps into exact integer counts per frame and object (areas,
intersection, boundary pixels, boundary matches); `scores_from_counts` applies the reference's float64 arithmetic to them in the
reference's order, so J and F equal the reference's bit for bit.  `python -m xmem2_amd.evaluate` is the command-line form.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SLOTS = ('gt_area', 'pred_area', 'inter', 'n_gt', 'n_pred', 'gt_match', 'pred_match')
MAX_RADIUS = 63
MAX_LABEL = 254
FRAMES_PER_LAUNCH = 64          # bounds the device copy of the label maps of one launch (64 x 1080p x 2 maps = 265 MB)


def bound_pix(bound_th, shape):
    """f_measure's dilation radius (util/metrics.py:157-158): bound_th itself when >= 1, else ceil(bound_th * |(H, W)|).  A
    non-integer bound_th >= 1 is refused: the reference's disk would then be of even size, off-centre."""
    if bound_th < 0:
        raise ValueError(f'bound_th {bound_th!r} must be >= 0')
    if bound_th >= 1:
        if float(bound_th) != int(bound_th):
            raise ValueError(f'bound_th {bound_th!r} >= 1 must be an integer number of pixels')
        return int(bound_th)
    return int(np.ceil(bound_th * np.linalg.norm(tuple(shape))))


def _check_pair(y_true, y_pred):
    """The reference's shape checks and ValueErrors; label maps come back as uint8 numpy arrays or uint8 device tensors."""
    import torch
    if isinstance(y_true, torch.Tensor) and isinstance(y_pred, torch.Tensor) and y_true.is_cuda and y_pred.is_cuda:
        shp_t, shp_p = tuple(y_true.shape), tuple(y_pred.shape)
    else:
        y_true = np.asarray(y_true.cpu() if isinstance(y_true, torch.Tensor) else y_true)
        y_pred = np.asarray(y_pred.cpu() if isinstance(y_pred, torch.Tensor) else y_pred)
        shp_t, shp_p = y_true.shape, y_pred.shape
    if len(shp_t) != 3:
        raise ValueError('y_true array must have 3 dimensions.')
    if len(shp_p) != 3:
        raise ValueError('y_pred array must have 3 dimensions.')
    if shp_t != shp_p:
        raise ValueError('y_true and y_pred must have the same shape. {} != {}'.format(shp_t, shp_p))
    out = []
    for a, name in ((y_true, 'y_true'), (y_pred, 'y_pred')):
        if isinstance(a, torch.Tensor):
            if a.dtype != torch.uint8:
                raise ValueError(f'{name}: a device tensor must be uint8')
        elif a.dtype != np.uint8:
            if a.size and (a.min() < 0 or a.max() > 255):
                raise ValueError(f'{name}: labels must lie in 0..255')
            a = a.astype(np.uint8)
        out.append(a)
    return out[0], out[1]


def object_ids(y_true, nb_objects=None):
    """The objects scored (util/metrics.py:46-51): the ids 0 < v < 255 of the whole sequence's ground truth, or 1..nb_objects."""
    import torch
    if nb_objects is None:
        if isinstance(y_true, torch.Tensor):
            present = torch.bincount(y_true.reshape(-1).to(torch.int64), minlength=256).cpu().numpy() > 0
            ids = np.nonzero(present[1:255])[0] + 1
        else:
            v = np.asarray(y_true)
            ids = np.unique(v[(v < 255) & (v > 0)])
    else:
        if int(nb_objects) > MAX_LABEL:
            raise ValueError(f'nb_objects {nb_objects} > {MAX_LABEL}: label 255 is void and not scored here')
        ids = np.arange(1, int(nb_objects) + 1)
    if len(ids) == 0:
        raise ValueError('Number of objects in y_true should be higher than 0.')
    return np.asarray(ids, np.int64)


def counts(y_true, y_pred, radius, lut=None):
    """xmem_jf_counts over [B,H,W] label maps (numpy or device uint8) -> int64 numpy [B,256,7] (SLOTS).  A few launches, one sync."""
    import torch
    from . import ops
    if not torch.cuda.is_available():
        raise RuntimeError('xmem2_amd.metrics needs an MI355X (HIP) device - there is no CPU path')
    dev = torch.device('cuda', torch.cuda.current_device())
    B = y_true.shape[0]
    out = torch.empty((B, 256, len(SLOTS)), dtype=torch.int32, device=dev)
    for b0 in range(0, B, FRAMES_PER_LAUNCH):
        sl = slice(b0, min(B, b0 + FRAMES_PER_LAUNCH))
        g = y_true[sl] if isinstance(y_true, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y_true[sl]))
        p = y_pred[sl] if isinstance(y_pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y_pred[sl]))
        ops.jf_counts(g.to(dev), p.to(dev), radius, lut=lut, out=out[sl])
    return out.cpu().numpy().astype(np.int64)


def scores_from_counts(c, ids):
    """Per-frame, per-object (J, F) float64 [B, nObj] from counts [B,256,7], in the reference's arithmetic:
    J = 1 when the union is 0, else inter / union (util/metrics.py:60-64); F from precision = pred_match / n_pred and
    recall = gt_match / n_gt with the four cases of f_measure (:178-193), then 2 * precision * recall / (precision + recall)."""
    c = np.asarray(c, np.int64)[:, np.asarray(ids, np.int64), :]
    ga, pa, inter, n_gt, n_fg, gt_match, fg_match = (c[..., i] for i in range(len(SLOTS)))
    union = ga + pa - inter
    J = np.where(union == 0, 1.0, inter / np.where(union == 0, 1, union))
    precision = np.where(n_fg == 0, 1.0, fg_match / np.where(n_fg == 0, 1, n_fg).astype(np.float64))
    recall = np.where(n_gt == 0, 1.0, gt_match / np.where(n_gt == 0, 1, n_gt).astype(np.float64))
    precision = np.where((n_fg > 0) & (n_gt == 0), 0.0, precision)
    recall = np.where((n_fg == 0) & (n_gt > 0), 0.0, recall)
    s = precision + recall
    F = np.where(s == 0, 0.0, 2 * precision * recall / np.where(s == 0, 1.0, s))
    return np.ascontiguousarray(J, np.float64), np.ascontiguousarray(F, np.float64)


def jf(y_true, y_pred, average_over_objects=True, nb_objects=None, bound_th=0.008):
    """(J, F) of batched_jaccard and batched_f_measure from one kernel pass: float64 numpy [B] (average_over_objects) or [B, nObj]."""
    y_true, y_pred = _check_pair(y_true, y_pred)
    ids = object_ids(y_true, nb_objects)
    r = bound_pix(bound_th, tuple(y_true.shape[1:]))
    if r > MAX_RADIUS:
        raise ValueError(f'dilation radius {r} > {MAX_RADIUS} is not supported')
    J, F = scores_from_counts(counts(y_true, y_pred, r), ids)
    if average_over_objects:
        J, F = J.mean(axis=1), F.mean(axis=1)
    return J, F


def batched_jaccard(y_true, y_pred, average_over_objects=True, nb_objects=None):
    """util/metrics.py:10-69: J per frame (average_over_objects) or per frame and object, float64."""
    return jf(y_true, y_pred, average_over_objects=average_over_objects, nb_objects=nb_objects)[0]


def batched_f_measure(y_true, y_pred, average_over_objects=True, nb_objects=None, bound_th=0.008):
    """util/metrics.py:199-258: F per frame (average_over_objects) or per frame and object, float64."""
    return jf(y_true, y_pred, average_over_objects=average_over_objects, nb_objects=nb_objects, bound_th=bound_th)[1]


# ---- files (inference/run_experiments.py:316-320, 376-410) --------------------------------------------------------------------
def _sorted_files(d):
    return sorted(os.path.join(d, f) for f in os.listdir(d) if os.path.isfile(os.path.join(d, f)))


def _load_gt(path):
    from PIL import Image
    return np.array(Image.open(path).convert('P'), np.uint8)


def _load_pred(path, palette, size):
    from PIL import Image
    im = Image.open(path).convert('RGB').resize(size, resample=Image.Resampling.NEAREST)
    return np.array(im.quantize(palette=palette, dither=Image.Dither.NONE), np.uint8)


def load_video(gt_dir, pred_dir, pool):
    """(gts, preds) uint8 [T,H,W] of one video: GT as convert('P'), predictions as RGB resized (nearest) to the GT size and quantised
    to the first GT mask's palette; files paired in sorted order."""
    from PIL import Image
    gt_files, pred_files = _sorted_files(gt_dir), _sorted_files(pred_dir)
    if len(gt_files) != len(pred_files):
        raise ValueError(f'{pred_dir}: {len(pred_files)} predicted masks for {len(gt_files)} ground-truth masks in {gt_dir}')
    if not gt_files:
        raise ValueError(f'{gt_dir}: no ground-truth masks')
    first = Image.open(gt_files[0]).convert('P')
    first.load()
    w, h = first.size
    gts = np.stack(list(pool.map(_load_gt, gt_files)))
    preds = np.stack(list(pool.map(lambda p: _load_pred(p, first, (w, h)), pred_files)))
    if gts.shape != preds.shape:
        raise ValueError(f'{pred_dir}: ground truth {gts.shape} and predictions {preds.shape} differ')
    return gts, preds


PRED_FORMATS = ('auto', 'png', 'tracks')
TRACKS_NAME = 'tracks.json'


def _has_files(d):
    return os.path.isdir(d) and any(os.path.isfile(os.path.join(d, f)) for f in os.listdir(d))


def _tracks_of(video_dir, png_dir, fmt):
    """The tracks file one side of a video is read from, or None for its PNGs: 'tracks' forces the file, 'png' the PNGs, 'auto'
    takes the file only where `png_dir` is absent or holds no file and `<video_dir>/tracks.json` exists."""
    path = os.path.join(video_dir, TRACKS_NAME)
    if fmt == 'tracks':
        if not os.path.isfile(path):
            raise FileNotFoundError(f'{video_dir}: no {TRACKS_NAME}')
        return path
    if fmt == 'auto' and not _has_files(png_dir) and os.path.isfile(path):
        return path
    return None


def _device_maps(path):
    """Every frame of a tracks file as device label maps uint8 [T,H,W] holding the annotations' labels (`ops.rle_decode`): no pixel
    is touched on the host.  A frame without an entry is all zero."""
    from .rle import TrackReader
    return TrackReader(path).masks_device(values='label')[0]


def _gt_tracks(gt_dir):
    """`<gt>/<video>/tracks.json` when the directory holds no other file (no PNG), else None."""
    path = os.path.join(gt_dir, TRACKS_NAME)
    if os.path.isfile(path) and not any(f != TRACKS_NAME and os.path.isfile(os.path.join(gt_dir, f)) for f in os.listdir(gt_dir)):
        return path
    return None


def load_video_tracks(name, gt_dir, gt_tracks, pred_dir, pred_tracks, pool):
    """(gts, preds) of one video with at least one side read from tracks.json.  Frames pair in order; the tracks' size must be the
    ground truth's (tracks are not resampled) and both sides must have one entry per frame: ValueError naming the video otherwise."""
    import torch
    if gt_tracks is not None:
        gts = _device_maps(gt_tracks)
    else:
        gt_files = _sorted_files(gt_dir)
        if not gt_files:
            raise ValueError(f'{gt_dir}: no ground-truth masks')
        gts = np.stack(list(pool.map(_load_gt, gt_files)))
    if pred_tracks is not None:
        preds = _device_maps(pred_tracks)
    else:                                                            # PNG predictions against ground truth from tracks: no palette
        pred_files = _sorted_files(pred_dir)                         # to quantise to, the index plane is taken as it is
        if len(pred_files) != gts.shape[0]:
            raise ValueError(f'video {name}: {len(pred_files)} predicted masks for {gts.shape[0]} ground-truth frames')
        preds = np.stack(list(pool.map(_load_gt, pred_files))) if pred_files else np.zeros((0,) + tuple(gts.shape[1:]), np.uint8)
    if preds.shape[0] != gts.shape[0]:
        raise ValueError(f'video {name}: {preds.shape[0]} predicted frames for {gts.shape[0]} ground-truth frames')
    if gts.shape[0] == 0:
        raise ValueError(f'video {name}: no ground-truth masks')
    if tuple(preds.shape[1:]) != tuple(gts.shape[1:]):
        raise ValueError(f'video {name}: predictions are {tuple(preds.shape[1:])}, the ground truth is {tuple(gts.shape[1:])} '
                         '(tracks are not resampled)')
    if isinstance(gts, torch.Tensor) != isinstance(preds, torch.Tensor):      # `jf` takes a pair on one side
        dev = gts.device if isinstance(gts, torch.Tensor) else preds.device
        gts = gts if isinstance(gts, torch.Tensor) else torch.from_numpy(gts).to(dev)
        preds = preds if isinstance(preds, torch.Tensor) else torch.from_numpy(preds).to(dev)
    return gts, preds


def compute_metrics(p_source_masks, p_preds, pred_to_annot_names_lookup=None, workers=8, pred_format='auto'):
    """Per-video mean J ('iou') and F ('f') of the predictions under `p_preds/<video>/masks/` against `p_source_masks/<video>/`
    (run_experiments.py:376-410), plus 'jf' = (iou + f) / 2.  DataFrame indexed by video_name, rows sorted by it.  PNG decoding runs
    on `workers` host threads; each video is scored in one or a few kernel launches.
    `pred_format`: 'auto' reads the PNGs wherever `masks/` holds a file and `p_preds/<video>/tracks.json` (config['save_tracks'])
    where it is absent or empty; 'png' / 'tracks' force one source.  Tracks are decoded on the device and scored there - no
    prediction pixel reaches the host, no image is opened for them.  The ground truth of a video may come from
    `p_source_masks/<video>/tracks.json` in the same way when the directory holds no other file."""
    import pandas as pd
    if pred_format not in PRED_FORMATS:
        raise ValueError(f'pred_format must be one of {PRED_FORMATS}, got {pred_format!r}')
    p_source_masks, p_preds = str(p_source_masks), str(p_preds)
    rows = []
    with ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix='xmem-metrics') as pool:
        for entry in sorted(os.listdir(p_preds)):
            pred_video = os.path.join(p_preds, entry)
            if not os.path.isdir(pred_video):
                continue
            name = pred_to_annot_names_lookup[entry] if pred_to_annot_names_lookup is not None else entry
            gt_dir, pred_dir = os.path.join(p_source_masks, name), os.path.join(pred_video, 'masks')
            pred_tracks = _tracks_of(pred_video, pred_dir, pred_format)
            gt_tracks = _gt_tracks(gt_dir)
            if pred_tracks is None and gt_tracks is None:
                gts, preds = load_video(gt_dir, pred_dir, pool)
            else:
                gts, preds = load_video_tracks(name, gt_dir, gt_tracks, pred_dir, pred_tracks, pool)
            J, F = jf(gts, preds)
            rows.append({'video_name': name, 'iou': float(J.mean(axis=0)), 'f': float(F.mean(axis=0))})
    if not rows:
        raise ValueError(f'{p_preds}: no video directories')
    df = pd.DataFrame.from_records(rows).set_index('video_name')
    df['jf'] = (df['iou'] + df['f']) / 2
    return df


class InLoopScorer:
    """J and F of a running video, frame by frame on the compute stream: each frame's ground truth is uploaded next to the predicted
    index mask (MaskMapper dense ids) and one xmem_jf_counts launch writes its counts into a [T,256,7] device table, with the
    mapper's current dense -> original LUT.  Nothing is read back until `scores`.
    The ground truth goes up through a ring of RING pinned host buffers (allocated once) on a copy stream of its own into RING device
    buffers, and the compute stream waits for that copy with an event.  A slot is written again only after the launch that read it
    (`_free` events)."""

    RING = 4

    def __init__(self, n_frames, device, bound_th=0.008):
        self.n, self.device, self.bound_th = n_frames, device, bound_th
        self.table = None
        self._copy, self._bufs, self._free, self._k = None, [], [], 0
        self.frames = []
        self.radius = None
        self.shape = None
        self._lut, self._lut_key = None, None

    def _lut_for(self, mapper):
        import torch
        if mapper.coherent:
            return None
        key = tuple(sorted(mapper.remappings.items()))
        if key != self._lut_key:                     # changes only on annotated frames that introduce an object
            lut = np.zeros(256, np.uint8)
            for original, dense in mapper.remappings.items():
                lut[dense] = original
            self._lut, self._lut_key = torch.from_numpy(lut).to(self.device), key
        return self._lut

    def add(self, ti, gt, pred_dev, mapper):
        """Frame ti: `gt` the host uint8 [H,W] ground truth, `pred_dev` the device uint8 [H,W] predicted mask in dense ids."""
        import torch
        from . import ops
        shape = tuple(gt.shape)
        if shape != tuple(pred_dev.shape):
            raise ValueError(f'frame {ti}: ground truth {shape} and prediction {tuple(pred_dev.shape)} differ in size')
        if self.table is None:
            self.shape = shape
            self.radius = bound_pix(self.bound_th, shape)
            if self.radius > MAX_RADIUS:
                raise ValueError(f'dilation radius {self.radius} > {MAX_RADIUS} is not supported')
            self.table = torch.empty((self.n, 256, len(SLOTS)), dtype=torch.int32, device=self.device)
            self._copy = torch.cuda.Stream(device=self.device)
            self._bufs = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(self.RING)]
            self._host = [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(self.RING)]
            self._free = [None] * self.RING
        elif shape != self.shape:
            raise ValueError(f'frame {ti}: ground truth {shape}, earlier frames {self.shape}')
        i = self._k % self.RING
        self._k += 1
        if self._free[i] is not None:                # the launch RING frames ago has read this slot (long done in practice)
            self._free[i].synchronize()
        np.copyto(self._host[i].numpy(), gt, casting='unsafe')
        with torch.cuda.stream(self._copy):
            self._bufs[i].copy_(self._host[i], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self._copy)
        main = torch.cuda.current_stream()
        main.wait_event(ready)
        ops.jf_counts(self._bufs[i], pred_dev, self.radius, lut=self._lut_for(mapper), out=self.table[ti:ti + 1])
        free = torch.cuda.Event()
        free.record(main)
        self._free[i] = free
        self.frames.append(ti)

    def scores(self):
        """(J, F) float64 [T]: per-frame means over the sequence's ground-truth object ids; NaN for frames without ground truth (and for
        every frame when the ground truth holds no object)."""
        J, F = np.full(self.n, np.nan), np.full(self.n, np.nan)
        if not self.frames:
            return J, F
        rows = np.asarray(self.frames, np.int64)
        c = self.table.cpu().numpy().astype(np.int64)[rows]
        ids = np.nonzero(c[:, 1:MAX_LABEL + 1, 0].sum(axis=0) > 0)[0] + 1
        if len(ids) == 0:
            return J, F
        j, f = scores_from_counts(c, ids)
        J[rows], F[rows] = j.mean(axis=1), f.mean(axis=1)
        return J, F
