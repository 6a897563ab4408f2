"""Video harness with the reference's ``run_on_video`` surface (inference/run_on_video.py:31-282).

Frame decoding, mask reading and PNG writing are host I/O outside the timed region of the reference
(run_on_video.py:106-113) and outside this tier's hot path; this module supplies a minimal reader/writer
(PIL only - torchvision / cv2 are not available) so that the drop-in call works end to end:

    stats = run_on_video(imgs_in_path, masks_in_path, masks_out_path, frames_with_masks=[0, 10])

What is reproduced from the reference: config merge and the derived ``enable_long_term_count_usage``
(:190-196), preload of all annotated frames into permanent memory before the loop (:59-66), the per-frame
``step`` call and its flags (:98-108), resize + argmax post-processing (:165-173, on the GPU), the stats rows
(:115-123) and the output layout ``<out>/masks/<frame>.png`` (+ ``overlay/<frame>.jpg``).
Not reproduced: mp4 extraction (needs cv2).  `augment_images_with_masks` uses xmem2_amd/augmentations.py (unpinned restatement).

There is one frame loop, `_run_frame_loop`: `hinted` decides which frames are hinted when, `_FrameOutputs` is the whole output side
(scorer, tracks, mask copy one frame behind, stats rows, saver jobs).  `run_on_video` and `run_on_video_ensemble` are a preload and
three callbacks each (hint / prepare / frame); `VideoSession` shares `hinted`, `_stats_row` and `_saver_job`.
"""
import collections
import os
import queue
import threading
from dataclasses import dataclass
from time import perf_counter
from typing import Iterable, Optional
from warnings import warn

import numpy as np
import torch

from . import ops
from .configuration import VIDEO_INFERENCE_CONFIG
from .inference_core import InferenceCore
from .mask_cleanup import parse_cleanup
from .mask_mapper import MaskMapper
from .metrics import InLoopScorer
from .network import XMem
from .tensor_util import compute_array_iou

IM_MEAN = np.array([0.485, 0.456, 0.406], np.float32)     # dataset/range_transform.py:5-8
IM_STD = np.array([0.229, 0.224, 0.225], np.float32)


@dataclass
class Sample:
    """inference/data/video_reader.py:20-28.  `rgb_u8` is the decoded (and, if asked, resized) H x W x 3 uint8 frame;
    `rgb` - the reference's normalised 3 x H x W float tensor - is derived from it on first use (the harness itself
    hands `rgb_u8` to the device, where ToTensor + Normalize + padding are one kernel).
    A reader made with `resize_on_device=True` does not resize: `rgb_u8` is None, `src_u8` is the decoded SOURCE-size frame and
    `target_hw` the working size the device resizes it to (`ops.resize_u8`, the same bytes as the host resize)."""
    rgb_u8: Optional[torch.Tensor]
    raw_image_pil: object
    frame: str
    save: bool
    shape: tuple
    need_resize: bool
    mask: Optional[np.ndarray] = None
    _rgb: Optional[torch.Tensor] = None
    src_u8: Optional[torch.Tensor] = None
    target_hw: Optional[tuple] = None

    @property
    def rgb(self):
        if self._rgb is None:
            if self.rgb_u8 is None:                      # resize_on_device: the host restatement of the same resize
                from .pil_resize import resize_u8_host
                u8 = resize_u8_host(self.src_u8.numpy(), *self.target_hw)
            else:
                u8 = self.rgb_u8.numpy()
            arr = (u8.astype(np.float32) / 255.0 - IM_MEAN) / IM_STD
            self._rgb = torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))
        return self._rgb


class VideoReader:
    """Directory-of-frames reader (inference/data/video_reader.py:31-118 without cv2 / torchvision).
    `mask_dir` may name a tracks file (xmem2_amd/rle.py) instead of a directory of palette PNGs, or a directory that holds no PNG
    but a tracks.json: frames then match the file's `file_names` by stem, a frame's mask is `TrackReader.mask_host`, the first mask
    is the first frame with an entry, and - tracks carry no palette - the written PNGs take the DAVIS palette, so that their indices
    are the tracks' labels."""
    tracks = None                                   # the TrackReader when the annotations come from a tracks file

    def __init__(self, vid_name, video_path, mask_dir, size=-1, use_all_masks=False, resize_on_device=False):
        from PIL import Image
        self.resize_on_device = bool(resize_on_device)
        self._Image = Image
        if os.path.isfile(video_path):
            raise NotImplementedError('video files need cv2 for frame extraction; pass a directory of frames')
        self.vid_name, self.image_dir, self.mask_dir = vid_name, video_path, mask_dir
        self.size, self.use_all_masks = size, use_all_masks
        self.frames = sorted(os.listdir(self.image_dir))
        tracks_path = mask_dir if os.path.isfile(mask_dir) else None
        if tracks_path is None:
            masks = sorted(os.listdir(mask_dir))
            if 'tracks.json' in masks and not any(m.endswith(('.png', '.PNG')) for m in masks):
                tracks_path = os.path.join(mask_dir, 'tracks.json')
        if tracks_path is not None:
            from .rle import TrackReader
            from .scribble import _palette
            self.tracks = TrackReader(tracks_path)
            self.first_gt_path = None
            self._first_track_frame = next((t for t in range(len(self.tracks)) if self.tracks.has_mask(t)), None)
            self.reference_mask = Image.new('P', (1, 1))
            self.reference_mask.putpalette(_palette())
            return
        self.first_gt_path = os.path.join(mask_dir, masks[0])
        self.reference_mask = Image.open(self.first_gt_path).convert('P')
        self.reference_mask.load()                   # decoded once here: the writer threads only read it afterwards

    def __len__(self):
        return len(self.frames)

    def _target_hw(self, h, w):
        if self.size < 0:
            return h, w
        s = self.size / min(h, w)                  # Resize(size): shorter side -> size
        return (self.size, int(w * s)) if h <= w else (int(h * s), self.size)

    def frame_u8(self, img):
        """PIL RGB image -> the working-size H x W x 3 uint8 tensor (the Resize of im_transform, video_reader.py:61-65;
        ToTensor + Normalize happen on the device)."""
        Image = self._Image
        shape = (img.size[1], img.size[0])
        th, tw = self._target_hw(*shape)
        work = img if (th, tw) == shape else img.resize((tw, th), Image.BILINEAR)
        return torch.from_numpy(np.array(work, dtype=np.uint8))                   # owns its memory

    def frame_src_u8(self, img):
        """PIL RGB image -> (the decoded source-size H x W x 3 uint8 tensor, the working size (th, tw) it is resized to on the
        device): `frame_u8` without the resize."""
        return torch.from_numpy(np.array(img, dtype=np.uint8)), self._target_hw(img.size[1], img.size[0])

    def __getitem__(self, idx) -> Sample:
        Image = self._Image
        name = self.frames[idx]
        img = Image.open(os.path.join(self.image_dir, name)).convert('RGB')
        shape = (img.size[1], img.size[0])
        rgb_u8 = src_u8 = target_hw = None
        if self.resize_on_device:
            src_u8, target_hw = self.frame_src_u8(img)
        else:
            rgb_u8 = self.frame_u8(img)
        mask = None
        if self.tracks is not None:
            t = self.tracks.frame_index(name[:-4])
            if t is not None and (self.use_all_masks or t == self._first_track_frame):
                mask = self.tracks.mask_host(t)
        else:
            gt_path = os.path.join(self.mask_dir, name[:-4] + '.png')
            if not os.path.exists(gt_path):
                gt_path = os.path.join(self.mask_dir, name[:-4] + '.PNG')
            if (self.use_all_masks or gt_path == self.first_gt_path) and os.path.exists(gt_path):
                mask = np.array(Image.open(gt_path).convert('P'), dtype=np.uint8)
        return Sample(rgb_u8=rgb_u8, raw_image_pil=img, frame=name, save=True, shape=shape,
                      need_resize=not (self.size < 0), mask=mask, src_u8=src_u8, target_hw=target_hw)

    def resize_mask(self, onehot):
        """nearest resize of a [K,H,W] one-hot mask to the working size (video_reader.py:148-153)."""
        h, w = onehot.shape[-2:]
        m = min(h, w)
        th, tw = int(h / m * self.size), int(w / m * self.size)
        if (th, tw) == (h, w):
            return onehot
        ys = (np.arange(th) * (h / th)).astype(np.int64)
        xs = (np.arange(tw) * (w / tw)).astype(np.int64)
        return onehot[:, torch.from_numpy(ys)][:, :, torch.from_numpy(xs)]

    def map_the_colors_back(self, pred_mask):
        Image = self._Image
        return pred_mask.quantize(palette=self.reference_mask, dither=Image.Dither.NONE).convert('RGB')


class _AsyncSaver:
    """Background threads that colour-map and write masks / overlays (the reference uses two writer processes,
    util/image_saver.py:240-345).  PIL releases the GIL inside quantize / PNG / JPEG encoding, so threads scale."""

    def __init__(self, out_dir, vid_name, max_queue=200, workers=4):
        self.root = os.path.join(out_dir, vid_name)
        self.q = queue.Queue(max_queue)
        self.err = None
        self.threads = [threading.Thread(target=self._run, daemon=True) for _ in range(max(1, workers))]
        for t in self.threads:
            t.start()

    def _run(self):
        while True:
            job = self.q.get()
            if job is None:
                return
            try:
                for img, sub, name in job():
                    d = os.path.join(self.root, sub)
                    os.makedirs(d, exist_ok=True)
                    if isinstance(img, bytes):                       # a finished file (config['png_on_device'])
                        with open(os.path.join(d, name), 'wb') as fh:
                            fh.write(img)
                        continue
                    img.save(os.path.join(d, name), **({'compress_level': 1} if name.endswith('.png') else {}))
            except Exception as e:                                   # surfaced by close()
                self.err = e

    def submit(self, job):
        """job() -> iterable of (PIL image or the bytes of a finished file, sub-directory, file name); runs on a writer thread."""
        self.q.put(job)

    def close(self):
        for _ in self.threads:
            self.q.put(None)
        for t in self.threads:
            t.join()
        if self.err is not None:
            raise self.err


class FramePrefetcher:
    """Decode ahead on worker threads (the reference's DataLoader worker, inference/run_on_video.py:80-92): frames are
    requested in order and arrive as Samples whose uint8 frame is already in pinned host memory."""

    def __init__(self, reader, depth=16, workers=8):
        from concurrent.futures import ThreadPoolExecutor
        self.reader, self.depth = reader, max(1, depth)
        self.pool = ThreadPoolExecutor(max_workers=max(1, workers), thread_name_prefix='xmem-decode')
        self.futures = collections.deque()
        self.next_submit = 0

    def _load(self, idx):
        smp = self.reader[idx]
        with ops.CAPTURE_LOCK:                                   # not while the main thread captures a stage (see ops.CAPTURE_LOCK)
            if smp.rgb_u8 is None:                               # resize_on_device: the source-size frame travels
                smp.src_u8 = smp.src_u8.pin_memory()
            else:
                smp.rgb_u8 = smp.rgb_u8.pin_memory()
        return smp

    def _top_up(self):
        while self.next_submit < len(self.reader) and len(self.futures) < self.depth:
            self.futures.append(self.pool.submit(self._load, self.next_submit))
            self.next_submit += 1

    def get(self, n):
        """The next n frames, in order (blocks on the decoder only if it fell behind)."""
        self._top_up()
        out = []
        for _ in range(n):
            out.append(self.futures.popleft().result())
            self._top_up()
        return out

    def close(self):
        self.pool.shutdown(wait=False, cancel_futures=True)


def _overlay(img, mask_rgb, alpha=0.5):
    from PIL import Image
    m = np.asarray(mask_rgb.resize(img.size, Image.NEAREST) if mask_rgb.size != img.size else mask_rgb)
    fg = m.sum(-1) > 0
    a = np.full(m.shape[:2], 255, np.uint8)
    a[fg] = int(alpha * 255)
    return Image.composite(img, Image.fromarray(m), Image.fromarray(a, mode='L'))


class AsyncMaskFetcher:
    """Device->host delivery of the uint8 index masks one frame behind the GPU: the copy of frame t goes to pinned
    memory on the compute stream and is waited for only after frame t+1 has been enqueued, so the GPU never idles
    on the host round trip (the reference blocks on `.cpu()` every frame, run_on_video.py:170-172)."""

    def __init__(self, depth=3):
        self.depth = depth
        self.slots = [None] * depth
        self.pending = []          # (tag, host tensor, event)
        self._n = 0

    def submit(self, tag, mask_gpu):
        i = self._n % self.depth
        self._n += 1
        buf = self.slots[i]
        if buf is None or buf.shape != mask_gpu.shape:
            buf = torch.empty(mask_gpu.shape, dtype=torch.uint8, pin_memory=True)
            self.slots[i] = buf
        buf.copy_(mask_gpu, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((tag, buf, ev))
        ready = []
        while len(self.pending) >= self.depth:      # keep at most depth-1 frames in flight
            ready.append(self._pop())
        return ready

    def _pop(self):
        tag, buf, ev = self.pending.pop(0)
        ev.synchronize()
        return tag, buf.numpy().copy()

    def drain(self):
        out = []
        while self.pending:
            out.append(self._pop())
        return out


def _post_process_gpu(sample, prob, confidence=None, ti=None, given=False):
    """run_on_video.py:165-170 on the device: resize to the original shape if needed, argmax over classes.  `confidence`
    (config['confidence']: a `confidence.FrameConfidence`): its kernel takes the place of the argmax, yields the same mask and keeps
    frame ti's record."""
    if sample.need_resize and tuple(prob.shape[-2:]) != tuple(sample.shape):
        prob = ops.resize_bilinear(prob, sample.shape)
    if confidence is not None:
        return confidence.mask(ti, prob, sample.frame, given)
    return ops.argmax_u8(prob)


def _clean_output(spec, out_dev, totals=None):
    """config['mask_cleanup'] (as `mask_cleanup.parse_cleanup` returns it) on the index mask a frame loop is about to hand on: `out_dev`
    itself without the option - nothing is loaded or launched for it - else the cleaned mask in a tensor of its own, its four
    counters added to `totals` on the device.  The probabilities that go back into the memory are not this function's business:
    propagation is the same with and without the option, only what is written differs."""
    if spec is None:
        return out_dev
    out, stats = ops.clean_masks(out_dev, **spec)
    if totals is not None:
        totals.add_(stats)
    return out


def _cleanup_totals(spec, device):
    """the per-video sum of xmem_mask_clean's counters, kept on the device and fetched once after the loop (None without the option)"""
    return None if spec is None else torch.zeros(4, dtype=torch.int64, device=device)


def _cleanup_report(totals):
    from .mask_cleanup import STATS
    return dict(zip(STATS, (int(v) for v in totals.cpu().tolist())))


class _TrackLoop:
    """config['save_tracks'] inside a frame loop: one `ops.rle_encode` launch sequence per frame on the compute stream, the record
    delivered through pinned memory one frame behind like the mask (its own AsyncMaskFetcher, fed right before the mask's: when the
    mask of a frame has arrived, so has its record), the counts made on the host per event, the file written at the end.  A frame
    whose events did not fit is encoded again when its record arrives, and the capacity of the frames after it grows to twice its size.
    counts='compressed' (config['tracks_counts']): `ops.rle_compress` runs right behind the encoder on the same stream and what
    travels is meta + string lengths + characters, not the events; a frame whose events or characters did not fit is done again at
    its exact size when its record arrives.
    polygons (config['tracks_polygons']): `ops.mask_polygons` runs right behind the encoder (and the compressor) on the same stream,
    its record travels at the end of the same buffer, and a frame whose corners did not fit is traced again when it arrives, the
    capacity of the frames after it growing to twice its size.  Without the option nothing is loaded or launched for it."""

    def __init__(self, counts='list', polygons=None):
        from .polygons import parse_polygons
        from .rle import check_count_form
        self.counts = check_count_form(counts)
        self.polygons = parse_polygons(polygons)
        # made for the first frame's size (that of the written PNGs)
        self.writer = self.capacity = self.char_capacity = self.poly_capacity = None
        self.fetcher = AsyncMaskFetcher()

    def submit(self, tag, mask_dev, k):
        """-> the (tag, record) pairs that have arrived.  `mask_dev` must stay untouched until its record was delivered: it is
        encoded again should its events not fit."""
        if self.writer is None:
            from .rle import TrackWriter, default_capacity, default_char_capacity
            self.writer, self.capacity = TrackWriter(*mask_dev.shape, polygons=self.polygons), default_capacity(*mask_dev.shape)
            self.char_capacity = default_char_capacity(*mask_dev.shape)
            if self.polygons is not None:
                from .polygons import default_capacity as default_corners
                self.poly_capacity = default_corners(*mask_dev.shape)
        rec = ops.rle_encode(mask_dev, k, self.capacity, wait=False)
        if self.counts == 'compressed':
            from .rle import META
            srec = ops.rle_compress(rec, *mask_dev.shape, k, self.capacity, self.char_capacity, wait=False)
            parts, sizes = [rec[:k * META].view(torch.uint8), srec], (self.capacity, self.char_capacity)
        else:
            parts, sizes = [rec.view(torch.uint8)], (self.capacity,)
        if self.polygons is not None:                                # the last 4 (2 k + poly_capacity) bytes of what travels
            parts.append(ops.mask_polygons(mask_dev, k, self.poly_capacity, wait=False).view(torch.uint8))
        return self.fetcher.submit((tag, mask_dev, k) + sizes + (self.poly_capacity,),
                                   torch.cat(parts) if len(parts) > 1 else parts[0])

    def drain(self):
        return self.fetcher.drain()

    def finish(self, item, name, mapper):
        from .rle import inverse_labels, split_record
        (_, mask_dev, k, *_sizes, poly_capacity), buf = item
        rings = None
        if poly_capacity is not None:
            from .polygons import META as POLY_META
            n = 4 * (k * POLY_META + poly_capacity)
            rings, buf = self._finish_polygons(mask_dev, k, poly_capacity, buf[len(buf) - n:]), buf[:len(buf) - n]
        if self.counts == 'compressed':
            return self._finish_compressed((item[0][:-1], buf), name, mapper, rings)
        capacity = _sizes[0]
        meta, events = split_record(buf, 1, k, capacity)
        meta, events = meta[0], events[0]
        total = int(meta[:, 0].sum())
        if total > capacity:                                         # the exact size is known now: once more, nothing is cut off
            ops.RLE_STATS['retries'] += 1
            meta_all, ev_all = ops.rle_encode(mask_dev, k, capacity=total)
            meta, events = meta_all[0], ev_all[0]
            self.capacity = max(self.capacity, 2 * total)            # and the frames to come get room for a video as ragged as this
        self.writer.add_frame(name, meta, events, inverse_labels(mapper, k), polygons=rings)

    def _finish_polygons(self, mask_dev, k, capacity, buf):
        """-> (meta [k, 2], the frame's corner words) of the record that arrived; the frame is traced again when they did not fit"""
        from .polygons import split_record
        meta, corners = split_record(buf.view(np.int32), 1, k, capacity)
        meta, total = meta[0], int(meta[0, :, 0].sum())
        if total <= capacity:
            return meta, corners[0, :total]
        ops.POLY_STATS['retries'] += 1                               # the exact size is known now: once more, nothing is cut off
        meta_all, words_all = ops.mask_polygons(mask_dev, k, capacity=total)
        if (meta_all[0] != meta).any():
            raise RuntimeError('tracks_polygons: a frame traced again gave other counts')
        self.poly_capacity = max(self.poly_capacity, 2 * total)      # and the frames to come get room for a video as ragged as this
        return meta_all[0], words_all[0]

    def _finish_compressed(self, item, name, mapper, rings=None):
        from .rle import META, inverse_labels, label_strings, split_string_record
        (_, mask_dev, k, capacity, char_capacity), buf = item
        meta = buf[:4 * k * META].view(np.int32).reshape(k, META)
        str_len, chars = split_string_record(buf[4 * k * META:], 1, k, char_capacity)
        total, need = int(meta[:, 0].sum()), int(str_len[0].sum())   # need < 0: the events did not fit, no string was made
        if total > capacity or need > char_capacity:                 # the exact sizes are known now: once more, nothing is cut off
            if total > capacity:
                ops.RLE_STATS['retries'] += 1
                self.capacity = max(self.capacity, 2 * total)        # the frames to come get room for a video as ragged as this
            else:
                ops.RLE_STRING_STATS['retries'] += 1
            rec = ops.rle_encode(mask_dev, k, max(total, 1), wait=False)
            strings = ops.rle_compress(rec, *mask_dev.shape, k, max(total, 1), max(need, char_capacity))[0]
            self.char_capacity = max(self.char_capacity, 2 * sum(len(v) for v in strings))
        else:
            strings = label_strings(str_len[0], chars[0])
        self.writer.add_frame(name, meta, None, inverse_labels(mapper, k), strings=strings, polygons=rings)

    def write(self, masks_out_path):
        return self.writer.write(os.path.join(str(masks_out_path), 'tracks.json'))


def _parse_mattes(config):
    """config['mattes'] as `matte.parse_mattes` returns it; None without the key - nothing is imported for it then"""
    if config.get('mattes') is None:
        return None
    from .matte import parse_mattes
    return parse_mattes(config['mattes'])


def _parse_smooth(config):
    """config['temporal_smooth'] as `temporal.parse_smooth` returns it; None without the key - nothing is imported for it then"""
    if config.get('temporal_smooth') is None:
        return None
    from .temporal import parse_smooth
    return parse_smooth(config['temporal_smooth'])


def _parse_confidence(config):
    """config['confidence'] as `confidence.parse_confidence` returns it; None without the key - nothing is imported for it then"""
    if config.get('confidence') is None:
        return None
    from .confidence import parse_confidence
    return parse_confidence(config['confidence'])


def _frame_confidence(spec, vid_length, device, saver, config, vid_name, png_on_device):
    """config['confidence']: the loop's `confidence.FrameConfidence`; None without the option - nothing is imported, allocated or
    launched for it then"""
    if spec is None:
        return None
    from .confidence import FrameConfidence
    return FrameConfidence(spec, vid_length, device, saver, config['masks_out_path'], vid_name, png_on_device)


def _with_confidence(confidence, outputs):
    """`outputs` with the loop's FrameConfidence drained and closed beside it; `outputs` itself without the option"""
    if confidence is None:
        return outputs
    from .confidence import LoopOutputs
    return LoopOutputs(outputs, confidence)


def _with_confidence_report(df, confidence, mapper):
    """config['confidence']: the frame confidence per row in `df['confidence']` and the table in `df.attrs['confidence']` (one
    transfer, after the loop)"""
    if confidence is not None:
        df['confidence'] = confidence.frame_confidence()[:len(df)]
        df.attrs['confidence'] = confidence.report(mapper)
    return df


def _motion_frames(spec, dev_resize, source_frame):
    """config['temporal_smooth']['motion']: `frame_of(sample)`, the sample's frame at the MASK's size - the source size - for the
    motion search; None without the key.  With `resize_on_device` the source-size frame travels anyway (`src_u8`); else
    `source_frame` is the loop's way to a frame it works on at the source size, unmirrored, or None if it has no such pass - an
    error, before the loop starts."""
    if spec is None or spec.get('motion') is None:
        return None
    if dev_resize:
        return lambda sample: sample.src_u8
    if source_frame is None:
        raise ValueError("config['temporal_smooth']['motion'] needs frames of the masks' size, and this run resizes them on the host: "
                         "set config['resize_on_device'] = True, or run at the source size (config['size'] = -1)")
    return source_frame


def _source_pass(passes):
    """the index of the first of the ensemble's (working size, flip) passes that works at the source size, unmirrored; None if none"""
    return next((p for p, (size, flip) in enumerate(passes) if size < 0 and not flip), None)


def _pass_frame(p):
    """`sample -> the frame of its pass p` (an ensemble sample's `rgb_u8` is a list); None for p None"""
    return None if p is None else (lambda sample: sample.rgb_u8[p])


def _with_smoothing(spec, outputs, vid_length, device, frame_of=None):
    """config['temporal_smooth']: `outputs` behind a delay line that hands every frame on as the majority vote over its neighbours in
    time; `outputs` itself without the option - nothing is imported, allocated or launched for it then.  The vote comes after
    `_clean_output` and before everything `_FrameOutputs` does; the probabilities that go back into the memory are not touched, so
    propagation is the same with and without the option.  `frame_of`: `_motion_frames`' answer, for the compensated vote."""
    if spec is None:
        return outputs
    from .temporal import DelayLine
    return DelayLine(outputs, spec, vid_length, device, frame_of=frame_of)


def _with_smooth_report(df, outputs, say=False):
    """config['temporal_smooth']: the radius and the video's changed pixels and frames in `df.attrs['temporal_smooth']` (one transfer,
    after the loop)"""
    if hasattr(outputs, 'report'):
        df.attrs['temporal_smooth'] = outputs.report()
        if say:
            print('TEMPORAL SMOOTHING: ' + ', '.join(f'{k.replace("_", " ")} {v}' for k, v in df.attrs['temporal_smooth'].items()))
    return df


class _MatteLoop:
    """config['mattes'] inside a frame loop: one `ops.mask_mattes` launch sequence per frame on the compute stream, right behind the
    clean-up, on the index mask the loop hands on (cleaned, at the original resolution).  The planes - uint8 [T, K, H, W], one per table
    (matte, trimap) and label the mapper knows at that frame - are delivered through pinned memory one frame behind like the mask
    (their own AsyncMaskFetcher) and written by `_AsyncSaver` threads as <masks_out_path>/mattes/<label>/<frame>.png and, with a
    trimap, <masks_out_path>/trimaps/<label>/<frame>.png, 8-bit mode L, <label> the annotation's label as in tracks.json.  Masks,
    tracks and what goes back into the memory are not touched.  `saver`: the loop's, or None - then the planes get writers of
    their own, closed with the loop.  `png_on_device` (config['png_on_device']): the T x K planes of a frame are encoded as 'grey' PNGs in
    one `ops.png_encode` call right behind the look-up and the files' bytes travel, not the planes; a frame with a file that did not
    fit is encoded again when its record arrives, and the frames after it get twice that room."""

    def __init__(self, spec, saver, masks_out_path, vid_name='', png_on_device=False):
        from .matte import tables_of
        self.names, self._tables, self.R = tables_of(spec)
        self.png_on_device, self.capacity = bool(png_on_device), None
        self.own_saver = _AsyncSaver(masks_out_path, vid_name) if saver is None else None
        self.saver = self.own_saver if saver is None else saver
        self.tables = None                                           # on the device, from the first frame on
        self.fetcher = AsyncMaskFetcher()

    def submit(self, tag, mask_dev, k):
        """-> the (tag, planes) pairs that have arrived"""
        if k == 0:
            return []
        if self.tables is None:
            self.tables = torch.from_numpy(self._tables).to(mask_dev.device)
        planes = ops.mask_mattes(mask_dev, k, self.tables, self.R)
        if not self.png_on_device:
            return self.fetcher.submit((tag, k), planes)
        from .png import default_capacity
        if self.capacity is None:
            self.capacity = default_capacity(*planes.shape[-2:], 'grey')
        planes = planes.reshape((-1,) + tuple(planes.shape[-2:]))
        return self.fetcher.submit((tag, k, planes, self.capacity), ops.png_encode(planes, 'grey', capacity=self.capacity, wait=False))

    def drain(self):
        return self.fetcher.drain()

    def finish(self, item, mapper):
        from .matte import plane_job
        from .rle import inverse_labels
        if self.png_on_device:
            from .png import bytes_job, files_of_record, plane_files
            ((sample, _), k, planes_dev, capacity), buf = item

            def again(n, length):
                ops.PNG_STATS['retries'] += 1
                return ops.png_encode(planes_dev[n], 'grey', capacity=length)[0]

            def grow(length):
                self.capacity = max(self.capacity, 2 * length)
            files = files_of_record(buf, planes_dev.shape[0], capacity, again, grow)
            self.saver.submit(bytes_job(plane_files(self.names, inverse_labels(mapper, k), files, sample.frame[:-4])))
            return
        ((sample, _), k), planes = item
        self.saver.submit(plane_job(self.names, inverse_labels(mapper, k), planes, sample.frame[:-4]))

    def close(self):
        if self.own_saver is not None:
            self.own_saver.close()                                   # re-raises a writer's error


def _parse_png(config):
    """config['png_on_device'] as `png.parse_option` returns it; None without the key - nothing is imported for it then"""
    if config.get('png_on_device') is None:
        return None
    from .png import parse_option
    return parse_option(config['png_on_device'])


class _PngLoop:
    """config['png_on_device'] inside a frame loop: one `ops.png_encode` launch sequence per frame on the compute stream, on the index
    mask the loop hands on (behind the clean-up and the delay line), the record - meta and `capacity` bytes - delivered through pinned
    memory one frame behind like the mask (its own AsyncMaskFetcher, fed before the mask's: when a frame's mask has arrived, so has its
    file).  mode 'rgb': the colours `map_the_colors_back` gives the labels as of that frame, so masks/<frame>.png opens to what the
    host path writes; 'palette': the index PNG with the annotation's palette.  The tables are made per label map and stay on the
    device.  A frame whose file did not fit is encoded again at its true length when its record arrives, and the frames after it get
    twice that room.  `mask_dev` must stay untouched until then."""

    def __init__(self, spec, reader):
        self.mode, self.reader = spec['mode'], reader
        self.capacity = None                                         # made for the first frame's size
        self._tables = {}                                            # label map -> (table, palette) on the device
        self.fetcher = AsyncMaskFetcher()

    def _device_tables(self, mapper, device):
        from .png import label_map, mask_tables
        key = label_map(mapper).tobytes()
        if key not in self._tables:
            self._tables[key] = tuple(None if t is None else torch.from_numpy(t).to(device) for t in mask_tables(self.reader, mapper, self.mode))
        return self._tables[key]

    def submit(self, tag, mask_dev, mapper):
        """-> the (tag, record) pairs that have arrived"""
        if self.capacity is None:
            from .png import default_capacity
            self.capacity = default_capacity(*mask_dev.shape, self.mode)
        table, palette = self._device_tables(mapper, mask_dev.device)
        rec = ops.png_encode(mask_dev, self.mode, table, palette, capacity=self.capacity, wait=False)
        return self.fetcher.submit((tag, mask_dev, table, palette, self.capacity), rec)

    def drain(self):
        return self.fetcher.drain()

    def finish(self, item):
        """-> (the frame's name, the bytes of its file)"""
        from .png import files_of_record
        (tag, mask_dev, table, palette, capacity), buf = item

        def again(n, length):
            ops.PNG_STATS['retries'] += 1
            return ops.png_encode(mask_dev, self.mode, table, palette, capacity=length)[0]

        def grow(length):
            self.capacity = max(self.capacity, 2 * length)           # the frames to come get room for a video as ragged as this
        return tag[0].frame, files_of_record(buf, 1, capacity, again, grow)[0]


def _working_u8(src_u8, target_hw, device, flip=False):
    """resize_on_device outside the frame loop (preloads, key extraction): upload a source-size frame (or take a device one) and
    resize it on the current stream."""
    dev = src_u8.to(device)
    if tuple(dev.shape[:2]) == tuple(target_hw) and not flip:
        return dev
    return ops.resize_u8(dev, target_hw, flip=flip)


def _adopt_network(network, config, device):
    """A network that outlives the call (one per dataset, as eval.py:134-163 builds it): checked against the call's config, which then
    receives the dimensions `XMem.__init__` would have written into it.  The cores of successive calls take over each other's owner
    token and with it the captured stages (XMem.acquire_owner), so a second video of the same geometry replays instead of capturing."""
    if config.get('model') != network.model_path:
        raise ValueError(f"config['model'] = {config.get('model')!r}, but the given network was built from {network.model_path!r}")
    want = config.get('precision', os.environ.get('XMEM_PRECISION', 'fp32'))
    if want != network.precision:
        raise ValueError(f"config['precision'] = {want!r}, but the given network runs in {network.precision!r}")
    if network.device != device:
        raise ValueError(f'the given network lives on {network.device}, the call runs on {device}')
    config['key_dim'], config['value_dim'], config['hidden_dim'] = network.key_dim, network.value_dim, network.hidden_dim
    if config.get('model') is None:                                  # as a call that builds its own network says
        warn('No model weights were loaded, as config["model"] was not specified.')
    return network


def _make_network(config, device, network=None):
    if network is not None:
        return _adopt_network(network, config, device)
    model_path = config['model']
    network = XMem(config, model_path, pretrained_key_encoder=False, pretrained_value_encoder=False).to(device).eval()
    if model_path is None:
        warn('No model weights were loaded, as config["model"] was not specified.')
    return network


def _merged_config(overwrite_config, masks_out_path):
    """VIDEO_INFERENCE_CONFIG with the call's overrides; `masks_out_path` is written into the given dict too."""
    config = VIDEO_INFERENCE_CONFIG.copy()
    overwrite_config['masks_out_path'] = masks_out_path
    config.update(overwrite_config)
    return config


def _inference_device():
    if not torch.cuda.is_available():
        raise RuntimeError('xmem2_amd.run_on_video needs an MI355X (HIP) device - there is no CPU path')
    torch.autograd.set_grad_enabled(False)
    return torch.device('cuda', torch.cuda.current_device())


def _set_long_term_count_usage(config, vid_length):
    config['enable_long_term_count_usage'] = (                       # run_on_video.py:190-196
        config['enable_long_term'] and
        (vid_length / (config['max_mid_term_frames'] - config['min_mid_term_frames']) * config['num_prototypes'])
        >= config['max_long_term_elements'])


def _load_main_objects(imgs_in_path, masks_in_path, config, device, network=None):
    network = _make_network(config, device, network)
    vid_reader = VideoReader('', imgs_in_path, masks_in_path, size=config['size'], use_all_masks=True,
                             resize_on_device=config.get('resize_on_device', False))
    _set_long_term_count_usage(config, len(vid_reader))
    return MaskMapper(), InferenceCore(network, config=config), vid_reader


def hinted(order, key_batch, prefetch):
    """Yield (frame index, what `prefetch` returned for it) over `order`, hinting the key encoder ahead of the frame loop: whenever
    fewer than `key_batch` hinted frames are pending, the next `key_batch` frames IN THE DIRECTION OF TRAVEL go to
    `prefetch(list of indices) -> list` as one batch; a tail shorter than a batch goes frame by frame (no new graph shapes)."""
    key_batch = max(1, int(key_batch))
    pending, nxt = collections.deque(), 0
    for _ in order:
        if len(pending) < key_batch and nxt < len(order):
            remaining = len(order) - nxt
            n = key_batch if remaining >= key_batch else 1
            batch = list(order[nxt:nxt + n])
            pending.extend(zip(batch, prefetch(batch)))
            nxt += n
        yield pending.popleft()


def _stats_row(frame, had_mask, compute_iou, out_mask=None, gt=None):
    """One row of the returned DataFrame (run_on_video.py:115-123)."""
    stat = {'frame': frame, 'mask_provided': had_mask}
    if compute_iou:
        stat['iou'] = float(compute_array_iou(out_mask, gt)) if (gt is not None and not had_mask) else -1
    return stat


def _saver_job(reader, ids, frame, overlay_image=None, png=None):
    """The _AsyncSaver job that colour-maps the index mask `ids` and yields <frame>.png and, when `overlay_image() -> PIL image` is
    given, the overlay <frame>.jpg on it.  `png`: the bytes of <frame>.png, built on the device; the colours are then made for the
    overlay alone, and without an overlay `ids` is not looked at."""
    def job():
        from PIL import Image
        if png is not None:
            yield png, 'masks', frame[:-4] + '.png'
            if overlay_image is None:
                return
        out_img = reader.map_the_colors_back(Image.fromarray(ids))
        if png is None:
            yield out_img, 'masks', frame[:-4] + '.png'
        if overlay_image is not None:
            yield _overlay(overlay_image(), out_img), 'overlay', frame[:-4] + '.jpg'
    return job


class _FrameOutputs:
    """Everything a frame loop does with a frame's index mask once it is on the device: J&F scoring, the track record, the copy to the
    host one frame behind, and - when a frame has arrived - its stats row and its saver job.  `submit` and `drain` enqueue and wait
    (the caller times them); `deliver` is the host side of whatever arrived.  With tracks only, no mask travels: a frame is delivered
    with its record.  `reused_output`: the caller rewrites `out_dev` next frame, so the track loop, which may encode a frame again when
    its record arrives, gets a copy."""

    def __init__(self, reader, mapper, fetcher, saver=None, tracks=None, scorer=None, compute_iou=False, save_overlay=True,
                 masks_out_path=None, reused_output=False, mattes=None, pngs=None, confidence=None):
        self.reader, self.mapper, self.fetcher, self.saver, self.tracks, self.scorer = reader, mapper, fetcher, saver, tracks, scorer
        self.confidence = confidence                                 # config['confidence']: the loop's FrameConfidence, for the tracks' scores
        self.mattes = mattes                                         # config['mattes']: a _MatteLoop, None without the option
        self.pngs = pngs if saver is not None else None              # config['png_on_device']: a _PngLoop, None without the option
        self.compute_iou, self.save_overlay, self.masks_out_path, self.reused_output = compute_iou, save_overlay, masks_out_path, reused_output
        # the H x W mask itself travels only for who reads it on the host: the PNG writers and compute_iou
        self.need_mask = tracks is None or saver is not None or compute_iou
        if self.pngs is not None:                                    # the files come from the device: only the overlays and compute_iou read it
            self.need_mask = save_overlay or compute_iou
        self.stats = []
        self._arrived = ((), ())
        self._matted = ()
        self._encoded = ()

    def _tags(self, tdone):
        """no mask travels: the frames whose track record or PNG record arrived stand in for the masks that were never copied"""
        return [(it[0][0], None) for it in (tdone if self.tracks is not None else self._encoded)]

    def submit(self, ti, sample, had_mask, out_dev):
        if self.scorer is not None and sample.mask is not None:
            self.scorer.add(ti, sample.mask, out_dev, self.mapper)
        tag = (sample, had_mask)
        tdone = self.tracks.submit(tag, out_dev.clone() if self.reused_output else out_dev, len(self.mapper.labels)) \
            if self.tracks is not None else ()
        if self.mattes is not None:                                  # fed before the mask: when a frame's mask has arrived, so have its planes
            self._matted = self.mattes.submit(tag, out_dev, len(self.mapper.labels))
        if self.pngs is not None:                                    # likewise; a frame may be encoded again when its record arrives
            self._encoded = self.pngs.submit(tag, out_dev.clone() if self.reused_output else out_dev, self.mapper)
        self._arrived = tdone, (self.fetcher.submit(tag, out_dev) if self.need_mask else self._tags(tdone))

    def drain(self):
        tdone = self.tracks.drain() if self.tracks is not None else ()
        if self.mattes is not None:
            self._matted = self.mattes.drain()
        if self.pngs is not None:
            self._encoded = self.pngs.drain()
        self._arrived = tdone, (self.fetcher.drain() if self.need_mask else self._tags(tdone))

    def deliver(self, last=False):
        tdone, done = self._arrived
        self._arrived = ((), ())
        for item in tdone:
            self.tracks.finish(item, item[0][0][0].frame, self.mapper)
        for item in self._matted:
            self.mattes.finish(item, self.mapper)
        self._matted = ()
        files = dict(self.pngs.finish(item) for item in self._encoded) if self.pngs is not None else None      # by frame name
        self._encoded = ()
        for (sample, had_mask), out_mask in done:
            self.stats.append(_stats_row(sample.frame, had_mask, self.compute_iou, out_mask, sample.mask))
            if files is not None:
                overlay = self.save_overlay and out_mask is not None
                self.saver.submit(_saver_job(self.reader, self.mapper.remap_index_mask(out_mask) if overlay else None, sample.frame,
                                             (lambda s=sample: s.raw_image_pil) if overlay else None, png=files.pop(sample.frame)))
            elif self.saver is not None:
                ids = self.mapper.remap_index_mask(out_mask)         # label LUT as of this frame (cheap); the rest is off-thread
                self.saver.submit(_saver_job(self.reader, ids, sample.frame,
                                             (lambda s=sample: s.raw_image_pil) if self.save_overlay else None))
        if last and self.tracks is not None:
            if self.confidence is not None:                          # the table's one transfer, after the loop
                self.tracks.writer.set_confidence(self.confidence.track_entries(self.mapper))
            self.tracks.write(self.masks_out_path)

    def close(self):
        try:
            if self.mattes is not None:
                self.mattes.close()
        finally:
            if self.saver is not None:
                self.saver.close()                                   # re-raises a writer's error


def _run_frame_loop(vid_length, key_batch, decoder, outputs, hint, prepare, frame):
    """The frame loop of run_on_video and of the ensemble.  Frames come from `decoder` (a FramePrefetcher: the DataLoader role, outside
    the timed region, run_on_video.py:80-113) and are hinted `key_batch` ahead: `hint(samples) -> one device input per sample`.
    Per frame, `prepare(ti, sample)` is the untimed host side of an annotation (the reference converts the mask before it starts the
    clock, :94-105) and `frame(ti, sample, inputs, prepared) -> (had_mask, out_dev)` the timed step; the clock covers `frame` and
    `outputs.submit` - which includes the wait for the earlier frame's copy - and the final drain, nothing else.
    -> (total_time, loop_wall, total_wall)."""
    def prefetch(batch):
        samples = decoder.get(len(batch))
        return zip(samples, hint(samples))

    total_time, loop_t0 = 0.0, perf_counter()
    try:
        for ti, (sample, inputs) in hinted(range(vid_length), key_batch, prefetch):
            prepared = prepare(ti, sample)
            a = perf_counter()
            had_mask, out_dev = frame(ti, sample, inputs, prepared)
            outputs.submit(ti, sample, had_mask, out_dev)
            total_time += perf_counter() - a
            outputs.deliver()
        a = perf_counter()
        outputs.drain()
        total_time += perf_counter() - a
        outputs.deliver(last=True)
    finally:
        decoder.close()
        loop_wall = perf_counter() - loop_t0
        outputs.close()
        total_wall = perf_counter() - loop_t0
    return total_time, loop_wall, total_wall


def _inference_on_video(frames_with_masks, imgs_in_path, masks_in_path, masks_out_path, original_memory_mechanism=False,
                        compute_iou=False, manually_curated_masks=False, print_progress=True,
                        augment_images_with_masks=False, overwrite_config: dict = None, save_overlay=True,
                        object_color_if_single_object=(255, 255, 255), print_fps=False, image_saving_max_queue_size=200,
                        compute_jf=False, network=None):
    import pandas as pd
    device = _inference_device()
    frames_with_masks = set(frames_with_masks)
    config = _merged_config({} if overwrite_config is None else overwrite_config, masks_out_path)   # the caller's dict receives the path
    cleanup = parse_cleanup(config.get('mask_cleanup'))              # opt-in (default: absent): despeckle / fill holes / keep largest
    mattes = _parse_mattes(config)                                   # opt-in (default: absent): feathered mattes / trimaps per label
    png_spec = _parse_png(config)                                   # opt-in (default: absent): the PNG files are built on the device
    smooth = _parse_smooth(config)                                   # opt-in (default: absent): a majority vote over time
    conf_spec = _parse_confidence(config)                            # opt-in (default: absent): per-object confidence, uncertainty maps
    mapper, processor, vid_reader = _load_main_objects(imgs_in_path, masks_in_path, config, device, network=network)
    vid_length = len(vid_reader)
    motion_frames = _motion_frames(smooth, vid_reader.resize_on_device, (lambda sample: sample.rgb_u8) if vid_reader.size < 0 else None)

    to_permanent = [0] if original_memory_mechanism else sorted(frames_with_masks)
    loaded, preload_time = False, 0.0
    for j in to_permanent:                                           # _preload_permanent_memory, :201-244
        sample = vid_reader[j]
        if sample.mask is None:
            raise FileNotFoundError(f"Couldn't find mask {j}! Check that the filename is the same as for frame {j}.")
        msk, _ = mapper.convert_mask(sample.mask, exhaustive=True)
        if min(msk.shape) == 0:
            warn(f'Skipping adding frame {j} to permanent memory, as the mask is empty')
            continue
        if sample.need_resize:
            msk = vid_reader.resize_mask(msk)
        processor.set_all_labels(list(mapper.remappings.values()))
        # Opt-in (config['resize_on_device'] = True; default False): the reader hands over source-size frames and the working-size resize
        # runs on the device, in the host library's integer arithmetic - the same bytes, hence the same masks.
        dev_resize = sample.rgb_u8 is None
        a = perf_counter()
        # Opt-in (config['augment_on_device'] = True; default False): the device path is pinned to this repo's host restatement only
        # to float ties (blur within 1 LSB, < 2e-4 of the pixels of the nearest-sampling transforms, batched conv plans ~2e-4), and the
        # default output is the fp32 parity contract - a caller chooses the 20x faster preload knowingly.
        on_device = augment_images_with_masks and not sample.need_resize and config.get('augment_on_device', False)
        if on_device:
            # the annotated frame and its 11 'best_all' augmentations: made on the device in one launch, preloaded through ONE
            # batched key + value pass (the reference runs 12 sequential passes over host-side PIL transforms, :231-242).
            # With a working-size resize the reference augments BEFORE resizing: that case keeps the host path below.
            from .augmentations import augment_on_device
            rgb_dev = _working_u8(sample.src_u8, sample.target_hw, device) if dev_resize else sample.rgb_u8.to(device)
            msk_dev = msk.to(device)
            aug_rgb, aug_msk = augment_on_device(rgb_dev, msk_dev, subset='best_all')
            processor.put_many_to_permanent_memory([rgb_dev] + [aug_rgb[i] for i in range(aug_rgb.shape[0])], [msk_dev] + aug_msk)
        else:
            rgb_dev = _working_u8(sample.src_u8, sample.target_hw, device) if dev_resize else sample.rgb_u8.to(device)
            processor.put_to_permanent_memory(rgb_dev, msk.to(device))
        torch.cuda.synchronize()
        preload_time += perf_counter() - a
        loaded = True
        if augment_images_with_masks and not on_device:              # run_on_video.py:231-242, subset 'best_all' (host path)
            from .augmentations import get_determenistic_augmentations
            h, w = sample.target_hw if dev_resize else sample.rgb_u8.shape[:2]
            for img_aug, mask_aug in get_determenistic_augmentations((3, h, w), msk, subset='best_all'):
                if dev_resize:                                       # augmented at the source size on the host, resized on the device
                    rgb_aug = _working_u8(*vid_reader.frame_src_u8(img_aug(sample.raw_image_pil)), device)
                else:
                    rgb_aug = vid_reader.frame_u8(img_aug(sample.raw_image_pil)).to(device)
                processor.put_to_permanent_memory(rgb_aug, mask_aug(msk).to(device))
    if not loaded:
        raise ValueError('No valid masks provided!')

    scorer = InLoopScorer(vid_length, device) if compute_jf else None
    cleaned = _cleanup_totals(cleanup, device)
    # Opt-in (config['save_tracks'] = True; default False): the device finds the run boundaries, the host receives those (rle.py).
    saver = _AsyncSaver(config['masks_out_path'], vid_reader.vid_name, image_saving_max_queue_size) if config['save_masks'] else None
    conf = _frame_confidence(conf_spec, vid_length, device, saver, config, vid_reader.vid_name, png_spec is not None)
    outputs = _FrameOutputs(
        vid_reader, mapper, AsyncMaskFetcher(), saver=saver,
        tracks=_TrackLoop(config.get('tracks_counts', 'list'), config.get('tracks_polygons')) if config.get('save_tracks', False) else None,
        scorer=scorer,
        compute_iou=compute_iou, save_overlay=save_overlay, masks_out_path=config['masks_out_path'],
        mattes=None if mattes is None else _MatteLoop(mattes, saver, config['masks_out_path'], vid_reader.vid_name, png_spec is not None),
        pngs=None if png_spec is None or saver is None else _PngLoop(png_spec, vid_reader), confidence=conf)
    outputs = _with_confidence(conf, _with_smoothing(smooth, outputs, vid_length, device, motion_frames))

    def hint(samples):
        if samples[0].rgb_u8 is None:                                # resize_on_device: source frames; H2D + resize on the side stream too
            return processor.prefetch_keys([smp.src_u8 for smp in samples], working_size=samples[0].target_hw)
        return processor.prefetch_keys([smp.rgb_u8 for smp in samples])      # uint8 H2D + normalise + key encoder, side stream

    def prepare(ti, sample):
        if ti not in frames_with_masks or sample.mask is None:
            return None
        msk, labels = mapper.convert_mask(sample.mask, exhaustive=True)
        if sample.need_resize:
            msk = vid_reader.resize_mask(msk)
        processor.set_all_labels(list(mapper.remappings.values()))
        return msk.to(device), labels

    def frame(ti, sample, rgb, given):
        msk, labels = given or (None, None)
        skip_add = (ti == 0) if original_memory_mechanism else (msk is not None)
        prob = processor.step(rgb, msk, labels, end=(ti == vid_length - 1),
                              manually_curated_masks=manually_curated_masks, do_not_add_mask_to_memory=skip_add)
        raw = _post_process_gpu(sample, prob) if conf is None else _post_process_gpu(sample, prob, conf, ti, msk is not None)
        return msk is not None, _clean_output(cleanup, raw, cleaned)

    key_batch = max(1, int(config.get('key_batch', 4)))                # frames per batched key-encoder hint
    decoder = FramePrefetcher(vid_reader, depth=4 * key_batch, workers=int(config.get('decode_workers', 8)))
    total_time, loop_wall, total_wall = _run_frame_loop(vid_length, key_batch, decoder, outputs, hint, prepare, frame)
    if print_fps:
        print(f'TOTAL PRELOADING TIME: {preload_time:.4f}s')
        print(f'TOTAL PROCESSING TIME: {total_time:.4f}s')
        print(f'TOTAL PROCESSING FPS: {vid_length / total_time:.4f}')
        print(f'TOTAL FPS (excluding image saving): {vid_length / (preload_time + total_time):.4f}')
        print(f'WALL-CLOCK FPS of the frame loop incl. decode: {vid_length / loop_wall:.4f}; incl. writing every mask: '
              f'{vid_length / total_wall:.4f}')
    df = _with_smooth_report(_with_cleanup(_with_jf(pd.DataFrame(outputs.stats), scorer), cleaned, print_fps), outputs, print_fps)
    return _with_confidence_report(df, conf, mapper)


def _with_cleanup(df, totals, say=False):
    """config['mask_cleanup']: the video's totals of the four counters in `df.attrs['cleanup']` (one transfer, after the loop)"""
    if totals is not None:
        df.attrs['cleanup'] = _cleanup_report(totals)
        if say:
            print('MASK CLEAN-UP: ' + ', '.join(f'{k.replace("_", " ")} {v}' for k, v in df.attrs['cleanup'].items()))
    return df


def _with_jf(df, scorer):
    """compute_jf=True: the J and F columns (per-frame means over the sequence's ground-truth objects, NaN without a ground truth)."""
    if scorer is not None:
        df['J'], df['F'] = scorer.scores()
    return df


def run_on_video(imgs_in_path, masks_in_path, masks_out_path, frames_with_masks: Iterable[int] = (0,),
                 compute_iou=False, print_progress=True, network=None, **kwargs):
    """Same signature / return as inference/run_on_video.py:247-282: per-frame stats DataFrame
    (frame, mask_provided[, iou]); predicted masks are written under ``masks_out_path/masks``.
    ``compute_jf=True`` adds DAVIS J and F columns, scored on the device against every frame's ground truth
    (xmem2_amd.metrics; frames without one get NaN).
    ``network``: an `XMem` to run on instead of building one from ``config['model']`` (which, like ``config['precision']``, must
    agree with it): its weights stay uploaded and its captured stages are replayed by the next call of the same geometry."""
    return _inference_on_video(network=network, imgs_in_path=imgs_in_path, masks_in_path=masks_in_path, masks_out_path=masks_out_path,
                               frames_with_masks=frames_with_masks, compute_iou=compute_iou,
                               print_progress=print_progress, **kwargs)


MAX_ENSEMBLE_PASSES = 16


def parse_ensemble(spec, size):
    """overwrite_config['ensemble'] -> tuple of (size, flip) passes.  `size` means what config['size'] means (-1: native);
    absent (None): the flip ensemble at `size`.  Duplicates are kept (each is a pass of its own)."""
    if spec is None:
        spec = [[size, False], [size, True]]
    if not isinstance(spec, (list, tuple)) or not spec:
        raise ValueError('ensemble: expected a non-empty list of [size, flip] passes')
    if len(spec) > MAX_ENSEMBLE_PASSES:
        raise ValueError(f'ensemble: {len(spec)} passes, at most {MAX_ENSEMBLE_PASSES}')
    passes = []
    for item in spec:
        if not isinstance(item, (list, tuple)) or len(item) != 2:
            raise ValueError(f'ensemble: pass {item!r} is not a [size, flip] pair')
        s, f = item
        if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)) or not (s == -1 or s > 0):
            raise ValueError(f'ensemble: size {s!r} must be an integer > 0, or -1 for the native size')
        if not isinstance(f, (bool, np.bool_)) and f not in (0, 1):
            raise ValueError(f'ensemble: flip {f!r} must be a boolean')
        passes.append((int(s), bool(f)))
    return tuple(passes)


def _mirror(a):
    """Horizontal flip of an H x W [x 3] host array (torch.flip(x, dims=[-1]) of eval.py:217-218 in the array's own layout)."""
    return np.ascontiguousarray(a[:, ::-1])


@dataclass
class EnsembleSample:
    """One decoded frame and its per-pass inputs: `rgb_u8[p]` is pass p's working-size (mirrored if asked) uint8 frame, `mask` the
    annotation's raw index array at the ORIGINAL resolution (each pass mirrors it before its own convert / resize).  With
    `resize_on_device` readers `rgb_u8` is None and `src_u8` the one decoded source-size frame every variant is made from on the
    device."""
    rgb_u8: Optional[list]
    raw_image_pil: object
    frame: str
    save: bool
    shape: tuple
    mask: Optional[np.ndarray] = None
    src_u8: Optional[torch.Tensor] = None


class EnsembleFramePrefetcher(FramePrefetcher):
    """FramePrefetcher for an ensemble: each frame is decoded ONCE on a worker thread, resized once per distinct working size
    (PIL bilinear, VideoReader.frame_u8) and mirrored there for the flipped passes; passes with the same (size, flip) share one
    array.  The arrays are pinned by `get`, on the calling thread, not on the workers: the P cores capture their graphs over the first
    frames while the workers decode ahead, and with the pinning on the workers captures failed (hipErrorStreamCaptureInvalidated, in a
    conv launch of a later core's first key-encoder capture) - the pinned-memory allocator queries events, which a capture in progress
    on another thread does not allow."""

    def __init__(self, readers, passes, depth=16, workers=8):
        super().__init__(readers[passes[0][0]], depth=depth, workers=workers)
        self.readers, self.passes = readers, passes

    def _load(self, idx):
        base = self.reader[idx]                                   # decode + the first pass's size (+ the raw annotation)
        if base.rgb_u8 is None:                                   # resize_on_device: one source frame, the variants are made on the device
            return EnsembleSample(rgb_u8=None, raw_image_pil=base.raw_image_pil, frame=base.frame, save=base.save, shape=base.shape,
                                  mask=base.mask, src_u8=base.src_u8)
        by_size = {self.passes[0][0]: base.rgb_u8}
        variants = {}
        for s, f in self.passes:
            if (s, f) not in variants:
                if s not in by_size:
                    by_size[s] = self.readers[s].frame_u8(base.raw_image_pil)
                a = by_size[s]
                variants[(s, f)] = torch.from_numpy(_mirror(a.numpy())) if f else a
        return EnsembleSample(rgb_u8=[variants[p] for p in self.passes], raw_image_pil=base.raw_image_pil, frame=base.frame,
                              save=base.save, shape=base.shape, mask=base.mask)

    def get(self, n):
        out = super().get(n)
        for smp in out:
            if smp.rgb_u8 is None:
                smp.src_u8 = smp.src_u8.pin_memory()
                continue
            pinned = {}
            for t in smp.rgb_u8:
                if id(t) not in pinned:
                    pinned[id(t)] = t.pin_memory()
            smp.rgb_u8 = [pinned[id(t)] for t in smp.rgb_u8]
        return out


def _pass_mask(mapper, reader, raw, flip, need_resize):
    """eval.py:191-200 for one pass: mirror the raw index mask, then convert_mask, then the nearest resize (the nearest resize is
    not mirror-symmetric, so the order matters)."""
    msk, labels = mapper.convert_mask(_mirror(raw) if flip else raw, exhaustive=True)
    if need_resize:
        msk = reader.resize_mask(msk)
    return msk, labels


def _ensemble_on_video(frames_with_masks, imgs_in_path, masks_in_path, masks_out_path, original_memory_mechanism=False,
                       compute_iou=False, manually_curated_masks=False, print_progress=True,
                       augment_images_with_masks=False, overwrite_config: dict = None, save_overlay=True,
                       object_color_if_single_object=(255, 255, 255), print_fps=False, image_saving_max_queue_size=200,
                       compute_jf=False, network=None):
    import pandas as pd
    config = _merged_config(dict(overwrite_config or {}), masks_out_path)           # on a copy: the caller's dict stays as it is
    passes = parse_ensemble(config.get('ensemble'), config['size'])
    cleanup = parse_cleanup(config.get('mask_cleanup'))
    mattes = _parse_mattes(config)
    png_spec = _parse_png(config)
    smooth = _parse_smooth(config)
    conf_spec = _parse_confidence(config)
    if augment_images_with_masks:
        raise NotImplementedError('run_on_video_ensemble: augment_images_with_masks is not supported (the augmented preload is '
                                  'defined for one working size and orientation); run the passes without it')
    device = _inference_device()                                     # after the errors of the call itself, which need no device
    frames_with_masks = set(frames_with_masks)
    P = len(passes)

    # one network (weights uploaded and transformed once), one InferenceCore + MaskMapper per pass
    network = _make_network(config, device, network)
    dev_resize = bool(config.get('resize_on_device', False))        # opt-in: one decode, one upload, every (size, flip) variant by kernel
    readers = {}
    for s, _ in passes:
        if s not in readers:
            readers[s] = VideoReader('', imgs_in_path, masks_in_path, size=s, use_all_masks=True, resize_on_device=dev_resize)
    vid_reader = readers[passes[0][0]]
    vid_length = len(vid_reader)
    motion_frames = _motion_frames(smooth, dev_resize, _pass_frame(_source_pass(passes)))
    _set_long_term_count_usage(config, vid_length)                   # once for all passes
    mappers = [MaskMapper() for _ in passes]
    cores = [InferenceCore(network, config=config) for _ in passes]

    def pass_masks(raw):
        """per-pass (one-hot mask, labels); every mapper sees the same annotation, so their remappings must agree"""
        out = [_pass_mask(mappers[p], readers[s], raw, f, s >= 0) for p, (s, f) in enumerate(passes)]
        for m in mappers[1:]:
            assert m.remappings == mappers[0].remappings and m.labels == mappers[0].labels, 'ensemble: pass label maps diverged'
        return out

    to_permanent = [0] if original_memory_mechanism else sorted(frames_with_masks)
    loaded, preload_time = False, 0.0
    for j in to_permanent:                                           # _preload_permanent_memory, :201-244, per pass
        sample = vid_reader[j]
        if sample.mask is None:
            raise FileNotFoundError(f"Couldn't find mask {j}! Check that the filename is the same as for frame {j}.")
        per_pass = pass_masks(sample.mask)
        if min(per_pass[0][0].shape) == 0:
            warn(f'Skipping adding frame {j} to permanent memory, as the mask is empty')
            continue
        by_size = {passes[0][0]: sample.rgb_u8}
        a = perf_counter()
        src_dev, variants = (sample.src_u8.to(device), {}) if dev_resize else (None, None)
        for p, (s, f) in enumerate(passes):
            if dev_resize:
                if (s, f) not in variants:
                    variants[(s, f)] = _working_u8(src_dev, readers[s]._target_hw(*sample.shape), device, flip=f)
                rgb = variants[(s, f)]
            else:
                if s not in by_size:
                    by_size[s] = readers[s].frame_u8(sample.raw_image_pil)
                rgb = torch.from_numpy(_mirror(by_size[s].numpy())) if f else by_size[s]
            cores[p].set_all_labels(list(mappers[p].remappings.values()))
            cores[p].put_to_permanent_memory(rgb.to(device), per_pass[p][0].to(device))
        torch.cuda.synchronize()
        preload_time += perf_counter() - a
        loaded = True
    if not loaded:
        raise ValueError('No valid masks provided!')

    mapper = mappers[0]
    scorer = InLoopScorer(vid_length, device) if compute_jf else None
    cleaned = _cleanup_totals(cleanup, device)
    saver = _AsyncSaver(config['masks_out_path'], vid_reader.vid_name, image_saving_max_queue_size) if config['save_masks'] else None
    conf = _frame_confidence(conf_spec, vid_length, device, saver, config, vid_reader.vid_name, png_spec is not None)
    outputs = _FrameOutputs(                                         # on the merged mask, a buffer the next frame writes again - unless cleaned
        vid_reader, mapper, AsyncMaskFetcher(), saver=saver,
        tracks=_TrackLoop(config.get('tracks_counts', 'list'), config.get('tracks_polygons')) if config.get('save_tracks', False) else None,
        scorer=scorer,
        compute_iou=compute_iou, save_overlay=save_overlay, masks_out_path=config['masks_out_path'], reused_output=cleanup is None,
        mattes=None if mattes is None else _MatteLoop(mattes, saver, config['masks_out_path'], vid_reader.vid_name, png_spec is not None),
        pngs=None if png_spec is None or saver is None else _PngLoop(png_spec, vid_reader), confidence=conf)
    outputs = _with_confidence(conf, _with_smoothing(smooth, outputs, vid_length, device, motion_frames))
    bufs = {}                                                        # (C, H, W) -> (uint16 score sum, uint8 merged mask)

    def hint(samples):
        if dev_resize:
            # one upload per frame; the first pass of each (size, flip) makes that variant on the side stream (copy, resize / mirror and
            # key pass are stream-ordered there: inputs_complete), later passes with the same variant hint the same tensors
            srcs = cores[0].upload_frames([smp.src_u8 for smp in samples])
            made, devs = {}, []
            for p, (s, f) in enumerate(passes):
                if (s, f) not in made:
                    made[(s, f)] = cores[p].prefetch_keys(srcs, inputs_complete=True, flip=f,
                                                          working_size=readers[s]._target_hw(*samples[0].shape))
                else:
                    cores[p].prefetch_keys(made[(s, f)], inputs_complete=True)
                devs.append(made[(s, f)])
        else:
            devs = [cores[p].prefetch_keys([smp.rgb_u8[p] for smp in samples]) for p in range(P)]   # each core hints its own variants
        return [[devs[p][i] for p in range(P)] for i in range(len(samples))]

    def prepare(ti, sample):
        return pass_masks(sample.mask) if ti in frames_with_masks and sample.mask is not None else None

    def frame(ti, sample, rgbs, per_pass):
        given = per_pass is not None
        skip_add = (ti == 0) if original_memory_mechanism else given
        H, W = sample.shape
        for p, (s, f) in enumerate(passes):
            msk = labels = None
            if given:
                msk, labels = per_pass[p][0].to(device), per_pass[p][1]
                cores[p].set_all_labels(list(mappers[p].remappings.values()))
            prob = cores[p].step(rgbs[p], msk, labels, end=(ti == vid_length - 1),
                                 manually_curated_masks=manually_curated_masks, do_not_add_mask_to_memory=skip_add)
            shp = (prob.shape[0], H, W)                              # one pair per object count (a late object adds a class)
            if shp not in bufs:
                bufs[shp] = (torch.empty(shp, dtype=torch.uint16, device=device), torch.empty((H, W), dtype=torch.uint8, device=device))
            acc, merged = bufs[shp]
            ops.ensemble_accumulate(prob, (H, W), f, acc, first=(p == 0), out=merged if p == P - 1 and conf is None else None)
        if conf is not None:                                         # the same first-index argmax of the sum, and the frame's record
            conf.mask(ti, acc, sample.frame, given, passes=P, out=merged)
        return given, _clean_output(cleanup, merged, cleaned)        # cleaned: into a tensor of its own, `merged` is rewritten next frame

    key_batch = max(1, int(config.get('key_batch', 4)))
    decoder = EnsembleFramePrefetcher(readers, passes, depth=4 * key_batch, workers=int(config.get('decode_workers', 8)))
    total_time, loop_wall, total_wall = _run_frame_loop(vid_length, key_batch, decoder, outputs, hint, prepare, frame)
    if print_fps:
        print(f'ENSEMBLE PASSES: {P} (' + ', '.join(str(s) + (' flip' if f else '') for s, f in passes) + ')')
        print(f'TOTAL PRELOADING TIME: {preload_time:.4f}s')
        print(f'TOTAL PROCESSING TIME: {total_time:.4f}s')
        print(f'TOTAL PROCESSING FPS: {vid_length / total_time:.4f} (ensemble of {P} passes; {P * vid_length / total_time:.4f} passes/s)')
        print(f'WALL-CLOCK FPS of the frame loop incl. decode: {vid_length / loop_wall:.4f}; incl. writing every mask: '
              f'{vid_length / total_wall:.4f}')
    df = _with_smooth_report(_with_cleanup(_with_jf(pd.DataFrame(outputs.stats), scorer), cleaned, print_fps), outputs, print_fps)
    return _with_confidence_report(df, conf, mapper)


def run_on_video_ensemble(imgs_in_path, masks_in_path, masks_out_path, frames_with_masks: Iterable[int] = (0,),
                          compute_iou=False, print_progress=True, network=None, **kwargs):
    """The test-time ensemble of eval.py (--size S [--flip] --save_scores, one run per pass) + merge_multi_scale.py, in one process on
    one network: `overwrite_config['ensemble']` lists the [size, flip] passes (default: [[size, False], [size, True]]).  Every pass
    runs its own InferenceCore; per frame, each pass's probabilities are resized to the original size, un-flipped, quantised to
    uint8 and summed on the device, and the argmax of the sum is the written mask.  Same signature and return as run_on_video
    (``network`` included)."""
    return _ensemble_on_video(network=network, imgs_in_path=imgs_in_path, masks_in_path=masks_in_path, masks_out_path=masks_out_path,
                              frames_with_masks=frames_with_masks, compute_iou=compute_iou,
                              print_progress=print_progress, **kwargs)


def _pil_to_tensor01(pic):
    """What torchvision's ToTensor yields for the PNG modes the harness writes/reads (run_on_video.py:334,362):
    uint8 planes scaled by 1/255, C x H x W; palette images contribute their raw INDEX plane (so object id 1 becomes
    1/255 - the reference feeds exactly that to the selector)."""
    arr = np.array(pic, copy=True)
    if pic.mode == '1':
        arr = arr.astype(np.uint8) * 255
    if arr.ndim == 2:
        arr = arr[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))
    return t.to(torch.float32).div(255) if t.dtype == torch.uint8 else t.to(torch.float32)


def select_k_next_best_annotation_candidates(imgs_in_path, masks_in_path, masks_out_path=None, k: int = 5,
                                             print_progress=True, previously_chosen_candidates=[0],
                                             use_previously_predicted_masks=True, alpha=0.5,
                                             min_mask_presence_percent=0.25, network=None, **kwargs):
    """inference/run_on_video.py:285-370, same arguments and return (list of new frame indices).  ``network``: as in run_on_video."""
    import tempfile
    from pathlib import Path
    from PIL import Image
    from .frame_selection import extract_keys, select_next_candidates

    if not torch.cuda.is_available():
        raise RuntimeError('xmem2_amd needs an MI355X (HIP) device - there is no CPU path')
    device = torch.device('cuda', torch.cuda.current_device())
    config = dict(VIDEO_INFERENCE_CONFIG)
    config.update(kwargs.get('overwrite_config') or {})     # the reference extracts keys with the default config
    _, processor, vid_reader = _load_main_objects(imgs_in_path, masks_in_path, config, device, network=network)   # honours config['resize_on_device']
    frame_keys, shrinkages, selections, *_ = extract_keys(vid_reader, processor, print_progress=print_progress,
                                                          flatten=False, keep_on_device=True)
    tmp = None
    p_masks_out = Path(masks_out_path) if masks_out_path is not None else None
    if use_previously_predicted_masks:
        assert masks_out_path is not None, \
            'When `use_existing_masks=True`, you need to put the path to previously predicted masks in `masks_out_path`'
    else:
        if p_masks_out is None:
            tmp = tempfile.TemporaryDirectory()
            p_masks_out = Path(tmp.name)
        run_on_video(imgs_in_path=imgs_in_path, masks_in_path=masks_in_path, masks_out_path=p_masks_out,
                     frames_with_masks=previously_chosen_candidates, compute_iou=False, print_progress=print_progress,
                     network=network, **kwargs)
    try:
        masks = [_pil_to_tensor01(Image.open(p)) for p in sorted((p_masks_out / 'masks').iterdir())]
    except Exception:
        warn('Loading previously predicting masks failed for `select_k_next_best_annotation_candidates`.')
        raise
    if len(masks) != len(frame_keys):
        raise FileNotFoundError(f'Not enough masks ({len(masks)}) for {len(frame_keys)} frames provided when using '
                                f'`use_previously_predicted_masks=True`!')
    chosen = select_next_candidates(torch.cat(frame_keys), shrinkages=torch.cat(shrinkages), selections=torch.cat(selections),
                                    masks=masks, num_next_candidates=k,
                                    previously_chosen_candidates=previously_chosen_candidates, print_progress=print_progress,
                                    alpha=alpha, only_new_candidates=True,
                                    min_mask_presence_percent=min_mask_presence_percent, device=device)
    if tmp is not None:
        tmp.cleanup()
    return chosen
