"""The output side of the frame loops: everything that happens to a frame's index mask once it is on the device.

`_FrameOutputs` feeds the J&F scorer, an ordered list of side channels and the mask copy, and - when a frame has arrived - makes its
stats row and its saver job.  A side channel (`_Channel`: the tracks, the mattes, the device-built PNGs) launches on the compute
stream, sends its record through pinned memory one frame behind through an `AsyncMaskFetcher` of its own, and looks at the record when
it arrives; a record that did not fit is made again at its exact size, and `_Room` gives the frames after it twice that.  What
travels with a record is a `Tag`.  `_PlaneChannel` delivers uint8 planes as files, raw or encoded on the device; the mattes and the
uncertainty maps (`confidence.FrameConfidence`) both go through it.

`loop_outputs` is the set-up of both runners (option parsing, saver, channels, delay line) and `loop_report` their returned DataFrame.
Without an option's key nothing is imported, allocated or launched for it.
"""
import os
import queue
import threading
from contextlib import ExitStack
from dataclasses import dataclass, replace
from importlib import import_module

import numpy as np
import torch

from . import ops
from .mask_cleanup import parse_cleanup
from .tensor_util import compute_array_iou


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


# ---- the side channels -------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Tag:
    """What travels with a record through an AsyncMaskFetcher: the frame it belongs to and, where a channel sent it, what a frame done
    again needs - the device tensors it reads and the room its record was made with."""
    frame: str
    sample: object = None
    had_mask: bool = False
    k: int = 0                                                       # the objects known when the frame was sent
    dev: tuple = ()
    room: tuple = ()


class _Room:
    """The room a channel's records start with and how it grows: `of(shape)` is `module.default(*shape, *extra)` of the first frame's
    shape - looked up then, not before - and `overflow(need)` counts one retry in `stats` and gives the frames to come twice the room
    of the one that did not fit, for a video as ragged as this."""

    def __init__(self, module, stats, default='default_capacity', extra=()):
        self.module, self.stats, self.default, self.extra, self.size = module, stats, default, tuple(extra), None

    def of(self, *shape):
        if self.size is None:
            self.size = getattr(import_module('.' + self.module, __package__), self.default)(*shape, *self.extra)
        return self.size

    def overflow(self, need, counted=True):
        if counted:
            self.stats['retries'] += 1
        self.size = max(self.size, 2 * need)


class _Channel:
    """A side output of the frame loop: `submit(tag, mask_dev, mapper)` launches on the compute stream and sends the record through its
    one AsyncMaskFetcher, `submit` and `drain` return the (tag, record) pairs that have arrived, `finish(item, mapper)` is the host
    side of one of them.  `rereads`: `finish` may read `mask_dev` again - a caller that rewrites its tensor hands over a copy.
    `every_frame`: a record arrives for every frame that was submitted."""
    rereads, every_frame = False, True

    def __init__(self):
        self.fetcher = AsyncMaskFetcher()

    def drain(self):
        return self.fetcher.drain()

    def close(self):
        pass


class _TrackLoop(_Channel):
    """config['save_tracks'] inside a frame loop: one `ops.rle_encode` launch sequence per frame, the counts made on the host per
    event, the file written at the end.  A frame whose events did not fit is encoded again when its record arrives.
    counts='compressed' (config['tracks_counts']): `ops.rle_compress` runs right behind the encoder on the same stream and what
    travels is meta + string lengths + characters, not the events; a frame whose events or characters did not fit is done again at
    its exact size when its record arrives.
    polygons (config['tracks_polygons']): `ops.mask_polygons` runs right behind the encoder (and the compressor) on the same stream,
    its record travels at the end of the same buffer, and a frame whose corners did not fit is traced again when it arrives.  Without
    the option nothing is loaded or launched for it.
    The three records differ in layout, so each is parsed by its own code; the room rule and the delivery are the shared ones."""
    rereads = True

    def __init__(self, counts='list', polygons=None):
        from .polygons import parse_polygons
        from .rle import check_count_form
        super().__init__()
        self.counts = check_count_form(counts)
        self.polygons = parse_polygons(polygons)
        self.writer = None                                           # made for the first frame's size (that of the written PNGs)
        self.events, self.chars = _Room('rle', ops.RLE_STATS), _Room('rle', ops.RLE_STRING_STATS, 'default_char_capacity')
        self.corners = _Room('polygons', ops.POLY_STATS)

    def submit(self, tag, mask_dev, mapper):
        k = len(mapper.labels)
        if self.writer is None:
            from .rle import TrackWriter
            self.writer = TrackWriter(*mask_dev.shape, polygons=self.polygons)
        capacity, char_capacity = self.events.of(*mask_dev.shape), self.chars.of(*mask_dev.shape)
        poly_capacity = self.corners.of(*mask_dev.shape) if self.polygons is not None else None
        rec = ops.rle_encode(mask_dev, k, capacity, wait=False)
        if self.counts == 'compressed':
            from .rle import META
            parts = [rec[:k * META].view(torch.uint8), ops.rle_compress(rec, *mask_dev.shape, k, capacity, char_capacity, wait=False)]
        else:
            parts = [rec.view(torch.uint8)]
        if self.polygons is not None:                                # the last 4 (2 k + poly_capacity) bytes of what travels
            parts.append(ops.mask_polygons(mask_dev, k, poly_capacity, wait=False).view(torch.uint8))
        return self.fetcher.submit(replace(tag, k=k, dev=(mask_dev,), room=(capacity, char_capacity, poly_capacity)),
                                   torch.cat(parts) if len(parts) > 1 else parts[0])

    def finish(self, item, mapper):
        from .rle import inverse_labels
        tag, buf = item
        rings = None
        if self.polygons is not None:
            from .polygons import META as POLY_META
            n = 4 * (tag.k * POLY_META + tag.room[2])
            rings, buf = self._polygons(tag, buf[len(buf) - n:]), buf[:len(buf) - n]
        meta, events, strings = self._strings(tag, buf) if self.counts == 'compressed' else self._events(tag, buf)
        self.writer.add_frame(tag.frame, meta, events, inverse_labels(mapper, tag.k), strings=strings, polygons=rings)

    def _events(self, tag, buf):
        """-> (meta, events, None) of the record that arrived; the frame is encoded again when its events did not fit"""
        from .rle import split_record
        (mask_dev,), capacity = tag.dev, tag.room[0]
        meta, events = split_record(buf, 1, tag.k, capacity)
        meta, events = meta[0], events[0]
        total = int(meta[:, 0].sum())
        if total > capacity:                                         # the exact size is known now: once more, nothing is cut off
            self.events.overflow(total)
            meta_all, ev_all = ops.rle_encode(mask_dev, tag.k, capacity=total)
            meta, events = meta_all[0], ev_all[0]
        return meta, events, None

    def _polygons(self, tag, buf):
        """-> (meta [k, 2], the frame's corner words) of the record that arrived; the frame is traced again when they did not fit"""
        from .polygons import split_record
        (mask_dev,), capacity = tag.dev, tag.room[2]
        meta, corners = split_record(buf.view(np.int32), 1, tag.k, capacity)
        meta, total = meta[0], int(meta[0, :, 0].sum())
        if total <= capacity:
            return meta, corners[0, :total]
        self.corners.overflow(total)                                 # the exact size is known now: once more, nothing is cut off
        meta_all, words_all = ops.mask_polygons(mask_dev, tag.k, capacity=total)
        if (meta_all[0] != meta).any():
            raise RuntimeError('tracks_polygons: a frame traced again gave other counts')
        return meta_all[0], words_all[0]

    def _strings(self, tag, buf):
        """-> (meta, None, the labels' strings) of the record that arrived.  An overflow of the events counts as theirs alone, and its
        retry makes the strings too; the characters' room grows to twice what the strings made again need."""
        from .rle import META, label_strings, split_string_record
        (mask_dev,), (capacity, char_capacity, _), k = tag.dev, tag.room, tag.k
        meta = buf[:4 * k * META].view(np.int32).reshape(k, META)
        str_len, chars = split_string_record(buf[4 * k * META:], 1, k, char_capacity)
        total, need = int(meta[:, 0].sum()), int(str_len[0].sum())   # need < 0: the events did not fit, no string was made
        if total <= capacity and need <= char_capacity:
            return meta, None, label_strings(str_len[0], chars[0])
        if total > capacity:                                         # the exact sizes are known now: once more, nothing is cut off
            self.events.overflow(total)
        rec = ops.rle_encode(mask_dev, k, max(total, 1), wait=False)
        strings = ops.rle_compress(rec, *mask_dev.shape, k, max(total, 1), max(need, char_capacity))[0]
        self.chars.overflow(sum(len(v) for v in strings), counted=total <= capacity)
        return meta, None, strings

    def write(self, masks_out_path):
        return self.writer.write(os.path.join(str(masks_out_path), 'tracks.json'))


class _PngLoop(_Channel):
    """config['png_on_device'] inside a frame loop: one `ops.png_encode` launch sequence per frame on the index mask the loop hands on
    (behind the clean-up and the delay line), the record being meta and the room's bytes.  mode 'rgb': the colours
    `map_the_colors_back` gives the labels as of that frame, so masks/<frame>.png opens to what the host path writes; 'palette': the
    index PNG with the annotation's palette.  The tables are made per label map and stay on the device.  A frame whose file did not
    fit is encoded again at its true length when its record arrives.  `files`: the finished files by frame name, for the frame's
    saver job to take."""
    rereads = True

    def __init__(self, spec, reader):
        super().__init__()
        self.mode, self.reader = spec['mode'], reader
        self.room = _Room('png', ops.PNG_STATS, extra=(self.mode,))
        self._tables = {}                                            # label map -> (table, palette) on the device
        self.files = {}

    def _device_tables(self, mapper, device):
        from .png import label_map, mask_tables
        key = label_map(mapper).tobytes()
        if key not in self._tables:
            self._tables[key] = tuple(None if t is None else torch.from_numpy(t).to(device) for t in mask_tables(self.reader, mapper, self.mode))
        return self._tables[key]

    def submit(self, tag, mask_dev, mapper):
        room = self.room.of(*mask_dev.shape)
        table, palette = self._device_tables(mapper, mask_dev.device)
        rec = ops.png_encode(mask_dev, self.mode, table, palette, capacity=room, wait=False)
        return self.fetcher.submit(replace(tag, dev=(mask_dev, table, palette), room=(room,)), rec)

    def finish(self, item, mapper):
        from .png import files_of_record
        tag, buf = item
        mask_dev, table, palette = tag.dev

        def again(n, length):
            return ops.png_encode(mask_dev, self.mode, table, palette, capacity=length)[0]
        self.files[tag.frame] = files_of_record(buf, 1, tag.room[0], again, self.room.overflow)[0]


class _PlaneChannel(_Channel):
    """uint8 planes [..., H, W] of a frame as 8-bit grey PNG files, one per plane, written by `_AsyncSaver` threads: `send` puts them on
    their way and `write` gives every plane of an arrived record its (sub-directory, file name).  `png_on_device`
    (config['png_on_device']): the planes of a frame are encoded as 'grey' PNGs in one `ops.png_encode` call and the files' bytes
    travel, not the planes; a frame with a file that did not fit is encoded again when its record arrives.  `saver`: the loop's, or
    None - then the planes get writers of their own, closed with the channel."""

    def __init__(self, saver, masks_out_path, vid_name='', png_on_device=False):
        super().__init__()
        self.png_on_device, self.room = bool(png_on_device), _Room('png', ops.PNG_STATS, extra=('grey',))
        self.own_saver = _AsyncSaver(masks_out_path, vid_name) if saver is None else None
        self.saver = self.own_saver if saver is None else saver

    def send(self, tag, planes):
        """-> the (tag, record) pairs that have arrived"""
        if not self.png_on_device:
            return self.fetcher.submit(tag, planes)
        room = self.room.of(*planes.shape[-2:])
        planes = planes.reshape((-1,) + tuple(planes.shape[-2:]))
        return self.fetcher.submit(replace(tag, dev=(planes,), room=(room,)), ops.png_encode(planes, 'grey', capacity=room, wait=False))

    def write(self, item, targets):
        tag, buf = item
        if not self.png_on_device:
            planes = buf.reshape((-1,) + buf.shape[-2:])

            def job():
                from PIL import Image
                for plane, (sub, name) in zip(planes, targets):
                    yield Image.fromarray(np.ascontiguousarray(plane)), sub, name
            self.saver.submit(job)
            return
        from .png import bytes_job, files_of_record
        (planes_dev,) = tag.dev

        def again(n, length):
            return ops.png_encode(planes_dev[n], 'grey', capacity=length)[0]
        files = files_of_record(buf, planes_dev.shape[0], tag.room[0], again, self.room.overflow)
        self.saver.submit(bytes_job([(data, sub, name) for data, (sub, name) in zip(files, targets)]))

    def close(self):
        if self.own_saver is not None:
            self.own_saver.close()                                   # re-raises a writer's error


class _MatteLoop(_PlaneChannel):
    """config['mattes'] inside a frame loop: one `ops.mask_mattes` launch sequence per frame on the compute stream, right behind the
    clean-up, on the index mask the loop hands on (cleaned, at the original resolution).  The planes - uint8 [T, K, H, W], one per table
    (matte, trimap) and label the mapper knows at that frame - become <masks_out_path>/mattes/<label>/<frame>.png and, with a trimap,
    <masks_out_path>/trimaps/<label>/<frame>.png, <label> the annotation's label as in tracks.json.  Masks, tracks and what goes back
    into the memory are not touched.  A frame without objects sends nothing."""
    every_frame = False

    def __init__(self, spec, saver, masks_out_path, vid_name='', png_on_device=False):
        from .matte import tables_of
        super().__init__(saver, masks_out_path, vid_name, png_on_device)
        self.names, self._tables, self.R = tables_of(spec)
        self.tables = None                                           # on the device, from the first frame on

    def submit(self, tag, mask_dev, mapper):
        k = len(mapper.labels)
        if k == 0:
            return []
        if self.tables is None:
            self.tables = torch.from_numpy(self._tables).to(mask_dev.device)
        return self.send(replace(tag, k=k), ops.mask_mattes(mask_dev, k, self.tables, self.R))

    def finish(self, item, mapper):
        from .rle import inverse_labels
        tag = item[0]
        self.write(item, [(os.path.join(sub, str(lab)), tag.frame[:-4] + '.png') for sub in self.names for lab in inverse_labels(mapper, tag.k)])


# ---- what a frame that has arrived becomes -------------------------------------------------------------------------------------------------

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
    """Everything a frame loop does with a frame's index mask once it is on the device: J&F scoring, the side channels in their order
    (tracks, mattes, PNGs), the copy to the host one frame behind, and - when a frame has arrived - its stats row and its saver job.
    The channels are fed before the mask: when a frame's mask has arrived, so have its records.  `submit` and `drain` enqueue and
    wait (the caller times them); `deliver` is the host side of whatever arrived.  Where no mask travels, a frame is delivered with
    the record of the first channel that has one for every frame.  `reused_output`: the caller rewrites `out_dev` next frame, so a
    channel that may read it again when its record arrives gets a copy.  `confidence` (config['confidence']: the loop's
    FrameConfidence): its planes are drained after the channels', its writers closed first, its scores go into the tracks file."""

    def __init__(self, reader, mapper, fetcher, saver=None, tracks=None, scorer=None, compute_iou=False, save_overlay=True,
                 masks_out_path=None, reused_output=False, mattes=None, pngs=None, confidence=None):
        self.reader, self.mapper, self.fetcher, self.saver, self.tracks, self.scorer = reader, mapper, fetcher, saver, tracks, scorer
        self.confidence, self.mattes = confidence, mattes
        self.pngs = pngs if saver is not None else None              # the files go to the loop's writers
        self.channels = [c for c in (tracks, mattes, self.pngs) if c is not None]
        self.compute_iou, self.save_overlay, self.masks_out_path, self.reused_output = compute_iou, save_overlay, masks_out_path, reused_output
        # the H x W mask itself travels only for who reads it on the host: the PNG writers and compute_iou
        self.need_mask = tracks is None or saver is not None or compute_iou
        if self.pngs is not None:                                    # the files come from the device: only the overlays and compute_iou read it
            self.need_mask = save_overlay or compute_iou
        self.stats = []
        self._arrived, self._done = [], ()

    def _keep(self, arrived, done):
        """what `deliver` finds: the channels' records, and the frames' masks - or, where no mask travels, the frames of the first
        channel that delivers every frame"""
        if done is None:
            done = [(tag, None) for tag, _ in next(items for ch, items in arrived if ch.every_frame)]
        self._arrived, self._done = arrived, done

    def submit(self, ti, sample, had_mask, out_dev):
        if self.scorer is not None and sample.mask is not None:
            self.scorer.add(ti, sample.mask, out_dev, self.mapper)
        tag = Tag(sample.frame, sample, had_mask)
        arrived = [(ch, ch.submit(tag, out_dev.clone() if self.reused_output and ch.rereads else out_dev, self.mapper)) for ch in self.channels]
        self._keep(arrived, self.fetcher.submit(tag, out_dev) if self.need_mask else None)

    def drain(self):
        arrived = [(ch, ch.drain()) for ch in self.channels]
        self._keep(arrived, self.fetcher.drain() if self.need_mask else None)
        if self.confidence is not None:
            self.confidence.drain()

    def deliver(self, last=False):
        arrived, done = self._arrived, self._done
        self._arrived, self._done = [], ()
        for ch, items in arrived:
            for item in items:
                ch.finish(item, self.mapper)
        for tag, out_mask in done:
            sample = tag.sample
            self.stats.append(_stats_row(sample.frame, tag.had_mask, self.compute_iou, out_mask, sample.mask))
            if self.pngs is not None:
                overlay = self.save_overlay and out_mask is not None
                self.saver.submit(_saver_job(self.reader, self.mapper.remap_index_mask(out_mask) if overlay else None, sample.frame,
                                             (lambda s=sample: s.raw_image_pil) if overlay else None, png=self.pngs.files.pop(sample.frame)))
            elif self.saver is not None:
                ids = self.mapper.remap_index_mask(out_mask)         # label LUT as of this frame (cheap); the rest is off-thread
                self.saver.submit(_saver_job(self.reader, ids, sample.frame,
                                             (lambda s=sample: s.raw_image_pil) if self.save_overlay else None))
        if last and self.tracks is not None:
            if self.confidence is not None:                          # the table's one transfer, after the loop
                self.tracks.writer.set_confidence(self.confidence.track_entries(self.mapper))
            self.tracks.write(self.masks_out_path)

    def close(self):
        """the confidence's writers, the channels', then the saver (which re-raises a writer's error); an error closes the rest all the same"""
        closers = ([self.confidence] if self.confidence is not None else []) + self.channels + ([self.saver] if self.saver is not None else [])
        with ExitStack() as stack:                                   # runs them last in, first out
            for c in reversed(closers):
                stack.callback(c.close)


# ---- the set-up and the report of both runners -----------------------------------------------------------------------------------------

def _option(config, key, module, parse):
    """config[key] as `module.parse` returns it; None without the key - nothing is imported for it then"""
    if config.get(key) is None:
        return None
    return getattr(import_module('.' + module, __package__), parse)(config[key])


@dataclass
class _LoopSide:
    """what `loop_outputs` made: `outputs` is what the loop drives, the rest is what its `frame` callback and `loop_report` read"""
    outputs: object
    mapper: object
    conf: object = None                                              # config['confidence']: the loop's FrameConfidence
    cleanup: dict = None                                             # config['mask_cleanup'], parsed
    cleaned: object = None                                           # its totals, on the device
    scorer: object = None                                            # compute_jf


def parse_outputs(config):
    """The output side's options, parsed - each opt-in, absent by default: 'mask_cleanup' (despeckle / fill holes / keep largest),
    'mattes' (feathered mattes / trimaps per label), 'png_on_device' (the PNG files are built on the device), 'temporal_smooth' (a
    majority vote over time), 'confidence' (per-object confidence, uncertainty maps).  Raises what the parsers raise: no device needed."""
    return dict(cleanup=parse_cleanup(config.get('mask_cleanup')), mattes=_option(config, 'mattes', 'matte', 'parse_mattes'),
                png=_option(config, 'png_on_device', 'png', 'parse_option'), smooth=_option(config, 'temporal_smooth', 'temporal', 'parse_smooth'),
                confidence=_option(config, 'confidence', 'confidence', 'parse_confidence'))


def loop_outputs(config, spec, reader, mapper, device, vid_length, reused_output=False, motion_frames=None, compute_iou=False,
                 save_overlay=True, compute_jf=False, max_queue=200):
    """The output side of a frame loop from the merged config and its `parse_outputs` - parsed apart, since a bad value is an error
    before the preload and this comes after it: the saver, the loop's FrameConfidence, the channels, `_FrameOutputs` and the delay line
    round it.  `motion_frames`: `sample -> its frame at the mask's size`, for the compensated vote.  Without an option's key nothing is
    imported, allocated or launched for it."""
    out_path, png_on_device = config['masks_out_path'], spec['png'] is not None
    scorer = None
    if compute_jf:
        from .metrics import InLoopScorer
        scorer = InLoopScorer(vid_length, device)
    saver = _AsyncSaver(out_path, reader.vid_name, max_queue) if config['save_masks'] else None
    conf = None
    if spec['confidence'] is not None:
        from .confidence import FrameConfidence
        conf = FrameConfidence(spec['confidence'], vid_length, device, saver, out_path, reader.vid_name, png_on_device)
    # Opt-in (config['save_tracks'] = True; default False): the device finds the run boundaries, the host receives those (rle.py).
    outputs = _FrameOutputs(
        reader, mapper, AsyncMaskFetcher(), saver=saver, scorer=scorer, compute_iou=compute_iou, save_overlay=save_overlay,
        masks_out_path=out_path, reused_output=reused_output, confidence=conf,
        tracks=_TrackLoop(config.get('tracks_counts', 'list'), config.get('tracks_polygons')) if config.get('save_tracks', False) else None,
        mattes=None if spec['mattes'] is None else _MatteLoop(spec['mattes'], saver, out_path, reader.vid_name, png_on_device),
        pngs=None if spec['png'] is None or saver is None else _PngLoop(spec['png'], reader))
    if spec['smooth'] is not None:
        # the vote comes after `_clean_output` and before everything `_FrameOutputs` does; the probabilities that go back into the
        # memory are not touched, so propagation is the same with and without the option
        from .temporal import DelayLine
        outputs = DelayLine(outputs, spec['smooth'], vid_length, device, frame_of=motion_frames)
    return _LoopSide(outputs, mapper, conf, spec['cleanup'], _cleanup_totals(spec['cleanup'], device), scorer)


def _with_jf(df, scorer):
    """compute_jf=True: the J and F columns (per-frame means over the sequence's ground-truth objects, NaN without a ground truth)."""
    if scorer is not None:
        df['J'], df['F'] = scorer.scores()
    return df


def _say(title, report):
    print(title + ': ' + ', '.join(f'{k.replace("_", " ")} {v}' for k, v in report.items()))


def loop_report(side, say=False):
    """The DataFrame a runner returns: the stats rows, J and F, and one transfer after the loop for each of df.attrs['cleanup'] (the
    video's totals of the four counters), df.attrs['temporal_smooth'] (the radius, the changed pixels and frames) and the frame
    confidence per row with the table in df.attrs['confidence']."""
    import pandas as pd
    df = _with_jf(pd.DataFrame(side.outputs.stats), side.scorer)
    if side.cleaned is not None:
        df.attrs['cleanup'] = _cleanup_report(side.cleaned)
        if say:
            _say('MASK CLEAN-UP', df.attrs['cleanup'])
    if hasattr(side.outputs, 'report'):
        df.attrs['temporal_smooth'] = side.outputs.report()
        if say:
            _say('TEMPORAL SMOOTHING', df.attrs['temporal_smooth'])
    if side.conf is not None:
        df['confidence'] = side.conf.frame_confidence()[:len(df)]
        df.attrs['confidence'] = side.conf.report(side.mapper)
    return df
