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

There is one frame loop, `_run_frame_loop`: `hinted` decides which frames are hinted when, and the whole output side (scorer, side
channels, mask copy one frame behind, stats rows, saver jobs, the returned DataFrame) is frame_outputs.py.  `run_on_video` and
`run_on_video_ensemble` are a preload and three callbacks each (hint / prepare / frame); `VideoSession` shares `hinted`.
"""
import collections
import os
from dataclasses import dataclass
from time import perf_counter
from typing import Iterable, Optional
from warnings import warn

import numpy as np
import torch

from . import ops
from .configuration import VIDEO_INFERENCE_CONFIG
# the output side; the names other code takes from this module stay importable from it
from .frame_outputs import (AsyncMaskFetcher, _AsyncSaver, _clean_output, _FrameOutputs, _TrackLoop,  # noqa: F401
                            loop_outputs, loop_report, parse_outputs)
from .inference_core import InferenceCore
from .mask_mapper import MaskMapper
from .network import XMem

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


def _post_process_gpu(sample, prob, confidence=None, ti=None, given=False):
    """run_on_video.py:165-170 on the device: resize to the original shape if needed, argmax over classes.  `confidence`
    (config['confidence']: a `confidence.FrameConfidence`): its kernel takes the place of the argmax, yields the same mask and keeps
    frame ti's record."""
    if sample.need_resize and tuple(prob.shape[-2:]) != tuple(sample.shape):
        prob = ops.resize_bilinear(prob, sample.shape)
    if confidence is not None:
        return confidence.mask(ti, prob, sample.frame, given)
    return ops.argmax_u8(prob)


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
    device = _inference_device()
    frames_with_masks = set(frames_with_masks)
    config = _merged_config({} if overwrite_config is None else overwrite_config, masks_out_path)   # the caller's dict receives the path
    out_spec = parse_outputs(config)
    mapper, processor, vid_reader = _load_main_objects(imgs_in_path, masks_in_path, config, device, network=network)
    vid_length = len(vid_reader)
    motion_frames = _motion_frames(out_spec['smooth'], vid_reader.resize_on_device, (lambda sample: sample.rgb_u8) if vid_reader.size < 0 else None)

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

    side = loop_outputs(config, out_spec, vid_reader, mapper, device, vid_length, motion_frames=motion_frames, compute_iou=compute_iou,
                        save_overlay=save_overlay, compute_jf=compute_jf, max_queue=image_saving_max_queue_size)
    conf = side.conf

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
        return msk is not None, _clean_output(side.cleanup, raw, side.cleaned)

    key_batch = max(1, int(config.get('key_batch', 4)))                # frames per batched key-encoder hint
    decoder = FramePrefetcher(vid_reader, depth=4 * key_batch, workers=int(config.get('decode_workers', 8)))
    total_time, loop_wall, total_wall = _run_frame_loop(vid_length, key_batch, decoder, side.outputs, hint, prepare, frame)
    if print_fps:
        print(f'TOTAL PRELOADING TIME: {preload_time:.4f}s')
        print(f'TOTAL PROCESSING TIME: {total_time:.4f}s')
        print(f'TOTAL PROCESSING FPS: {vid_length / total_time:.4f}')
        print(f'TOTAL FPS (excluding image saving): {vid_length / (preload_time + total_time):.4f}')
        print(f'WALL-CLOCK FPS of the frame loop incl. decode: {vid_length / loop_wall:.4f}; incl. writing every mask: '
              f'{vid_length / total_wall:.4f}')
    return loop_report(side, say=print_fps)


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
    config = _merged_config(dict(overwrite_config or {}), masks_out_path)           # on a copy: the caller's dict stays as it is
    passes = parse_ensemble(config.get('ensemble'), config['size'])
    out_spec = parse_outputs(config)
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
    motion_frames = _motion_frames(out_spec['smooth'], dev_resize, _pass_frame(_source_pass(passes)))
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
    # on the merged mask, a buffer the next frame writes again - unless cleaned
    side = loop_outputs(config, out_spec, vid_reader, mapper, device, vid_length, reused_output=out_spec['cleanup'] is None,
                        motion_frames=motion_frames, compute_iou=compute_iou, save_overlay=save_overlay, compute_jf=compute_jf,
                        max_queue=image_saving_max_queue_size)
    conf = side.conf
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
        return given, _clean_output(side.cleanup, merged, side.cleaned)       # cleaned: into a tensor of its own, `merged` is rewritten next frame

    key_batch = max(1, int(config.get('key_batch', 4)))
    decoder = EnsembleFramePrefetcher(readers, passes, depth=4 * key_batch, workers=int(config.get('decode_workers', 8)))
    total_time, loop_wall, total_wall = _run_frame_loop(vid_length, key_batch, decoder, side.outputs, hint, prepare, frame)
    if print_fps:
        print(f'ENSEMBLE PASSES: {P} (' + ', '.join(str(s) + (' flip' if f else '') for s, f in passes) + ')')
        print(f'TOTAL PRELOADING TIME: {preload_time:.4f}s')
        print(f'TOTAL PROCESSING TIME: {total_time:.4f}s')
        print(f'TOTAL PROCESSING FPS: {vid_length / total_time:.4f} (ensemble of {P} passes; {P * vid_length / total_time:.4f} passes/s)')
        print(f'WALL-CLOCK FPS of the frame loop incl. decode: {vid_length / loop_wall:.4f}; incl. writing every mask: '
              f'{vid_length / total_wall:.4f}')
    return loop_report(side, say=print_fps)


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
