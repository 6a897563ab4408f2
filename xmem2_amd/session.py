"""VideoSession: the annotate -> propagate -> select loop of XMem++ on one video, with everything that does not change between
iterations kept on the device.

The reference's interactive backend (inference/interact/gui.py:719-884 with resource_manager.py) is a tensor program behind a GUI:
it stores each propagated frame's key, shrinkage, selection and mask, hands exactly those to `select_next_candidates`, edits the
permanent memory in place when a reference is saved or removed and propagates forward or backward from any frame.  This module is
that program without the GUI, on the file conventions of `run_on_video`:

    s = VideoSession(imgs_in_path, masks_in_path, overwrite_config={...}, network=net)
    s.save_reference(0)                     # the annotation of frame 0 from masks_in_path
    s.full_propagation()                    # == run_on_video(frames_with_masks=s.references), masks stay on the device
    new = s.candidates(k=3)                 # no second encoder pass, no mask file read back
    s.save_reference(new[0], mask)          # an index array, a device tensor (S2M / click output) or a palette PNG
    s.full_propagation(); s.save(out_dir)

Paid once per video: decode, resize and upload of every frame (working-size uint8, on the device up to
`config['session_device_frame_bytes']`, in pinned host memory beyond it).  Paid once per network: upload, filter transforms and the
captured stages.  Recomputed per propagation: the key encoder, readout and decoder of every visited frame.  Never recomputed: keys
for the selector - every visited frame's key, shrinkage and selection come from its own `step` (the copies
`return_key_and_stuff=True` makes of the buffers the step used, taken before the step releases them to the next key pass) and are
stored in a per-video arena.

Opt-in, `config['session_feature_cache_bytes']` > 0 (`FeatureCache`): the key encoder is paid once per frame too.  Everything the
decoder and the value encoder take from a hinted key pass depends on the frame alone - key, shrinkage, selection, f16, the decoder's
two skip convolutions and the fuser's f16 half - and is saved per frame in one device arena; a later propagation restores a batch
with one copy launch per frame on the side stream instead of running the encoder (`InferenceCore.prefetch_cached`).  Bit-identical
to the cache being off; profiles/r07_session_cache.txt has the measurement.
"""
import argparse
import contextlib
import json
import os
import sys
from warnings import warn

import numpy as np
import torch

from . import ops
from .configuration import VIDEO_INFERENCE_CONFIG
from .inference_core import InferenceCore
from .mask_mapper import MaskMapper
from .run_on_video import hinted                 # the hint-ahead rule of every frame loop (re-exported: callers import it from here too)

DEFAULT_DEVICE_FRAME_BYTES = 16 << 30          # config['session_device_frame_bytes']: frames beyond it stay in pinned host memory
MASK_FORMS = ('objects', 'files')
ENTRY_ALIGN = 256                              # every tensor of a cache entry starts on a multiple of it: whole 16-byte chunks both ways


# ---- pure helpers (host) ---------------------------------------------------------------------------------------------
def visit_order(n_frames, start=0, direction='forward', stop=None):
    """Frame indices `propagate` visits: start, start +- 1, ..., stop (both included).  `stop` defaults to the end of the clip in the
    direction of travel."""
    if direction not in ('forward', 'backward'):
        raise ValueError(f"direction must be 'forward' or 'backward', got {direction!r}")
    if n_frames <= 0:
        raise ValueError('the video has no frames')
    step = 1 if direction == 'forward' else -1
    if stop is None:
        stop = n_frames - 1 if step > 0 else 0
    for name, v in (('start', start), ('stop', stop)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not (0 <= v < n_frames):
            raise ValueError(f'{name} = {v!r} is not a frame of this video (0..{n_frames - 1})')
    if (stop - start) * step < 0:
        raise ValueError(f'stop = {stop} lies behind start = {start} when going {direction}')
    return list(range(int(start), int(stop) + step, step))


def files_table(pic):
    """float32[256]: the mask value `_pil_to_tensor01` gives each pixel of `pic`, a PIL image of 256 pixels (pixel v stands for label
    v, any mode the harness reads), with the selector's max over channels folded in.  Computed by that function itself, so the
    arithmetic - float32(v) / 255 in IEEE division, a palette image contributing its raw INDEX plane - is the file path's."""
    from .run_on_video import _pil_to_tensor01
    t = _pil_to_tensor01(pic)
    if t.numel() != 256 * t.shape[0]:
        raise ValueError('files_table: expected an image of 256 pixels, one per label')
    return t.reshape(t.shape[0], 256).max(dim=0).values.contiguous()


def objects_table():
    """float32[256] of the GUI's meaning of a mask: any object -> 1.0, background -> 0.0."""
    t = torch.ones(256, dtype=torch.float32)
    t[0] = 0.0
    return t


def _remove_permanent_frame(core, t, pos):
    """Take the elements of frame t, the pos-th frame of the permanent store, out of it.  Not through
    `InferenceCore.remove_from_permanent_memory`, which keeps two quirks of the reference: the frame position `add` reports
    (kv_memory_store.py: (n_total + 1e-9) // (n + 1e-9) - 1) is one too small for every frame but the first (96.000000001 //
    48.000000001 is 1), and memory_manager.py:204-210 passes that POSITION as an ELEMENT offset.  The session knows the true position
    (its store is in frame order) and removes the frame's own h*w elements."""
    core._retire_early()
    mem = core.memory
    mem.frame_id_to_permanent_mem_idx.pop(t, None)
    mem.version += 1
    mem.permanent_work_mem.remove_at(pos * mem.HW, mem.HW)


class FeatureCache:
    """Per-frame outputs of the hinted key pass in one device arena (see the module docstring), and the policy of using them.

    * The entry layout - (shape, dtype) of one frame's key, shrinkage, selection, f16 and extras - is that of the first key pass after
      construction, so it follows the network's precision mode; the arena, min(budget, n_frames * entry_bytes) bytes, is allocated then.
    * Frames get an entry in the order they are first visited until the arena is full.  Nothing is ever evicted.
    * An entry is TAGGED with the batch size of the key pass that filled it.  `lookup(batch)` serves a batch only when every frame of it
      has an entry tagged len(batch); otherwise the batch runs the key pass, which overwrites and re-tags the entries of its frames
      (`claim`).  The tag is what keeps "cache on" equal to "cache off" byte for byte: convolution plans are chosen per batch size, so
      a frame encoded alone need not have the bits of the same frame encoded in a batch of four."""

    def __init__(self, n_frames, budget_bytes, device):
        self.n_frames, self.budget, self.device = int(n_frames), int(budget_bytes), device
        self.layout = None
        self.entry_bytes = 0
        self.arena = None
        self._slot = {}                        # frame -> index of its entry in the arena
        self._tag = {}                         # frame -> batch size of the pass that filled the entry
        self.capacity = 0
        self.hits = self.misses = 0

    def _entry(self, slot):
        base, views = slot * self.entry_bytes, []
        for shape, dtype in self.layout:
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            views.append(self.arena[base:base + nbytes].view(dtype).view(shape))
            base += -(-nbytes // ENTRY_ALIGN) * ENTRY_ALIGN
        return tuple(views)

    def lookup(self, batch):
        """The entries of `batch` (frame indices) when all of them were filled by a pass of len(batch) frames, else None; counted."""
        if all(self._tag.get(t) == len(batch) for t in batch):
            self.hits += len(batch)
            return [self._entry(self._slot[t]) for t in batch]
        self.misses += len(batch)
        return None

    def claim(self, batch, layout):
        """Called by the key pass of `batch` with its entry layout: the entry (or None: the arena is full) each frame is to be saved
        to, now tagged len(batch)."""
        layout = tuple((tuple(int(v) for v in shape), dtype) for shape, dtype in layout)
        if self.layout is None:
            self.layout = layout
            self.entry_bytes = sum(-(-int(np.prod(sh)) * torch.empty((), dtype=dt).element_size() // ENTRY_ALIGN) * ENTRY_ALIGN
                                   for sh, dt in layout)
            self.capacity = min(self.n_frames, self.budget // self.entry_bytes)
            self.arena = torch.empty(self.capacity * self.entry_bytes, dtype=torch.uint8, device=self.device)
        elif layout != self.layout:
            raise RuntimeError('FeatureCache: the key pass changed its output layout (one cache serves one geometry and precision)')
        out = []
        for t in batch:
            if t not in self._slot and len(self._slot) < self.capacity:
                self._slot[t] = len(self._slot)
            if t in self._slot:
                self._tag[t] = len(batch)
                out.append(self._entry(self._slot[t]))
            else:
                out.append(None)
        return out

    def info(self):
        return dict(entry_bytes=self.entry_bytes, frames=len(self._slot), bytes=self.arena.numel() if self.arena is not None else 0,
                    hits=self.hits, misses=self.misses)


class _Frame:
    """What `_post_process_gpu` and the writers need of a decoded frame (the fields of run_on_video.Sample they read)."""
    __slots__ = ('frame', 'shape', 'need_resize', 'raw_image_pil', 'mask')

    def __init__(self, smp):
        # the decoded original-size image is NOT kept (several GB for a long 1080p clip): only overlays need it, `save` reads it again
        self.frame, self.shape, self.need_resize, self.raw_image_pil, self.mask = smp.frame, smp.shape, smp.need_resize, None, smp.mask


class VideoSession:
    def __init__(self, imgs_in_path, masks_in_path=None, overwrite_config=None, network=None):
        from .frame_outputs import _cleanup_totals
        from .run_on_video import _make_network, _set_long_term_count_usage, _working_u8
        if not os.path.isdir(imgs_in_path):
            raise NotADirectoryError(f'imgs_in_path: {imgs_in_path!r} is not a directory of frames')
        if masks_in_path is not None and not os.path.isdir(masks_in_path) and not os.path.isfile(masks_in_path):
            raise NotADirectoryError(f'masks_in_path: {masks_in_path!r} is not a directory')      # a file: tracks (xmem2_amd/rle.py)
        if overwrite_config is not None and not isinstance(overwrite_config, dict):
            raise TypeError('overwrite_config must be a dict (or None)')
        if not torch.cuda.is_available():
            raise RuntimeError('xmem2_amd.session needs an MI355X (HIP) device - there is no CPU path')
        torch.autograd.set_grad_enabled(False)
        self.device = torch.device('cuda', torch.cuda.current_device())
        config = VIDEO_INFERENCE_CONFIG.copy()
        config.update(overwrite_config or {})
        self.config = config
        from .mask_cleanup import parse_cleanup
        self.cleanup = parse_cleanup(config.get('mask_cleanup'))         # opt-in: every propagated mask is cleaned before it is kept
        self.network = _make_network(config, self.device, network)
        self.imgs_in_path, self.masks_in_path = imgs_in_path, masks_in_path
        reader = _session_reader(imgs_in_path, masks_in_path, size=config['size'], resize_on_device=config.get('resize_on_device', False))
        self.reader = reader
        n = len(reader)
        if n == 0:
            raise ValueError(f'no frames in {imgs_in_path!r}')
        _set_long_term_count_usage(config, n)
        self.mapper = MaskMapper()
        self.core = InferenceCore(self.network, config=config)
        self.key_batch = max(1, int(config.get('key_batch', 4)))

        # every frame decoded ONCE: working-size uint8, on the device up to the byte cap, in pinned host memory beyond it
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=max(1, int(config.get('decode_workers', 8))), thread_name_prefix='xmem-decode') as pool:
            samples = list(pool.map(reader.__getitem__, range(n)))
        self.frames = [_Frame(s) for s in samples]
        if any(s.shape != samples[0].shape for s in samples):
            raise ValueError('the frames of a video must have one size')
        self.shape = samples[0].shape                                    # (H, W) of the original frames and of the masks
        dev_resize = samples[0].rgb_u8 is None
        th, tw = samples[0].target_hw if dev_resize else samples[0].rgb_u8.shape[:2]
        cap = int(config.get('session_device_frame_bytes', DEFAULT_DEVICE_FRAME_BYTES))
        per_frame = th * tw * 3
        self.n_device_frames = n if cap < 0 else min(n, cap // per_frame)
        self._dev_frames = torch.empty((self.n_device_frames, th, tw, 3), dtype=torch.uint8, device=self.device)
        self._host_frames = torch.empty((n - self.n_device_frames, th, tw, 3), dtype=torch.uint8, pin_memory=True) \
            if n > self.n_device_frames else None
        for i, s in enumerate(samples):
            if i < self.n_device_frames:
                self._dev_frames[i].copy_(_working_u8(s.src_u8, s.target_hw, self.device) if dev_resize else s.rgb_u8)
            elif dev_resize:
                from .pil_resize import resize_u8_host                   # the host restatement of the device resize: the same bytes
                self._host_frames[i - self.n_device_frames].copy_(torch.from_numpy(resize_u8_host(s.src_u8.numpy(), th, tw)))
            else:
                self._host_frames[i - self.n_device_frames].copy_(s.rgb_u8)
        del samples

        # arenas: one row block per frame, written by the propagation that visits the frame
        gh, gw = -(-th // 16), -(-tw // 16)                              # the stride-16 grid of the padded frame
        ck = self.network.key_dim
        self.grid_hw = (gh, gw)
        self.key = torch.empty((n, gh * gw, ck), dtype=torch.float32, device=self.device)
        self.shrinkage = torch.empty((n, gh * gw), dtype=torch.float32, device=self.device)
        self.selection = torch.empty((n, gh * gw, ck), dtype=torch.float32, device=self.device)
        self.masks = torch.zeros((n,) + tuple(self.shape), dtype=torch.uint8, device=self.device)   # dense ids (MaskMapper)
        self._present = [False] * n
        self._cleaned = _cleanup_totals(self.cleanup, self.device)      # the four counters of the clean-up, summed on the device
        self._refs = {}                                                  # frame index -> the annotation's raw H x W index array
        budget = int(config.get('session_feature_cache_bytes', 0))      # opt-in: the key pass of every frame kept on the device
        self._fcache = FeatureCache(n, budget, self.device) if budget > 0 else None
        self._confidence = None                                          # opt-in (config['confidence']): a record per propagated frame
        if config.get('confidence') is not None:
            from .confidence import FrameConfidence, parse_confidence
            spec = parse_confidence(config['confidence'])
            planes = torch.zeros((n,) + tuple(self.shape), dtype=torch.uint8, device=self.device) if spec['maps'] else None
            self._confidence = FrameConfidence(spec, n, self.device, planes=planes)     # 'maps': the planes stay here until `save`
        torch.cuda.synchronize()                                         # the frames are complete for every stream from here on

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self.frames)

    @property
    def references(self):
        """Sorted frame indices in the permanent memory."""
        return sorted(self._refs)

    def _check_frame(self, t):
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not (0 <= t < len(self)):
            raise IndexError(f'frame {t!r} is not a frame of this video (0..{len(self) - 1})')
        return int(t)

    def frame_u8(self, t):
        """The working-size uint8 frame t as `step` / `prefetch_keys` take it (a device tensor, or pinned host memory beyond the cap)."""
        t = self._check_frame(t)
        return self._dev_frames[t] if t < self.n_device_frames else self._host_frames[t - self.n_device_frames]

    def all_masks_present(self):
        return all(self._present)

    def cache_info(self):
        """dict(entry_bytes, frames, bytes, hits, misses) of the feature cache (`config['session_feature_cache_bytes']`): bytes of one
        entry and of the arena, frames that own an entry, and frames served from it / sent to the key pass so far.  All zero while the
        cache is off or no key pass has run."""
        fc = getattr(self, '_fcache', None)
        return fc.info() if fc is not None else dict(entry_bytes=0, frames=0, bytes=0, hits=0, misses=0)

    def _label_lut(self):
        """dense id -> original label value, as a host uint8[256] (identity while the annotation's ids are 1, 2, 3, ...)."""
        lut = np.arange(256, dtype=np.uint8)
        if not self.mapper.coherent:
            lut[:] = 0
            for original, dense in self.mapper.remappings.items():
                lut[dense] = original
        return lut

    def mask(self, t):
        """Device uint8 [H, W] with the original label values, or None when no propagation has visited frame t."""
        t = self._check_frame(t)
        if not self._present[t]:
            return None
        if self.mapper.coherent:
            return self.masks[t].clone()                                  # a copy: the arena is the session's state
        key = tuple(sorted(self.mapper.remappings.items()))
        if getattr(self, '_lut_dev', (None, None))[0] != key:            # changes only when an annotation brings a new label
            self._lut_dev = (key, torch.from_numpy(self._label_lut()).to(self.device))
        return self._lut_dev[1][self.masks[t].long()]

    # ---- references ----------------------------------------------------------------------------------------------------
    def _raw_mask(self, t, mask):
        """The annotation as the reader would have read it: an H x W uint8 index array at the original size."""
        from PIL import Image
        if mask is None:
            raw = self.frames[t].mask
            if raw is None:
                raise FileNotFoundError(f"Couldn't find mask {t}! Check that the filename is the same as for frame {t}.")
        elif isinstance(mask, (str, os.PathLike)):
            raw = np.array(Image.open(mask).convert('P'), dtype=np.uint8)
        elif torch.is_tensor(mask):
            m = mask
            if m.dim() == 3:                                             # [K+1, H, W] probabilities (aggregate_wbg output)
                m = ops.argmax_u8(m.to(self.device, torch.float32).contiguous()) if m.shape[0] > 1 else m[0]
            raw = m.to(torch.uint8).cpu().numpy()
        else:
            raw = np.asarray(mask).astype(np.uint8)
        if raw.ndim != 2 or tuple(raw.shape) != tuple(self.shape):
            raise ValueError(f'mask of frame {t}: expected an index mask of shape {tuple(self.shape)}, got {tuple(raw.shape)}')
        return np.ascontiguousarray(raw)

    def _put(self, t, raw):
        msk, _ = self.mapper.convert_mask(raw, exhaustive=True)
        if min(msk.shape) == 0:
            return None
        if self.frames[t].need_resize:
            msk = self.reader.resize_mask(msk)
        self.core.set_all_labels(list(self.mapper.remappings.values()))
        rgb = self.frame_u8(t)
        return self.core.put_to_permanent_memory(rgb.to(self.device), msk.to(self.device), t)

    def save_reference(self, t, mask=None):
        """gui.on_save_reference: put_to_permanent_memory(image, mask, t).  True if frame t was a reference already (its entry is
        replaced).  `mask`: None (the file of frame t in masks_in_path) | H x W index array | device tensor (an index mask,
        or [K+1, H, W] probabilities) | path to a palette PNG.
        The permanent memory is kept in frame order - a reference in front of existing ones makes those be put again behind it - so
        that the memory, and with it every result, is a function of the SET of references: what run_on_video builds for that set."""
        t = self._check_frame(t)
        raw = self._raw_mask(t, mask)
        if not self.mapper.labels and not raw.any():                     # no object known, none given (run_on_video.py:213-216)
            warn(f'Skipping adding frame {t} to permanent memory, as the mask is empty')
            return False
        # frame t itself (when it is replaced) and the references behind it are taken out and put again in frame order.  A replacement
        # does not go through update_permanent_memory: the position it would write to is the reference's, one frame too early.
        replaced = t in self._refs
        again = [r for r in self.references if r > t or r == t]
        if again:
            self._require_one_object_group('save_reference of a frame that is, or lies in front of, an existing reference')
        for r in reversed(again):
            _remove_permanent_frame(self.core, r, self.references.index(r))
        self._put(t, raw)
        self._refs[t] = raw
        for r in again:
            if r != t:
                self._put(r, self._refs[r])
        self._sync_positions()
        return replaced

    def remove_reference(self, t):
        """gui.on_remove_reference.  The labels the mask mapper has seen stay known."""
        t = self._check_frame(t)
        if t not in self._refs:
            raise KeyError(f'frame {t} is not a reference (references: {self.references})')
        self._require_one_object_group('remove_reference')
        _remove_permanent_frame(self.core, t, self.references.index(t))
        del self._refs[t]
        self._sync_positions()

    def _require_one_object_group(self, what):
        """Taking a frame out of the permanent store is defined for ONE object group only.  An object that first appears in a later
        reference opens a second group whose value arena starts at that frame and is shorter than the key arena; the store sieves
        every arena by the same element range, which would hit the wrong elements there (as for eviction, kv_memory_store.py:160-181,
        the store does not support it).  Nothing has been changed when this raises."""
        perm = getattr(self.core.memory, 'permanent_work_mem', None)
        if perm is not None and perm.num_groups > 1:
            raise NotImplementedError(f'{what}: the permanent memory holds {perm.num_groups} object groups (an object first appeared '
                                      'in a later reference); frames can only be appended to it - start a new VideoSession to '
                                      'annotate this set of references')

    def _sync_positions(self):
        """The memory's frame -> position table restated with the true positions (the store is in frame order)."""
        table = getattr(self.core.memory, 'frame_id_to_permanent_mem_idx', None)
        if table is not None:
            table.clear()
            table.update({r: i for i, r in enumerate(self.references)})

    # ---- propagation ---------------------------------------------------------------------------------------------------
    def propagate(self, start=0, direction='forward', stop=None, manually_curated_masks=False):
        """gui.on_propagation: step over start..stop in `direction` on the memory as it stands; per visited frame the call
        run_on_video's frame loop makes.  Returns the visited frame indices."""
        from .frame_outputs import _clean_output
        from .run_on_video import _post_process_gpu
        order = visit_order(len(self), start, direction, stop)
        if not self._refs:
            raise ValueError('No valid masks provided!')
        core, device = self.core, self.device
        on_device = all(t < self.n_device_frames for t in order)

        fcache = getattr(self, '_fcache', None)
        cleanup, cleaned = getattr(self, 'cleanup', None), getattr(self, '_cleaned', None)
        conf = getattr(self, '_confidence', None)

        def prefetch(batch):
            # resident frames were complete long ago (synchronised at construction): the pass may start under the current frame
            frames = [self.frame_u8(t) for t in batch]
            if fcache is None:
                return core.prefetch_keys(frames, inputs_complete=on_device)
            entries = fcache.lookup(batch)
            if entries is not None:                                      # every frame saved by a pass of this batch size: no key stage
                return core.prefetch_cached(frames, entries, inputs_complete=on_device)
            return core.prefetch_keys(frames, inputs_complete=on_device, save_to=lambda layout: fcache.claim(batch, layout))

        for i, (t, rgb) in enumerate(hinted(order, self.key_batch, prefetch)):
            fr = self.frames[t]
            msk = labels = None
            if t in self._refs:
                msk, labels = self.mapper.convert_mask(self._refs[t], exhaustive=True)
                if fr.need_resize:
                    msk = self.reader.resize_mask(msk)
                msk = msk.to(device)
                core.set_all_labels(list(self.mapper.remappings.values()))
            prob, key, shr, sel = core.step(rgb, msk, labels, end=(i == len(order) - 1), manually_curated_masks=manually_curated_masks,
                                            do_not_add_mask_to_memory=(msk is not None), return_key_and_stuff=True)
            gh, gw = self.grid_hw
            self.key[t].view(gh, gw, -1).copy_(key[0].permute(1, 2, 0))
            self.shrinkage[t].view(gh, gw).copy_(shr[0, 0])
            self.selection[t].view(gh, gw, -1).copy_(sel[0].permute(1, 2, 0))
            raw = _post_process_gpu(fr, prob) if conf is None else _post_process_gpu(fr, prob, conf, t, msk is not None)
            self.masks[t].copy_(_clean_output(cleanup, raw, cleaned))
            self._present[t] = True
        return order

    def full_propagation(self):
        """gui.on_full_propagation: clear_memory(keep_permanent=True), then forward from frame 0."""
        if not self._refs:
            raise ValueError('No valid masks provided!')
        self.core.clear_memory(keep_permanent=True)
        return self.propagate(0, 'forward')

    def clean(self, min_area=0, max_hole=0, keep_largest=False, batch=32):
        """`ops.clean_masks` on the masks as they stand, `batch` frames per call, in place of what they held; a frame without a mask
        is all zero and stays so.  Returns the totals {components_removed, pixels_removed, holes_filled, pixels_filled}."""
        from .mask_cleanup import parse_cleanup
        from .frame_outputs import _cleanup_report
        spec = parse_cleanup({'min_area': min_area, 'max_hole': max_hole, 'keep_largest': keep_largest})
        totals = torch.zeros(4, dtype=torch.int64, device=self.device)
        step = max(1, int(batch))
        with torch.cuda.device(self.device):
            for i in range(0, len(self) if spec is not None else 0, step):
                out, stats = ops.clean_masks(self.masks[i:i + step], **spec)
                self.masks[i:i + step].copy_(out)
                totals.add_(stats.sum(0))
        return _cleanup_report(totals)

    def grow(self, r, batch=32):
        """`ops.grow_masks` on the masks as they stand, `batch` frames per call, in place of what they held: r > 0 grows every object
        by r pixels into the background (objects never eat one another, ties go to the smaller dense id), r < 0 shrinks it; |r| in
        1..127.  A frame without a mask is all zero and stays so."""
        step = max(1, int(batch))
        with torch.cuda.device(self.device):
            for i in range(0, len(self), step):
                self.masks[i:i + step].copy_(ops.grow_masks(self.masks[i:i + step], r))

    def smooth(self, radius, batch=32, motion=None):
        """`ops.temporal_mode` on the masks as they stand, in place of what they held: every frame becomes the majority vote over the
        frames within `radius` of it (1..7; `temporal.mode_host` has the definition).  The references vote but stay as they are, a
        frame without a mask neither votes nor changes.  The vote runs `batch` frames per launch and every batch reads unsmoothed
        frames: a batch is written back only when no later one reads it, so the result does not depend on `batch`.  Returns the
        number of pixels changed per frame.  The session does not read config['temporal_smooth'] - `propagate` visits frames in
        either direction and in parts, so there is no one delay line to hold: this method is its surface.
        `motion` (True, or {'search', 'bias', 'max_sad'}: `motion.parse_motion`): the motion-compensated vote,
        `temporal.mode_mc_host` of the masks and the lumas of the resident frames (`ops.temporal_mode_mc_ring`), for which the
        working size must be the masks' size - ValueError otherwise."""
        from .temporal import frame_flags
        T, step = len(self), max(1, int(batch))
        vote = lambda i, n, **kw: ops.temporal_mode_ring(self.masks, T, i, n, radius, flags, **kw)
        if motion is not None:
            from .motion import parse_motion
            spec = parse_motion(motion, 'VideoSession.smooth: motion')
            if tuple(self.frame_u8(0).shape[:2]) != tuple(self.shape):
                raise ValueError(f'VideoSession.smooth: motion needs frames of the masks\' size; the session works at '
                                 f'{tuple(self.frame_u8(0).shape[:2])}, the masks are {tuple(self.shape)}')
            lumas = torch.empty_like(self.masks)
            with torch.cuda.device(self.device):
                for t in range(T):
                    ops.luma_u8(self.frame_u8(t).to(self.device, non_blocking=True), out=lumas[t])
            vote = lambda i, n, **kw: ops.temporal_mode_mc_ring(self.masks, lumas, T, i, n, radius, flags, **spec, **kw)
        locked = [t in set(self.references) for t in range(T)]
        flags = torch.from_numpy(frame_flags(T, self._present, locked)).to(self.device)
        changed = torch.empty(T, dtype=torch.int32, device=self.device)
        waiting = []                                                     # (first frame, smoothed batch) a later batch still reads under
        with torch.cuda.device(self.device):
            for i in range(0, T, step):
                n = min(step, T - i)
                out, _ = vote(i, n, changed=changed[i:i + n])
                waiting.append((i, out))
                while waiting and waiting[0][0] + waiting[0][1].shape[0] <= i + n - radius:
                    at, done = waiting.pop(0)
                    self.masks[at:at + done.shape[0]].copy_(done)
            for at, done in waiting:
                self.masks[at:at + done.shape[0]].copy_(done)
        return [int(v) for v in changed.cpu().tolist()]

    # ---- confidence ----------------------------------------------------------------------------------------------------
    def _require_confidence(self, what):
        conf = getattr(self, '_confidence', None)
        if conf is None:
            raise RuntimeError(f"{what} needs overwrite_config={{'confidence': ...}} (xmem2_amd/confidence.py)")
        return conf

    def confidence(self):
        """The records of the frames propagated so far (config['confidence']), one row per frame in frame order: {'threshold',
        'labels' (0, the background, then the annotation's labels), 'frames' (their indices), 'confidence' (float64, the frame
        confidence), 'area', 'margin_sum', 'low', 'contested' (int64 [rows, len(labels)])}.  A later visit of a frame overwrites its
        row.  One transfer of the device table."""
        conf = self._require_confidence('confidence()')
        rows = [t for t, v in enumerate(conf.visited) if v]
        out = conf.report(self.mapper)
        for name in out:
            if name not in ('threshold', 'labels'):
                out[name] = out[name][rows]
        out['frames'], out['confidence'] = rows, conf.frame_confidence()[rows]
        return out

    def review_queue(self, k=5, min_gap=0):
        """The `k` frames whose least sure object is the least sure (`confidence.review_queue` on the table): references and frames
        without a record are never proposed, NaN sorts last, ties go to the lower index, a frame within `min_gap` of one already
        chosen is passed over."""
        from .confidence import review_queue
        conf = self._require_confidence('review_queue()')
        skip = set(self._refs) | {t for t, v in enumerate(conf.visited) if not v} | {t for t, p in enumerate(self._present) if not p}
        return review_queue(conf.frame_confidence(), skip, k, min_gap)

    # ---- candidates ----------------------------------------------------------------------------------------------------
    def mask_table(self, mask_form='objects'):
        """float32[256] on the host: the selector's mask value of a DENSE id.  'objects': any object 1.0 (the GUI's masks);
        'files': what reading the PNG `save` writes back through `_pil_to_tensor01` gives (max over channels)."""
        if mask_form not in MASK_FORMS:
            raise ValueError(f'mask_form must be one of {MASK_FORMS}, got {mask_form!r}')
        if mask_form == 'objects':
            return objects_table()
        from PIL import Image
        labels = Image.fromarray(np.arange(256, dtype=np.uint8)[None])          # pixel v = original label v, as `save` hands it over
        by_label = files_table(self.reader.map_the_colors_back(labels))
        return by_label[torch.from_numpy(self._label_lut()).long()].contiguous()

    def candidates(self, k=5, alpha=0.5, min_mask_presence_percent=0.25, mask_form='objects', epsilon=0.5):
        """gui.on_compute_candidates: `select_next_candidates` on what the propagation left on the device, with `references` as the
        previously chosen frames.  Every frame must have a mask (gui.confirm_ready_for_candidates_selection)."""
        from .frame_selection import SelectorState, greedy_selection
        if not self.all_masks_present():
            missing = [t for t, p in enumerate(self._present) if not p]
            raise RuntimeError(f'Run propagation on all frames first! ({len(missing)} frame(s) without a mask, first: {missing[0]})')
        if not self._refs:
            raise RuntimeError('candidates need at least one reference')
        if k <= 0 or not (0.0 <= alpha <= 1.0) or min_mask_presence_percent < 0:
            raise ValueError('candidates: k > 0, 0 <= alpha <= 1 and min_mask_presence_percent >= 0 are required')
        if len(self._refs) >= len(self):
            raise ValueError('every frame is a reference already')
        lut = self.mask_table(mask_form).to(self.device)
        with torch.cuda.device(self.device):
            state = SelectorState.from_label_planes(self.key, self.shrinkage, self.selection, self.grid_hw, self.masks, lut, alpha, epsilon)
            return greedy_selection(state, k, self.references, min_mask_presence_percent, self.device)

    # ---- output --------------------------------------------------------------------------------------------------------
    def _host_masks(self):
        return self.masks.cpu().numpy()

    def save(self, masks_out_path, save_overlay=True, png_on_device=None, batch=32):
        """Exactly the files run_on_video writes: <out>/masks/<frame>.png (+ overlay/<frame>.jpg) for every frame that has a mask.
        `png_on_device` (config['png_on_device']: None, True or {'mode': 'rgb' | 'palette'}): the PNGs are built on the device from the
        resident `masks` in calls of `batch` frames (`ops.png_encode`) and their bytes reach the host; the masks travel only for the
        overlays."""
        from PIL import Image
        from .frame_outputs import _AsyncSaver, _saver_job
        spec = None
        if png_on_device is not None:
            from .png import mask_tables, parse_option
            spec = parse_option(png_on_device)
        host = self._host_masks() if spec is None or save_overlay else None
        files = {}
        if spec is not None:
            table, palette = (None if t is None else torch.from_numpy(t).to(self.device) for t in mask_tables(self.reader, self.mapper, spec['mode']))
            present = [t for t, p in enumerate(self._present) if p]
            with torch.cuda.device(self.device):
                for i in range(0, len(present), max(1, int(batch))):
                    chunk = present[i:i + max(1, int(batch))]
                    contiguous = chunk == list(range(chunk[0], chunk[-1] + 1))
                    dev = self.masks[chunk[0]:chunk[-1] + 1] if contiguous else self.masks[torch.tensor(chunk, device=self.device)]
                    files.update(zip(chunk, ops.png_encode(dev, spec['mode'], table, palette)))
        saver = _AsyncSaver(str(masks_out_path), '')
        try:
            for t, fr in enumerate(self.frames):
                if not self._present[t]:
                    continue
                def reopen(name=fr.frame):                               # the decoded frames were not kept: on the writer thread
                    return Image.open(os.path.join(self.reader.image_dir, name)).convert('RGB')
                saver.submit(_saver_job(self.reader, self.mapper.remap_index_mask(host[t]) if host is not None else None, fr.frame,
                                        reopen if save_overlay else None, png=files.get(t)))
            conf = getattr(self, '_confidence', None)
            if conf is not None and conf.planes is not None:             # config['confidence'] with 'maps': uncertainty/<frame>.png
                from .confidence import plane_job
                planes = conf.planes.cpu().numpy()
                for t, fr in enumerate(self.frames):
                    if conf.visited[t]:
                        saver.submit(plane_job(planes[t], fr.frame[:-4]))
        finally:
            saver.close()

    def save_tracks(self, masks_out_path, batch=32, counts='list', polygons=None):
        """<masks_out_path>/tracks.json (xmem2_amd/rle.py) of the masks as they stand: the frames that have one are encoded from the
        resident `masks` in launches of `batch` frames and only their run boundaries, areas and boxes reach the host; a frame without a
        mask has null in every track.  counts='compressed': the record stays on the device, is turned into the compressed COCO strings
        there (`ops.rle_compress`) and those reach the host instead of the events.  `polygons` (config['tracks_polygons']: None, True
        or {'tolerance': t}): every entry gains its polygon outlines, traced on the device (`ops.mask_polygons`), corners and never a
        mask reaching the host.  Returns the file's path."""
        from .rle import META, TrackWriter, check_count_form, default_capacity, inverse_labels
        check_count_form(counts)
        k = len(self.mapper.labels)
        if k == 0:
            raise ValueError('No valid masks provided!')
        labels = inverse_labels(self.mapper, k)
        writer = TrackWriter(*self.shape, polygons=polygons)
        present = [t for t, p in enumerate(self._present) if p]
        encoded, rings = {}, {}
        for i in range(0, len(present), max(1, int(batch))):
            chunk = present[i:i + max(1, int(batch))]
            contiguous = chunk == list(range(chunk[0], chunk[-1] + 1))
            dev = self.masks[chunk[0]:chunk[-1] + 1] if contiguous else self.masks[torch.tensor(chunk, device=self.device)]
            if writer.polygons is not None:
                pmeta, words = ops.mask_polygons(dev, k)
                rings.update((t, (pmeta[j], words[j])) for j, t in enumerate(chunk))
            if counts == 'compressed':
                capacity = default_capacity(*self.shape)
                rec = ops.rle_encode(dev, k, capacity, wait=False)
                strings = ops.rle_compress(rec, *self.shape, k, capacity)
                meta = rec[:len(chunk) * k * META].cpu().numpy().reshape(len(chunk), k, META)
                for j, t in enumerate(chunk):
                    if strings[j] is None:                               # its events did not fit: this frame again, at its exact size
                        total = int(meta[j, :, 0].sum())
                        strings[j] = ops.rle_compress(ops.rle_encode(dev[j:j + 1], k, total, wait=False), *self.shape, k, total)[0]
                    encoded[t] = (meta[j], None, strings[j])
                continue
            meta, events = ops.rle_encode(dev, k)
            for j, t in enumerate(chunk):
                encoded[t] = (meta[j], events[j], None)
        for t, fr in enumerate(self.frames):
            meta, events, strings = encoded.get(t, (None, None, None))
            writer.add_frame(fr.frame, meta, events, labels=labels, strings=strings, polygons=rings.get(t))
        if getattr(self, '_confidence', None) is not None:               # config['confidence']: "score" and "confidence"
            writer.set_confidence(self._confidence.track_entries(self.mapper))
        return writer.write(os.path.join(str(masks_out_path), 'tracks.json'))

    def save_mattes(self, masks_out_path, batch=32, **spec):
        """What config['mattes'] writes in a frame loop, of the masks as they stand: <masks_out_path>/mattes/<label>/<frame>.png and,
        with `trimap`, <masks_out_path>/trimaps/<label>/<frame>.png for every frame that has a mask and every label the mapper knows,
        made from the resident `masks` in launches of `batch` frames (`ops.mask_mattes`).  `spec`: the keys of config['mattes']
        (feather, offset, falloff, trimap); none of them is `True`, a feather of 2 pixels.  Returns the number of files."""
        from .matte import parse_mattes, write_mattes
        from .rle import inverse_labels
        spec = parse_mattes(spec or True)
        k = len(self.mapper.labels)
        if k == 0:
            raise ValueError('No valid masks provided!')

        def masks_of(frames):
            return self.masks[frames[0]:frames[-1] + 1], [self._present[t] for t in frames]
        with torch.cuda.device(self.device):
            return write_mattes(masks_of, len(self), [fr.frame[:-4] for fr in self.frames], inverse_labels(self.mapper, k),
                                masks_out_path, spec, batch)

    def load_tracks(self, path, batch=32):
        """The inverse of `save_tracks`: the frames of tracks.json (`path`: the file, or the directory that holds it) that have an
        entry are decoded on the device, in launches of `batch` frames, into the resident `masks` with dense ids and marked present;
        labels the mapper has not seen are registered as an annotation registers them.  Returns the frames' indices.  Keys are not
        restored (what needs a key pass keeps needing it) and the references are not touched.  ValueError when the file's size or
        `file_names` are not the session's; nothing has been changed then."""
        from .rle import TrackReader
        path = str(path)
        reader = TrackReader(os.path.join(path, 'tracks.json') if os.path.isdir(path) else path)
        if (reader.height, reader.width) != tuple(self.shape):
            raise ValueError(f'load_tracks: the tracks are {(reader.height, reader.width)}, the video is {tuple(self.shape)}')
        names = [fr.frame for fr in self.frames]
        if reader.length != len(names) or reader.file_names != names:
            raise ValueError(f'load_tracks: the file_names of {path!r} are not the {len(names)} frames of this video')
        if len(reader.labels) > 254:
            raise ValueError(f'load_tracks: {len(reader.labels)} tracks, at most 254 fit a launch')
        present = [t for t in range(len(names)) if reader.has_mask(t)]
        if not present:
            return present
        for lab in reader.labels:                                        # in file order, which is `save_tracks`'s dense order: a new
            self.mapper.convert_mask(np.array([[lab]], np.uint8), exhaustive=True)      # label gets the next dense id, as annotated
        dense = torch.tensor([self.mapper.remappings[lab] for lab in reader.labels], dtype=torch.uint8, device=self.device)
        step = max(1, int(batch))
        with torch.cuda.device(self.device):
            for i in range(0, len(present), step):
                chunk = present[i:i + step]
                if any(reader.has_polygons(t) for t in chunk):                     # polygon-only entries: filled, not decoded
                    got, _ = reader.masks_device(chunk, device=self.device, values=dense.tolist(), batch=step)
                    self.masks[torch.tensor(chunk, device=self.device)] = got
                    continue
                records = [reader.record(t) for t in chunk]
                record = (np.stack([m for m, _ in records]), [e for _, e in records])
                if chunk == list(range(chunk[0], chunk[-1] + 1)):                  # straight into the arena
                    ops.rle_decode(record, *self.shape, len(reader.labels), values=dense, out=self.masks[chunk[0]:chunk[-1] + 1])
                else:
                    self.masks[torch.tensor(chunk, device=self.device)] = ops.rle_decode(record, *self.shape, len(reader.labels), values=dense)
        for t in present:
            self._present[t] = True
        return present

    def stats(self, compute_iou=False, compute_jf=False):
        """The DataFrame run_on_video returns for the frames that have a mask (compute_iou / compute_jf as there)."""
        import pandas as pd
        from .metrics import InLoopScorer
        from .frame_outputs import _cleanup_report, _stats_row, _with_jf
        host = self._host_masks() if compute_iou else None
        if compute_jf and not self.all_masks_present():
            raise RuntimeError('compute_jf scores the whole video: run propagation on all frames first')
        scorer = InLoopScorer(len(self), self.device) if compute_jf else None
        rows = []
        for t, fr in enumerate(self.frames):
            if not self._present[t]:
                continue
            if scorer is not None and fr.mask is not None:
                scorer.add(t, fr.mask, self.masks[t], self.mapper)
            rows.append(_stats_row(fr.frame, t in self._refs, compute_iou, host[t] if compute_iou else None, fr.mask))
        df = _with_jf(pd.DataFrame(rows), scorer)
        if getattr(self, 'cleanup', None) is not None:                                     # what config['mask_cleanup'] did in the propagations so far
            df.attrs['cleanup'] = _cleanup_report(self._cleaned)
        return df


def _session_reader(imgs_in_path, masks_in_path, size, resize_on_device):
    """run_on_video.VideoReader (use_all_masks=True); without annotation files the reader is set up by hand - it reads no masks and
    the written masks are mapped to a grey ramp instead of the first annotation's palette."""
    from PIL import Image
    from .run_on_video import VideoReader
    if masks_in_path is not None and (os.path.isfile(masks_in_path) or len(os.listdir(masks_in_path)) > 0):
        return VideoReader('', imgs_in_path, masks_in_path, size=size, use_all_masks=True, resize_on_device=resize_on_device)
    r = VideoReader.__new__(VideoReader)
    r.resize_on_device, r._Image = bool(resize_on_device), Image
    r.vid_name, r.image_dir, r.mask_dir = '', imgs_in_path, (masks_in_path or imgs_in_path)
    r.size, r.use_all_masks = size, False
    r.frames = sorted(os.listdir(imgs_in_path))
    r.first_gt_path = None
    ramp = Image.new('P', (1, 1))
    ramp.putpalette([v for i in range(256) for v in (i, i, i)])
    r.reference_mask = ramp
    return r


# ---- command line ------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m xmem2_amd.session',
                                 description='The XMem++ loop on one video with a simulated annotator: every round propagates with the '
                                             'references so far, lets the selector propose the next frames and takes their annotations '
                                             'from --masks (run_experiments.py).')
    ap.add_argument('--images', required=True, help='directory of frames')
    ap.add_argument('--masks', required=True, help='directory of annotations (palette PNGs named like the frames), or a tracks.json (xmem2_amd/rle.py)')
    ap.add_argument('--out', required=True, help='the masks of the last round are written to <out>/masks')
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--k', type=int, default=5, help='frames the selector proposes per round')
    ap.add_argument('--first', default='0', help='comma-separated frames annotated before the first round')
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--min-mask-presence-percent', type=float, default=0.25)
    ap.add_argument('--mask-form', default='objects', choices=MASK_FORMS)
    ap.add_argument('--config', default=None, help='JSON dict merged into VIDEO_INFERENCE_CONFIG')
    ap.add_argument('--overlay', action='store_true', help='write overlays next to the masks')
    ap.add_argument('--tracks', action='store_true', help='write <out>/tracks.json, run-length tracks encoded on the device, next to the masks')
    ap.add_argument('--tracks-counts', default='list', choices=('list', 'compressed'),
                    help='the counts in tracks.json: uncompressed lists, or the compressed COCO strings built on the device')
    ap.add_argument('--tracks-polygons', nargs='?', const=0.0, default=None, type=float, metavar='TOL',
                    help='with --tracks: add the polygon outlines of every entry, traced on the device; TOL > 0 simplifies the rings (lossy)')
    ap.add_argument('--png-on-device', nargs='?', const='rgb', default=None, choices=('rgb', 'palette'), metavar='MODE',
                    help="build the mask PNGs on the device (config['png_on_device']); MODE rgb (default): today's colours, palette: index PNGs")
    ap.add_argument('--review-by', default='dissimilarity', choices=('dissimilarity', 'confidence'),
                    help="where the next frames to annotate come from: the selector's key dissimilarity (`candidates`), or the frames whose "
                         "least sure object is the least sure (`review_queue`, which turns config['confidence'] on)")
    ap.add_argument('--feature-cache-gb', type=float, default=0.0,
                    help="device memory for the key encoder's per-frame outputs (config['session_feature_cache_bytes']); 0: off")
    args = ap.parse_args(argv)
    if args.rounds < 1 or args.k < 1:
        ap.error('--rounds and --k must be at least 1')
    if args.feature_cache_gb < 0:
        ap.error('--feature-cache-gb must not be negative')
    return args


def main(argv=None):
    args = parse_args(argv)
    config = json.loads(args.config) if args.config else {}
    if args.feature_cache_gb > 0:
        config['session_feature_cache_bytes'] = int(args.feature_cache_gb * (1 << 30))
    if args.review_by == 'confidence' and config.get('confidence') is None:
        config['confidence'] = True
    s = VideoSession(args.images, args.masks, overwrite_config=config or None)
    for t in sorted(int(x) for x in args.first.split(',') if x != ''):
        s.save_reference(t)
    chosen = []
    for r in range(args.rounds):
        for t in sorted(chosen):                                         # the simulated annotator: the ground truth, where there is one
            if s.frames[t].mask is not None:
                s.save_reference(t)
        s.full_propagation()
        if len(s.references) >= len(s):
            chosen = []
        elif args.review_by == 'confidence':
            chosen = s.review_queue(k=args.k)
        else:
            with contextlib.redirect_stdout(sys.stderr):                 # the selector's progress line: stdout carries the JSON only
                chosen = s.candidates(k=args.k, alpha=args.alpha, min_mask_presence_percent=args.min_mask_presence_percent,
                                      mask_form=args.mask_form)
        print(json.dumps(dict(round=r, references=s.references, chosen=chosen)), flush=True)
    s.save(args.out, save_overlay=args.overlay, png_on_device=None if args.png_on_device is None else {'mode': args.png_on_device})
    if args.tracks:
        s.save_tracks(args.out, counts=args.tracks_counts,
                      polygons=None if args.tracks_polygons is None else {'tolerance': args.tracks_polygons})
    return 0


if __name__ == '__main__':
    sys.exit(main())
