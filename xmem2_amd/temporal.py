"""Temporal mask smoothing: a sliding majority vote along the time axis of uint8 index masks.  This module is the definition, in
numpy; csrc/temporal.hip (include/xmem_hip_temporal.h, `ops.temporal_mode`) gives the same bytes on the device.

For frame t and pixel p of masks [T,H,W], with `present` and `locked` per frame and a radius r in 1..MAX_R:

  * t not present: the frame is handed on as it is (a frame without a mask is all zero and stays so) and does not vote;
  * t locked: handed on as it is - an annotated frame is never overwritten - but it votes for its neighbours;
  * otherwise the window is the PRESENT frames among max(0, t - r) .. min(T - 1, t + r): clipped, never padded - nothing exists outside
    the video.  The winner is the label that occurs most often at p; among labels that tie, the frame's own label if it is one of
    them, else the smallest (background before objects).

Every output frame is computed from the input frames, never from a neighbour already smoothed.  The vote is not motion compensated,
hence the small MAX_R: beyond it anything that moves is smeared.

The compensated vote (`mode_mc_host`, opt-in: {'radius': r, 'motion': ...}) first aligns every neighbour block by block
(`motion.block_motion_host` on the frames' lumas): the vote of frame f at pixel p of frame t is masks[f][p + vec[block of p]], and a
block whose match is poor (SAD > max_sad per pixel) abstains for f.  The frame rules and the key are the same.

`config['temporal_smooth']` (`parse_smooth`) turns it on inside `run_on_video` and `run_on_video_ensemble`, where `DelayLine` holds
frames back by r; `VideoSession.smooth` and `rle.smooth_tracks` apply it to results that exist.
"""
import numpy as np

MAX_R = 7            # a window of at most 15 frames: a count fits four bits
MAX_T = 65535        # frames of a video the kernel's entry point accepts
KEY = 'temporal_smooth'


def _radius(radius, where):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_R:
        raise ValueError(f'{where}: radius = {radius!r} must be an integer in 1..{MAX_R}')
    return int(radius)


def parse_smooth(value):
    """config['temporal_smooth'] -> {'radius': r} or None: None / False switch it off, True is radius 1, an int r or {'radius': r}
    with r in 1..MAX_R is that radius.  {'radius': r, 'motion': True | {'search': s, 'bias': b, 'max_sad': m}} asks for the
    motion-compensated vote -> {'radius': r, 'motion': {'search', 'bias', 'max_sad'}} (`motion.parse_motion` has the ranges and the
    defaults).  Anything else raises ValueError."""
    if value is None or value is False:
        return None
    if value is True:
        return {'radius': 1}
    if isinstance(value, dict) and set(value) == {'radius', 'motion'}:
        from .motion import parse_motion
        return {'radius': _radius(value['radius'], f"config['{KEY}']"), 'motion': parse_motion(value['motion'], f"config['{KEY}']['motion']")}
    if isinstance(value, dict):
        if set(value) != {'radius'}:
            raise ValueError(f"config['{KEY}'] = {value!r}: a dict must have the key 'radius' and may have 'motion'")
        value = value['radius']
    elif not isinstance(value, (int, np.integer)):
        raise ValueError(f"config['{KEY}'] = {value!r}: expected None, a bool, a radius in 1..{MAX_R} or {{'radius': r}}")
    return {'radius': _radius(value, f"config['{KEY}']")}


def frame_flags(T, present=None, locked=None):
    """bool [T] `present` (default: all) and `locked` (default: none) as the uint8 [T] flags of xmem_temporal_mode (1 present, 2 locked)"""
    present = np.ones(T, bool) if present is None else np.asarray(present, bool)
    locked = np.zeros(T, bool) if locked is None else np.asarray(locked, bool)
    if present.shape != (T,) or locked.shape != (T,):
        raise ValueError(f'temporal: present {present.shape} and locked {locked.shape} must both be [{T}]')
    return present.astype(np.uint8) | (locked.astype(np.uint8) << 1)


def mode_host(masks, radius, present=None, locked=None):
    """The definition above on the host: uint8 [T,H,W] -> (out uint8 [T,H,W], changed int64 [T] = pixels with out != masks)."""
    masks = np.asarray(masks)
    if masks.dtype != np.uint8 or masks.ndim != 3:
        raise ValueError(f'mode_host: masks must be uint8 [T,H,W], got {masks.dtype} {masks.shape}')
    r = _radius(radius, 'mode_host')
    T = masks.shape[0]
    flags = frame_flags(T, present, locked)
    out = masks.copy()
    changed = np.zeros(T, np.int64)
    for t in range(T):
        if flags[t] != 1:                                            # absent, or locked
            continue
        voters = [f for f in range(max(0, t - r), min(T - 1, t + r) + 1) if flags[f] & 1]
        win = masks[voters].astype(np.int32)                         # [n,H,W]
        centre = win[voters.index(t)]
        count = (win[:, None] == win[None]).sum(1)                   # occurrences of each entry's label
        key = count * 512 + (win == centre) * 256 + (255 - win)
        out[t] = np.take_along_axis(win, key.argmax(0)[None], 0)[0].astype(np.uint8)
        changed[t] = int((out[t] != masks[t]).sum())
    return out, changed


def mode_mc_host(masks, luma, radius, search=None, bias=None, max_sad=None, present=None, locked=None):
    """The motion-compensated vote on the host: masks and luma uint8 [T,H,W] -> (out uint8 [T,H,W], changed int64 [T]).  The frame
    rules are `mode_host`'s.  For an output frame t and a voting frame f != t of its window, `block_motion_host(luma[t], luma[f])`
    gives every block a vector and a SAD; f votes masks[f][p + vec] at the block's pixels unless SAD > max_sad * pixels of the block,
    where it abstains.  The centre always votes with its own pixel; the key is `mode_host`'s over the entries that vote."""
    from . import motion
    masks, luma = np.asarray(masks), np.asarray(luma)
    if masks.dtype != np.uint8 or masks.ndim != 3 or luma.dtype != np.uint8 or luma.shape != masks.shape:
        raise ValueError(f'mode_mc_host: masks and luma must be uint8 [T,H,W] of one shape, got {masks.dtype} {masks.shape} and {luma.dtype} {luma.shape}')
    r = _radius(radius, 'mode_mc_host')
    spec = motion.parse_motion({k: v for k, v in (('search', search), ('bias', bias), ('max_sad', max_sad)) if v is not None}, 'mode_mc_host')
    T, H, W = masks.shape
    flags = frame_flags(T, present, locked)
    limit = spec['max_sad'] * motion.block_pixels(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = masks.copy()
    changed = np.zeros(T, np.int64)
    for t in range(T):
        if flags[t] != 1:
            continue
        centre = masks[t].astype(np.int32)
        win, votes = [centre], [np.ones((H, W), bool)]
        for f in range(max(0, t - r), min(T - 1, t + r) + 1):
            if f == t or not flags[f] & 1:
                continue
            vec, sad = motion.block_motion_host(luma[t], luma[f], spec['search'], spec['bias'])
            v = motion.per_pixel(vec, H, W).astype(np.int32)
            win.append(masks[f][yy + v[..., 0], xx + v[..., 1]].astype(np.int32))
            votes.append(motion.per_pixel(sad <= limit, H, W))
        win, votes = np.stack(win), np.stack(votes)
        count = ((win[:, None] == win[None]) & votes[None]).sum(1)   # occurrences of each entry's label among the entries that vote
        key = np.where(votes, count * 512 + (win == centre) * 256 + (255 - win), -1)
        out[t] = np.take_along_axis(win, key.argmax(0)[None], 0)[0].astype(np.uint8)
        changed[t] = int((out[t] != masks[t]).sum())
    return out, changed


class DelayLine:
    """config['temporal_smooth'] inside a frame loop: `_FrameOutputs`' interface (submit, drain, deliver, close, stats) round the real
    one, `inner`, and a delay line of r frames - a device ring of 2 r + 1 masks at output resolution, the pending (ti, sample,
    had_mask) tags and a device array of one flag byte per frame of the video.

    `submit` of frame t copies the mask into slot t % ring (the caller may rewrite its tensor), sets the frame's flag - locked exactly
    when `had_mask` - and, from t = r on, emits frame t - r: one `temporal_mode_ring` launch, then `inner.submit` with that frame's
    own tag.  `drain` emits the last r frames with their windows clipped at the end of the video - a `deliver` after each, since a
    submit overwrites what the one before it brought - and drains `inner`.  A video of at most r frames is emitted there entirely.

    `inner.submit` of frame t - r runs when frame t is in: `len(mapper.labels)` is the label count as of the NEWER frame.  That is
    wanted: a vote can bring a label into a frame before the frame it was first annotated on, and the track record must have that row.

    No host synchronisation: the flags are uploaded as 'present' for every frame before the loop, and a frame with a mask of its own
    patches its byte by a device fill.  The per-frame counts of changed pixels stay on the device until `report`.

    With spec['motion'] (the compensated vote) a second ring holds the frames' lumas: `submit` uploads `frame_of(sample)` - the
    frame at the mask's size, uint8 [H,W,3], pinned by the loop's decoder - and writes its luma into slot t % ring; `_emit` runs
    `temporal_mode_mc_ring` - the motion search of the frame against its window, then the vote.  Three launches per frame and still
    no host synchronisation.  The upload is a second one: the loop's own device copy of the frame is not reused.  `vote`, `luma` and `frame_of` are stand-ins for host tests."""

    def __init__(self, inner, spec, vid_length, device, vote=None, luma=None, frame_of=None):
        import torch
        self.inner, self.r, self.T, self.device = inner, spec['radius'], int(vid_length), device
        self.ring = 2 * self.r + 1
        self.motion = spec.get('motion')
        if not 1 <= self.T <= MAX_T:
            raise ValueError(f"config['{KEY}']: a video of {self.T} frames; the vote serves 1..{MAX_T}")
        if self.motion is not None and frame_of is None:
            raise ValueError(f"config['{KEY}']['motion'] needs the loop's frames: frame_of(sample) -> uint8 [H,W,3] of the mask's size")
        if vote is None or (self.motion is not None and luma is None):
            from . import ops
            vote = vote or (ops.temporal_mode_ring if self.motion is None else ops.temporal_mode_mc_ring)
            luma = luma or ops.luma_u8
        self.vote, self.luma, self.frame_of = vote, luma, frame_of
        self.flags = torch.full((self.T,), 1, dtype=torch.uint8, device=device)
        self.changed = torch.zeros(self.T, dtype=torch.int32, device=device)
        self.frames = None                                           # [ring,H,W], allocated with the first mask
        self.lumas = self.vec = self.sad = None                      # with 'motion': the lumas beside them, and one frame's vectors
        self.pending = []
        self.emitted = 0

    @property
    def stats(self):
        return self.inner.stats

    def _emit(self):
        ti, sample, had_mask = self.pending.pop(0)
        if self.motion is None:
            out, _ = self.vote(self.frames, self.T, ti, 1, self.r, self.flags, changed=self.changed[ti:ti + 1])
        else:
            out, _ = self.vote(self.frames, self.lumas, self.T, ti, 1, self.r, self.flags, changed=self.changed[ti:ti + 1],
                               vec=self.vec, sad=self.sad, **self.motion)
        self.emitted += 1
        self.inner.submit(ti, sample, had_mask, out[0])

    def submit(self, ti, sample, had_mask, out_dev):
        import torch
        if self.frames is None:
            self.frames = torch.zeros((self.ring,) + tuple(out_dev.shape), dtype=torch.uint8, device=out_dev.device)
            if self.motion is not None:
                from .motion import blocks_of
                blocks = (1, 2 * self.r) + blocks_of(*out_dev.shape)
                self.lumas = torch.zeros_like(self.frames)
                self.vec = torch.zeros(blocks + (2,), dtype=torch.int8, device=out_dev.device)
                self.sad = torch.zeros(blocks, dtype=torch.int32, device=out_dev.device)
        self.frames[ti % self.ring].copy_(out_dev)
        if self.motion is not None:
            rgb = self.frame_of(sample)
            if tuple(rgb.shape) != tuple(out_dev.shape) + (3,):
                raise ValueError(f"config['{KEY}']['motion']: frame {ti} is {tuple(rgb.shape)}, its mask {tuple(out_dev.shape)}: the "
                                 f"motion search runs at the mask's size")
            self.luma(rgb.to(out_dev.device, non_blocking=True), out=self.lumas[ti % self.ring])
        if had_mask:
            self.flags[ti:ti + 1].fill_(3)
        self.pending.append((ti, sample, had_mask))
        if ti >= self.r:
            self._emit()

    def drain(self):
        while self.pending:
            self._emit()
            self.inner.deliver()
        self.inner.drain()

    def deliver(self, last=False):
        self.inner.deliver(last=last)

    def close(self):
        self.inner.close()

    def report(self):
        """{'radius', 'pixels_changed', 'frames_changed'} of the video, and with the compensated vote 'motion': {'search', 'bias',
        'max_sad'}: one transfer, after the loop"""
        changed = self.changed.cpu().numpy().astype(np.int64)
        out = {'radius': self.r, 'pixels_changed': int(changed.sum()), 'frames_changed': int((changed > 0).sum())}
        if self.motion is not None:
            out['motion'] = dict(self.motion)
        return out
