"""Per-object confidence and per-pixel uncertainty from the decoder's class scores.  This module is the definition, in numpy;
csrc/confidence.hip (include/xmem_hip_confidence.h, `ops.confidence_stats`) gives the same bytes on the device.

For every pixel of scores [C,H,W] (float32 probabilities, or the ensemble's uint16 sums of `passes` bytes), C in 1..255:

  * top    = the first maximal class, found by `ops.argmax_u8`'s `v > best` loop;
  * second = the first maximal class among the others, by the same loop (absent when C == 1);
  * m      = p[top] - p[second], one float32 subtraction (p[top] when C == 1);
  * q      = 0 unless m > 0, 255 when m * 256.0f >= 255.0f, else (int)(m * 256.0f); the product with a power of two is exact.
             Integer scores: q = min(255, (s[top] - s[second]) // passes).

mask = top, plane = 255 - q (bright means unsure) and record int64 [C, 4]: per class its `area` (pixels with top == c), `margin_sum`
(the sum of q over them), `low` (those with q < tau) and `contested` (pixels with second == c and q < tau).

q is a MARGIN: by how much the winner led, in 1/256 of the score range.  It is not a calibrated probability - it says nothing about
how often a pixel with that margin is right - and it describes the raw prediction, before clean-up and before the temporal vote.

Derived on the host in float64: an object's confidence margin_sum / (255 area) (NaN without pixels), a frame's confidence the minimum
of that over the objects (dense ids 1 and up) that have pixels (NaN without any), a track's score sum_t margin_sum / (255 sum_t area)
over the frames that were not given a mask.

`config['confidence']` (`parse_confidence`) turns it on inside `run_on_video`, `run_on_video_ensemble` and `VideoSession.propagate`,
where `FrameConfidence` takes the place of the `ops.argmax_u8` call.
"""
import numpy as np

from .frame_outputs import Tag, _PlaneChannel

KEY = 'confidence'
MAX_C = 255
MAX_TAU = 256
MAX_PASSES = 257
DEFAULT_TAU = 64
FIELDS = ('area', 'margin_sum', 'low', 'contested')              # the record's columns, in its order
MAPS_DIR = 'uncertainty'


def _int_in(value, low, top, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not low <= value <= top:
        raise ValueError(f'{what} = {value!r} must be an integer in {low}..{top}')
    return int(value)


def parse_confidence(value):
    """config['confidence'] -> None or {'threshold': tau, 'maps': bool}: None switches it off, True is the default threshold without
    maps, a dict may name 'threshold' (0..256) and 'maps' (a bool).  Anything else raises ValueError."""
    if value is None:
        return None
    if value is True:
        return {'threshold': DEFAULT_TAU, 'maps': False}
    if not isinstance(value, dict) or set(value) - {'threshold', 'maps'}:
        raise ValueError(f"config['{KEY}'] = {value!r}: expected None, True or {{'threshold': 0..{MAX_TAU}, 'maps': bool}}")
    maps = value.get('maps', False)
    if not isinstance(maps, (bool, np.bool_)):
        raise ValueError(f"config['{KEY}']: maps = {maps!r} must be a bool")
    return {'threshold': _int_in(value.get('threshold', DEFAULT_TAU), 0, MAX_TAU, f"config['{KEY}']: threshold"), 'maps': bool(maps)}


def _first_max(scores):
    """`ops.argmax_u8`'s loop over axis 0: the first maximal index, and its value"""
    best, index = scores[0].copy(), np.zeros(scores.shape[1:], np.int64)
    for c in range(1, scores.shape[0]):
        better = scores[c] > best
        best[better] = scores[c][better]
        index[better] = c
    return index, best


def stats_host(prob, tau=DEFAULT_TAU, passes=None):
    """The definition above on the host: scores [C,H,W] - float32 with passes=None, uint16 with `passes` in 1..257 -
    -> (mask uint8 [H,W], plane uint8 [H,W], record int64 [C,4])."""
    prob = np.asarray(prob)
    want = np.float32 if passes is None else np.uint16
    if prob.ndim != 3 or prob.dtype != want or not 1 <= prob.shape[0] <= MAX_C or prob.shape[1] < 1 or prob.shape[2] < 1:
        raise ValueError(f'stats_host: scores must be {np.dtype(want).name} [C,H,W] with C in 1..{MAX_C}, got {prob.dtype} {prob.shape}')
    tau = _int_in(tau, 0, MAX_TAU, 'stats_host: tau')
    if passes is not None:
        passes = _int_in(passes, 1, MAX_PASSES, 'stats_host: passes')
        prob = prob.astype(np.int64)
    C = prob.shape[0]
    top, p_top = _first_max(prob)
    second = None
    if C > 1:
        # the same loop over the classes that are not `top`: the first of them starts it, a later one wins only with `v > best`
        best, second, started = np.zeros_like(p_top), np.zeros(top.shape, np.int64), np.zeros(top.shape, bool)
        for c in range(C):
            rest = top != c
            take = rest & (~started | (prob[c] > best))
            best[take] = prob[c][take]
            second[take] = c
            started |= rest
        m = p_top - best                                                 # one float32 subtraction, or exact integers
    else:
        m = p_top
    if passes is None:
        scaled = m * np.float32(256.0)                                   # exact: a power of two
        assert scaled.dtype == np.float32
        q = np.where(m > 0, np.where(scaled >= np.float32(255.0), 255, np.clip(scaled, 0, 255).astype(np.int64)), 0)
    else:
        q = np.minimum(255, m // passes)                                 # m >= 0: top is maximal
    low = q < tau
    record = np.zeros((C, len(FIELDS)), np.int64)
    record[:, 0] = np.bincount(top.ravel(), minlength=C)
    record[:, 1] = [int(q[top == c].sum()) for c in range(C)]
    record[:, 2] = np.bincount(top[low], minlength=C)
    if second is not None:
        record[:, 3] = np.bincount(second[low], minlength=C)
    return top.astype(np.uint8), (255 - q).astype(np.uint8), record


# ---- derived on the host, in float64 ----------------------------------------------------------------------------------------------

def object_confidence(area, margin_sum):
    """margin_sum / (255 area) per entry in float64, NaN where area == 0"""
    area, margin_sum = np.asarray(area, np.float64), np.asarray(margin_sum, np.float64)
    out = np.full(area.shape, np.nan)
    np.divide(margin_sum, 255.0 * area, out=out, where=area > 0)
    return out


def frame_confidence(area, margin_sum):
    """[T, C] (column c = dense id c, column 0 the background) -> float64 [T]: the minimum of `object_confidence` over the objects
    (columns 1 and up) that have pixels, NaN for a frame without any"""
    conf = object_confidence(area, margin_sum)[..., 1:]
    has = ~np.isnan(conf)
    if not conf.shape[-1]:
        return np.full(conf.shape[:-1], np.nan)
    out = np.where(has, conf, np.inf).min(-1)
    out[~has.any(-1)] = np.nan
    return out


def track_scores(area, margin_sum, given):
    """[T, C] and bool [T] -> float64 [C]: sum_t margin_sum / (255 sum_t area) over the frames that were not given a mask, NaN for a
    class without pixels in them"""
    keep = ~np.asarray(given, bool)
    return object_confidence(np.asarray(area)[keep].sum(0), np.asarray(margin_sum)[keep].sum(0))


def review_queue(confidence, skip=(), k=5, min_gap=0):
    """The `k` frames with the lowest frame confidence: `confidence` float [T], `skip` the frames never proposed (references, frames
    without a mask).  NaN sorts last, ties go to the lower index, a frame within `min_gap` of one already chosen is passed over.
    Pure host logic."""
    confidence = np.asarray(confidence, np.float64)
    if confidence.ndim != 1:
        raise ValueError(f'review_queue: the frame confidence must be [T], got {confidence.shape}')
    k, min_gap = _int_in(k, 1, 1 << 30, 'review_queue: k'), _int_in(min_gap, 0, 1 << 30, 'review_queue: min_gap')
    skip = {int(t) for t in skip}
    order = sorted((t for t in range(confidence.size) if t not in skip),
                   key=lambda t: (bool(np.isnan(confidence[t])), 0.0 if np.isnan(confidence[t]) else float(confidence[t]), t))
    chosen = []
    for t in order:
        if len(chosen) >= k:
            break
        if all(abs(t - c) > min_gap for c in chosen):
            chosen.append(t)
    return chosen


def table_report(tau, table, labels):
    """df.attrs['confidence'] of a host table int64 [T, C, 4]: the threshold, the annotation's labels of the columns (0, the
    background, first) and the four [T, C] arrays"""
    out = {'threshold': int(tau), 'labels': [int(v) for v in labels]}
    out.update((name, np.ascontiguousarray(table[:, :, i])) for i, name in enumerate(FIELDS))
    return out


def plane_job(plane, stem):
    """The `_AsyncSaver` job that writes a frame's uncertainty plane, 8-bit grey"""
    def job():
        from PIL import Image
        yield Image.fromarray(plane, mode='L'), MAPS_DIR, stem + '.png'
    return job


# ---- inside a frame loop ----------------------------------------------------------------------------------------------------------

class FrameConfidence:
    """config['confidence'] inside a frame loop.  `mask(ti, scores)` is what takes the place of `ops.argmax_u8`: one
    `ops.confidence_stats` launch sequence on the current stream that yields the same mask and leaves frame ti's record in row ti of a
    device table int64 [T, C, 4].  C is the number of classes known so far; when an annotation brings a new one the table is copied into
    a wider one on the device.  Nothing reaches the host before `host_table`, one transfer after the loop.  A later visit of a frame
    overwrites its row (`VideoSession.propagate`).

    `maps`: the plane of every frame goes through a `frame_outputs._PlaneChannel` of its own - one frame behind, raw or with
    `png_on_device` as the bytes of a file built on the device, to the loop's `saver` or to writers of its own - and becomes
    <masks_out_path>/uncertainty/<frame>.png, keyed by the frame it belongs to and not by what the temporal delay line hands on.
    `planes`: a uint8 [T,H,W] device tensor that receives the planes in place of any of that (the session's arena)."""

    def __init__(self, spec, vid_length, device, saver=None, masks_out_path=None, vid_name='', png_on_device=False, planes=None):
        self.tau, self.maps, self.T, self.device = spec['threshold'], bool(spec['maps']), int(vid_length), device
        self.table = None
        self.visited, self.given = [False] * self.T, [False] * self.T
        self.planes = planes
        self.channel = _PlaneChannel(saver, masks_out_path, vid_name, png_on_device) if self.maps and planes is None else None
        self._host = None

    def _row(self, ti, C):
        import torch
        if self.table is None or self.table.shape[1] < C:
            wider = torch.zeros((self.T, C, len(FIELDS)), dtype=torch.int64, device=self.device)
            if self.table is not None:
                wider[:, :self.table.shape[1]].copy_(self.table)
            self.table = wider
        return self.table[ti, :C]

    def mask(self, ti, scores, name=None, given=False, passes=None, out=None):
        """-> the index mask of `scores` [C,H,W] (into `out`, or a new tensor); frame ti's record goes into the table, its plane on
        its way.  `passes`: the integer route of the ensemble."""
        from . import ops
        want_plane = self.maps
        plane_out = self.planes[ti] if (want_plane and self.planes is not None) else None
        mask, plane, _ = ops.confidence_stats(scores, self.tau, passes, want_mask=True, want_plane=want_plane,
                                              record=self._row(ti, scores.shape[0]), mask=out, plane=plane_out)
        self.visited[ti], self.given[ti], self._host = True, bool(given), None
        if self.channel is not None:
            self._write(self.channel.send(Tag(name, had_mask=bool(given)), plane))
        return mask

    def _write(self, arrived):
        for item in arrived:
            self.channel.write(item, [(MAPS_DIR, item[0].frame[:-4] + '.png')])

    def drain(self):
        """the planes still on their way, after the last frame"""
        if self.channel is not None:
            self._write(self.channel.drain())

    def close(self):
        if self.channel is not None:
            self.channel.close()                                         # re-raises an error of writers of its own

    def host_table(self):
        """int64 [T, C, 4] on the host: one transfer, kept until the next frame is visited"""
        if self._host is None:
            self._host = np.zeros((self.T, 1, len(FIELDS)), np.int64) if self.table is None else self.table.cpu().numpy()
        return self._host

    def labels(self, mapper):
        """the annotation's label of every column of the table: 0, the background, then `rle.inverse_labels`"""
        from .rle import inverse_labels
        return [0] + inverse_labels(mapper, self.host_table().shape[1] - 1)

    def report(self, mapper):
        return table_report(self.tau, self.host_table(), self.labels(mapper))

    def frame_confidence(self):
        """float64 [T]: NaN for a frame no propagation has visited"""
        t = self.host_table()
        conf = frame_confidence(t[:, :, 0], t[:, :, 1])
        conf[~np.asarray(self.visited, bool)] = np.nan
        return conf

    def track_entries(self, mapper):
        """{label: (track score, [T] object confidence per frame)} for `rle.TrackWriter.set_confidence`: NaN is None there"""
        t = self.host_table()
        scores = track_scores(t[:, :, 0], t[:, :, 1], self.given)
        per_frame = object_confidence(t[:, :, 0], t[:, :, 1])
        return {lab: (scores[c], per_frame[:, c]) for c, lab in enumerate(self.labels(mapper)) if c > 0}
