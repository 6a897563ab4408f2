"""Run-length object tracks: the host side of `ops.rle_encode` and the file `<masks_out_path>/tracks.json`.

The specification (plain numpy, `encode_host` / `decode`), which the kernel of csrc/rle.hip is tested against:

* the COCO order of pixel (y, x) of an H x W plane is j = x * H + y (column-major; the bottom pixel of column x and the top pixel of
  column x + 1 are neighbours, a run continues across them);
* for label k the binary plane is b_k[j] = (mask[j] == k) with b_k[-1] := 0; an EVENT of k is a j with b_k[j] != b_k[j - 1];
* the uncompressed COCO counts of k are diff([0, events..., H * W]): they start with the run of zeros (0 long when pixel 0 belongs to
  k), every later count is positive, they sum to H * W.

The device finds the events, areas and boxes (`ops.rle_encode`); the host turns events into counts (`counts_from_events`) - work per
event, never per pixel.  `TrackWriter` collects one video's frames into the YouTube-VIS layout

    {"videos": [{"id": 1, "height": H, "width": W, "length": T, "file_names": [...]}],
     "categories": [{"id": 1, "name": "object"}],
     "annotations": [{"id": n, "video_id": 1, "category_id": 1, "label": <label in the annotation PNGs>,
                      "segmentations": [{"size": [H, W], "counts": [...] | "..."} | null, ...],      one entry per frame
                      "bboxes": [[x, y, w, h] | null, ...], "areas": [int | null, ...]}]}

`counts` is the uncompressed list form, which COCO tools accept, or - config['tracks_counts'] = 'compressed' - the compressed ASCII
string of the COCO mask API (`compress_counts` / `decompress_counts` are its definition: the counts from the fourth on as differences
to the count two before, every value as little-endian groups of 5 bits with a continuation bit, characters '0'..'o'), the dict
`pycocotools.mask.decode` takes.  The device builds the strings from the event record (`ops.rle_compress`: per count a function of
four neighbouring events, then a scan) and reads them back into the record (`ops.rle_decompress`); every reader here takes both
forms, also mixed in one file.  A frame in which a label has no pixel, or which has no mask at all, carries null in all three lists.
With config['tracks_polygons'] an entry also holds "polygons": [[x0, y0, x1, y1, ...], ...], its outline as rings of lattice corners
(xmem2_amd/polygons.py, traced by `ops.mask_polygons`), and the video "polygons": {"tolerance": t, "fill": "evenodd"}; no reader here
needs the key.
`python -m xmem2_amd.rle --tracks F --out DIR` is the way back to index PNGs (`--recode` rewrites a file in the other form);
`TrackReader` is the way back without them: counts to events per event (`events_from_counts`), events to label maps
on the device (`ops.rle_decode`) - for scoring (`metrics.compute_metrics`), as annotations (`run_on_video.VideoReader`) and for
`VideoSession.load_tracks`.
"""
import argparse
import collections
import json
import os
import sys

import numpy as np

from ._lib import RLE_META as META              # int32 per (frame, label): events, area, x0, y0, x1, y1
EMPTY_BOX = (0, 0, -1, -1)
MIN_CAPACITY = 2048

HostRle = collections.namedtuple('HostRle', 'events counts area box')


def default_capacity(h, w):
    """Events per frame `ops.rle_encode` makes room for when it is not told: a label that crosses every column of the frame in two runs
    has 4 * W events, the clips measured so far stay far below it; more is never lost, the frame is encoded again."""
    return max(MIN_CAPACITY, 4 * int(w))


def default_char_capacity(h, w, capacity=None):
    """Bytes per frame `ops.rle_compress` makes room for when it is not told: two characters per event of `default_capacity`.  A count
    below 16 takes one character and a difference between counts within +-512 two, which covers the runs of an object outline (the
    chair annotations take 1.5 to 1.7 characters per count, about 1000 per frame); more is never lost, the frame is compressed again
    with its true length."""
    return 2 * (default_capacity(h, w) if capacity is None else int(capacity))


def compress_counts(counts):
    """Uncompressed COCO counts -> the compressed ASCII string of the COCO mask API (rleToString), the definition the device is tested
    against: x[i] = c[i] for i <= 2 and c[i] - c[i - 2] after that, every x as little-endian groups of 5 bits, bit 0x20 of a character
    saying that another group follows (it does until the remaining bits are the sign alone), characters offset by 48."""
    counts = [int(c) for c in counts]
    out = []
    for i, c in enumerate(counts):
        x = c - counts[i - 2] if i > 2 else c
        more = True
        while more:
            g = x & 0x1f
            x >>= 5                                                  # arithmetic: -1 stays -1
            more = (x != -1) if (g & 0x10) else (x != 0)
            out.append(chr((g | (0x20 if more else 0)) + 48))
    return ''.join(out)


MAX_GROUPS = 6                                  # characters per value: 30 bits, enough for |x| < 2^29 > 16384 * 16384


def decompress_counts(s):
    """The inverse of `compress_counts` (rleFrString): a str or ASCII bytes -> the list of counts.  ValueError for a character outside
    '0'..'o', a value of more than MAX_GROUPS characters, a string that ends inside a value and an empty string."""
    if isinstance(s, str):
        try:
            s = s.encode('ascii')
        except UnicodeEncodeError:
            raise ValueError('decompress_counts: a character outside 48..111') from None
    s = bytes(s)
    if not s:
        raise ValueError('decompress_counts: an empty string holds no counts')
    counts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise ValueError('decompress_counts: the string ends inside a value')
            c = s[p] - 48
            if not (0 <= c <= 63):
                raise ValueError(f'decompress_counts: character {s[p]} at {p} is outside 48..111')
            if k >= MAX_GROUPS:
                raise ValueError(f'decompress_counts: the value at {p - k} has more than {MAX_GROUPS} characters')
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def is_compressed(counts):
    """True for the string form of `counts` (str or bytes), False for the list form."""
    return isinstance(counts, (str, bytes, bytearray))


def _count_array(counts):
    """Either form of `counts` -> int64 [m]."""
    if is_compressed(counts):
        counts = decompress_counts(counts)
    return np.asarray(counts, dtype=np.int64).reshape(-1)


def counts_from_events(events, h, w):
    """Ascending event positions of one label -> its uncompressed COCO counts (a list of ints)."""
    ev = np.asarray(events, dtype=np.int64).reshape(-1)
    return np.diff(np.concatenate(([0], ev, [int(h) * int(w)]))).tolist()


def encode_host(mask, k):
    """The specification: label k of an H x W index array -> HostRle(events uint32 [E], counts list, area, box (x0, y0, x1, y1)
    inclusive; EMPTY_BOX without a pixel)."""
    mask = np.asarray(mask)
    if mask.ndim != 2:
        raise ValueError(f'encode_host: expected an H x W array, got shape {mask.shape}')
    h, w = mask.shape
    plane = mask == k
    b = plane.T.reshape(-1)                                          # column-major
    events = np.flatnonzero(b != np.concatenate(([False], b[:-1]))).astype(np.uint32)
    area = int(b.sum())
    if area:
        ys, xs = np.flatnonzero(plane.any(axis=1)), np.flatnonzero(plane.any(axis=0))
        box = (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))
    else:
        box = EMPTY_BOX
    return HostRle(events, counts_from_events(events, h, w), area, box)


def events_from_counts(counts, h, w):
    """COCO counts of one label (list or compressed string) -> its ascending event positions (uint32), the inverse of
    `counts_from_events`; refuses what `decode` refuses.  A cumulative sum: work per event."""
    counts = _count_array(counts)
    if counts.size == 0 or (counts < 0).any() or (counts[1:] == 0).any() or int(counts.sum()) != int(h) * int(w):
        raise ValueError(f'events_from_counts: counts do not describe a {h} x {w} plane')
    return np.cumsum(counts[:-1]).astype(np.uint32)                  # the last count ends at h * w, which is no event


def decode(counts, h, w):
    """COCO counts (list or compressed string) -> bool [h, w]."""
    counts = _count_array(counts)
    if counts.size == 0 or (counts < 0).any() or (counts[1:] == 0).any() or int(counts.sum()) != int(h) * int(w):
        raise ValueError(f'decode: counts do not describe a {h} x {w} plane')
    values = (np.arange(counts.size) & 1).astype(bool)
    return np.repeat(values, counts).reshape(int(w), int(h)).T


def split_record(buf, n_frames, k, capacity):
    """The int32 words one `ops.rle_encode` launch leaves ([n_frames * k * META] meta, then [n_frames * capacity] events) ->
    (meta int32 [n_frames, k, META], events uint32 [n_frames, capacity]) as views."""
    buf = np.asarray(buf).reshape(-1).view(np.int32)
    cut = n_frames * k * META
    return buf[:cut].reshape(n_frames, k, META), buf[cut:cut + n_frames * capacity].view(np.uint32).reshape(n_frames, capacity)


def split_string_record(buf, n_frames, k, char_capacity):
    """The bytes one `ops.rle_compress` launch leaves ([n_frames * k] int32 string lengths, then [n_frames * char_capacity] characters)
    -> (str_len int32 [n_frames, k], chars uint8 [n_frames, char_capacity]) as views."""
    buf = np.asarray(buf).reshape(-1).view(np.uint8)
    cut = 4 * n_frames * k
    return buf[:cut].view(np.int32).reshape(n_frames, k), buf[cut:cut + n_frames * char_capacity].reshape(n_frames, char_capacity)


def label_strings(str_len, chars):
    """One frame's packed characters -> the list of per-label strings (label 1 first, '' for a label without event).  `str_len` [K]
    holds the true lengths; the frame must have been compressed with room for all of them."""
    n = np.asarray(str_len).astype(np.int64)
    if (n < 0).any() or int(n.sum()) > len(chars):
        raise ValueError(f'label_strings: {int(n.sum())} characters, but only {len(chars)} were kept - compress the frame again')
    text = bytes(chars[:int(n.sum())]).decode('ascii')
    ends = np.cumsum(n)
    return [text[e - c:e] for c, e in zip(n, ends)]


def label_events(meta, events):
    """One frame's packed events -> the list of per-label event arrays (label 1 first).  `meta` [K, META] holds the true counts; the
    frame must have been encoded with room for all of them."""
    n = meta[:, 0].astype(np.int64)
    if int(n.sum()) > len(events):
        raise ValueError(f'label_events: {int(n.sum())} events, but only {len(events)} were kept - encode the frame again')
    ends = np.cumsum(n)
    return [events[e - c:e] for c, e in zip(n, ends)]


def record_host(mask, k):
    """(meta [k, META], packed events) of an H x W index array as `ops.rle_encode` returns them for one frame, by `encode_host`."""
    meta = np.zeros((k, META), np.int32)
    ev = []
    for lab in range(1, k + 1):
        r = encode_host(mask, lab)
        meta[lab - 1] = (len(r.events), r.area) + tuple(r.box)
        ev.append(r.events)
    return meta, np.concatenate(ev) if ev else np.zeros(0, np.uint32)


COUNT_FORMS = ('list', 'compressed')            # config['tracks_counts']
FILL_RULES = ('evenodd', 'union')               # the video entry's polygons.fill: an entry's rings filled together, or each on its own


def check_count_form(counts):
    if counts not in COUNT_FORMS:
        raise ValueError(f"tracks_counts must be one of {COUNT_FORMS}, got {counts!r}")
    return counts


def box_xywh(row):
    """A meta row (events, area, x0, y0, x1, y1 with inclusive corners) -> the file's [x, y, w, h]."""
    x0, y0, x1, y1 = (int(v) for v in row[2:6])
    return [x0, y0, x1 - x0 + 1, y1 - y0 + 1]


def read_json(path):
    with open(path) as f:
        return json.load(f)


def write_json(doc, path):
    """Write `doc` as compact JSON to the file `path`, whose directory is made; returns the text."""
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    text = json.dumps(doc, separators=(',', ':'))                    # dumps, not dump: one pass of the C encoder
    with open(path, 'w') as f:
        f.write(text)
    return text


def batches(frames, step):
    """The sequence `frames` in lists of `step` (at least 1), the last one shorter: what one launch serves."""
    step = max(1, int(step))
    for i in range(0, len(frames), step):
        yield list(frames[i:i + step])


class TrackWriter:
    """One video's tracks.  Frames are added in order; a track is opened when its label is first named and has null wherever the
    label was not known yet, had no pixel, or the frame had no mask."""

    def __init__(self, height, width, polygons=None):
        """`polygons`: config['tracks_polygons'] (None: the file is what it is without the option; xmem2_amd/polygons.py)."""
        from .polygons import parse_polygons
        self.height, self.width = int(height), int(width)
        self.file_names = []
        self._tracks = collections.OrderedDict()                     # label in the annotation PNGs -> {frame index: (counts, bbox, area)}
        self.polygons = parse_polygons(polygons)
        self._rings = {}                                             # (label, frame index) -> the entry's rings as flat integer lists
        self._confidence = None                                      # config['confidence']: label -> (track score, per-frame confidence)

    def open_track(self, label):
        """The entries {frame index: (counts, bbox, area)} of the track with this label, opened - so far without any - when the label
        is new: a track that never gets an entry is written with null in every frame."""
        return self._tracks.setdefault(int(label), {})

    def add_frame(self, file_name, meta=None, events=None, labels=None, strings=None, polygons=None):
        """`meta` [K, META] and the frame's packed `events` as `ops.rle_encode` gives them (`events` holding all of them), `labels`
        the annotation's label of every row (default 1..K; `inverse_labels`).  Without `meta` the frame has no mask.  `strings`: the
        rows' compressed counts as `ops.rle_compress` gives them; they are written in place of the lists and `events` is not read.
        `polygons`: (meta [K, 2], packed corner words) of the frame as `ops.mask_polygons` gives them; a writer made with the option
        needs them for every frame that has a mask, and simplifies each ring with its tolerance."""
        t = len(self.file_names)
        self.file_names.append(str(file_name))
        if meta is None:
            return
        meta = np.asarray(meta)
        labels = list(range(1, len(meta) + 1)) if labels is None else [int(v) for v in labels]
        if len(labels) != len(meta):
            raise ValueError(f'add_frame: {len(meta)} label rows, {len(labels)} labels')
        if strings is not None and len(strings) != len(meta):
            raise ValueError(f'add_frame: {len(meta)} label rows, {len(strings)} strings')
        rows = label_events(meta, events) if strings is None else strings
        if (polygons is None) != (self.polygons is None):
            raise ValueError('add_frame: a frame\'s polygons are given exactly when the writer was made with the option')
        rings = [None] * len(meta)
        if polygons is not None:
            from . import polygons as poly
            if len(polygons[0]) != len(meta):
                raise ValueError(f'add_frame: {len(meta)} label rows, polygons of {len(polygons[0])}')
            rings = poly.label_flat(*polygons, tolerance=self.polygons['tolerance'])
        for lab, row, ev, rr in zip(labels, meta, rows, rings):
            track = self.open_track(lab)
            area = int(row[1])
            if area and rr is not None:
                self._rings[(lab, t)] = rr
            if area:
                counts = counts_from_events(ev, self.height, self.width) if strings is None else str(ev)
                track[t] = (counts, box_xywh(row), area)

    def set_confidence(self, entries):
        """config['confidence'] (xmem2_amd/confidence.py): `entries` maps a track's label to (its score, its confidence in every
        frame).  Every annotation then gains "score" and every non-null segmentation "confidence"; NaN - no pixel to judge by - is
        written as null, and so is everything of a label without an entry.  Without this call the file is what it was."""
        self._confidence = {int(lab): (float(score), [float(v) for v in per_frame]) for lab, (score, per_frame) in entries.items()}

    def add_mask(self, file_name, mask, k=None, labels=None, counts='list'):
        """A frame from a host index array (dense ids 1..k, default its largest id), encoded on the host; None: a frame without mask.
        counts='compressed' writes the string form (`compress_counts`)."""
        check_count_form(counts)
        if mask is None:
            return self.add_frame(file_name)
        mask = np.asarray(mask)
        if tuple(mask.shape) != (self.height, self.width):
            raise ValueError(f'add_mask: expected {(self.height, self.width)}, got {tuple(mask.shape)}')
        k = int(mask.max()) if k is None else int(k)
        from . import polygons as poly
        if k == 0:
            return self.add_frame(file_name, np.zeros((0, META), np.int32), np.zeros(0, np.uint32), [],
                                  polygons=None if self.polygons is None else (np.zeros((0, poly.META), np.int32), np.zeros(0, np.uint32)))
        meta, events = record_host(mask, k)
        strings = None
        if counts == 'compressed':
            strings = [compress_counts(counts_from_events(ev, self.height, self.width)) for ev in label_events(meta, events)]
        return self.add_frame(file_name, meta, events, labels=labels, strings=strings,      # on the host, so are the rings
                              polygons=None if self.polygons is None else poly.record_host(mask, k))

    def to_dict(self):
        T, size = len(self.file_names), [self.height, self.width]
        anns = []
        for n, (lab, track) in enumerate(self._tracks.items(), start=1):
            seg = [{'size': size, 'counts': track[t][0]} if t in track else None for t in range(T)]
            if self.polygons is not None:
                for t in track:
                    seg[t]['polygons'] = self._rings[(lab, t)]
            anns.append({'id': n, 'video_id': 1, 'category_id': 1, 'label': lab, 'segmentations': seg,
                         'bboxes': [track[t][1] if t in track else None for t in range(T)],
                         'areas': [track[t][2] if t in track else None for t in range(T)]})
            if self._confidence is not None:
                def number(v):
                    return None if v != v else v                     # NaN is no JSON
                score, per_frame = self._confidence.get(lab, (float('nan'), []))
                anns[-1]['score'] = number(score)
                for t in track:
                    seg[t]['confidence'] = number(per_frame[t]) if t < len(per_frame) else None
        video = {'id': 1, 'height': self.height, 'width': self.width, 'length': T, 'file_names': list(self.file_names)}
        if self.polygons is not None:                                # simplified rings are lossy: the file says how it was written
            video['polygons'] = {'tolerance': self.polygons['tolerance'], 'fill': 'evenodd'}
        return {'videos': [video], 'categories': [{'id': 1, 'name': 'object'}], 'annotations': anns}

    def write(self, path):
        """Write the file (`path`: the file, or a directory that gets tracks.json); returns the file's path."""
        path = str(path)
        if os.path.isdir(path) or not path.endswith('.json'):
            path = os.path.join(path, 'tracks.json')
        write_json(self.to_dict(), path)
        return path


def inverse_labels(mapper, k):
    """The annotation's label of the dense ids 1..k of a MaskMapper (`remap_index_mask`, per label instead of per pixel)."""
    inv = {dense: original for original, dense in mapper.remappings.items()}
    return [int(inv.get(d, d)) for d in range(1, k + 1)]


def read_tracks(path):
    """tracks.json -> (video dict, list of index masks uint8 [H, W] holding the annotations' labels, None for a frame in which no
    track has an entry)."""
    doc = read_json(path)
    if len(doc.get('videos', [])) != 1:
        raise ValueError('read_tracks: expected one video per file')
    if any(seg is not None and 'counts' not in seg and 'polygons' in seg
           for ann in doc['annotations'] for seg in ann['segmentations']):       # polygon-only entries: the reader that knows them
        reader = TrackReader(doc)
        return reader.video, [reader.mask_host(t) for t in range(len(reader))]
    video = doc['videos'][0]
    h, w, T = int(video['height']), int(video['width']), int(video['length'])
    masks = [None] * T
    for ann in doc['annotations']:
        lab = int(ann['label'])
        if not (1 <= lab <= 255):
            raise ValueError(f'read_tracks: label {lab} does not fit an index PNG')
        if not (len(ann['segmentations']) == len(ann['bboxes']) == len(ann['areas']) == T):
            raise ValueError(f'read_tracks: track {ann["id"]} does not have one entry per frame')
        for t, seg in enumerate(ann['segmentations']):
            if seg is None:
                continue
            if list(seg['size']) != [h, w]:
                raise ValueError(f'read_tracks: track {ann["id"]}, frame {t}: size {seg["size"]} is not the video\'s {[h, w]}')
            if masks[t] is None:
                masks[t] = np.zeros((h, w), np.uint8)
            masks[t][decode(seg['counts'], h, w)] = lab
    return video, masks


def ring_rows(rings, fill):
    """An entry's rings as the rows of a fill: under 'evenodd' one row (its rings filled together, holes being rings), under 'union'
    one row per ring, each filled on its own."""
    return [[r] for r in rings] if fill == 'union' else [rings]


def pack_rows(rings_of, values, fill, least=0):
    """The rows that let one `ops.fill_polygons` serve a batch of frames -> (rows of every frame, value of every row).
    rings_of[a][j]: the rings of track a (there is at least one) in frame j, None where it has no polygon; values[a]: what its pixels
    get.  Every track owns a fixed run of rows in all frames - as many as its longest `ring_rows` list among them and at least
    `least`, shorter lists padded with [] -, so one values table serves them all; the first track gets a row when nobody has one."""
    per = [[[] if rings is None else ring_rows(rings, fill) for rings in of_track] for of_track in rings_of]
    width = [max([least] + [len(rows) for rows in of_track]) for of_track in per]
    if not any(width):
        width[0] = 1
    rows = [[row for of_track, n in zip(per, width) for row in of_track[j] + [[]] * (n - len(of_track[j]))] for j in range(len(per[0]))]
    return rows, [v for v, n in zip(values, width) for _ in range(n)]


class TrackReader:
    """One video's tracks.json, parsed once (`path_or_doc`: the file, or the parsed document) with `read_tracks`'s validation.  The
    annotations are the label rows of a record in file order, so a later annotation wins where tracks overlap, as in `read_tracks`.
    `mask_host(t)` decodes a frame on the host (few frames: annotations); `masks_device` builds packed records from the counts - work
    per event, never per pixel - and decodes them with `ops.rle_decode`.  Counts may be lists or compressed strings, also mixed in one
    file: a frame whose entries are all strings goes up as bytes and becomes its record on the device (`ops.rle_decompress`), the host
    doing nothing per character; `mask_host` and `record` read a string with `decompress_counts`.
    An entry may hold `polygons` without `counts` (a polygon-only entry: hand-drawn annotations, `polygons.from_labelme`; its `size`
    is optional, `bboxes` / `areas` may be null).  The video entry's `polygons.fill` names the rule: 'evenodd' (default: an entry's
    rings filled together, holes are rings) or 'union' (every ring on its own).  `mask_host` fills such a frame with
    `polygons.fill_rows_host`, `masks_device` with `ops.fill_polygons`; it has no `record`.  An entry with both keys is read from
    its counts.  A frame that mixes polygon-only entries with counts entries raises ValueError when it is read."""

    def __init__(self, path_or_doc):
        doc = path_or_doc if isinstance(path_or_doc, dict) else read_json(path_or_doc)
        if len(doc.get('videos', [])) != 1:
            raise ValueError('read_tracks: expected one video per file')
        self.video = doc['videos'][0]
        self.height, self.width, self.length = int(self.video['height']), int(self.video['width']), int(self.video['length'])
        self.file_names = [str(n) for n in self.video.get('file_names', [])]
        h, w, T = self.height, self.width, self.length
        self.labels, self._segs = [], []                             # per annotation: its label, {frame index: counts}
        self._polys = []                                             # per annotation: {frame index: rings} of its polygon-only entries
        self.fill = (self.video.get('polygons') or {}).get('fill', 'evenodd')
        if self.fill not in FILL_RULES:
            raise ValueError(f'read_tracks: polygons.fill = {self.fill!r}, known: {FILL_RULES}')
        for ann in doc['annotations']:
            lab = int(ann['label'])
            if not (1 <= lab <= 255):
                raise ValueError(f'read_tracks: label {lab} does not fit an index PNG')
            per_frame = [ann['segmentations']] + [v for v in (ann.get('bboxes'), ann.get('areas')) if v is not None]
            polygon_only = [seg is not None and 'counts' not in seg and 'polygons' in seg for seg in ann['segmentations']]
            if any(len(v) != T for v in per_frame) or (len(per_frame) != 3 and not any(polygon_only)):
                raise ValueError(f'read_tracks: track {ann["id"]} does not have one entry per frame')
            segs, polys = {}, {}
            for t, seg in enumerate(ann['segmentations']):
                if seg is None:
                    continue
                if ('size' in seg or not polygon_only[t]) and list(seg['size']) != [h, w]:
                    raise ValueError(f'read_tracks: track {ann["id"]}, frame {t}: size {seg["size"]} is not the video\'s {[h, w]}')
                if polygon_only[t]:                                  # an entry with both keys is read from its counts
                    polys[t] = seg['polygons']
                else:
                    segs[t] = seg['counts']
            self.labels.append(lab)
            self._segs.append(segs)
            self._polys.append(polys)
        self._polygon_frames = {t for polys in self._polys for t in polys}
        self._mixed = {t for t in self._polygon_frames if any(t in segs for segs in self._segs)}      # refused when they are read
        self._index = {}
        for t, name in enumerate(self.file_names):
            self._index.setdefault(os.path.splitext(name)[0], t)
        self._events = {}                                            # (annotation, frame) -> validated events

    def __len__(self):
        return self.length

    def frame_names(self):
        """One name per frame: the video's `file_names`, or the frame numbers where it does not name every frame."""
        return self.file_names if len(self.file_names) == len(self) else [str(t) for t in range(len(self))]

    def require_unique_labels(self, who):
        """ValueError, in the name of the tool `who`, for a file that has two tracks with one label: a label map cannot hold them."""
        if len(set(self.labels)) != len(self.labels):
            raise ValueError(f'{who}: two tracks share a label')

    def _frame(self, t):
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not (0 <= t < self.length):
            raise IndexError(f'frame {t!r} is not a frame of these tracks (0..{self.length - 1})')
        return int(t)

    def has_mask(self, t):
        """True when any track has an entry for frame t."""
        t = self._frame(t)
        return t in self._polygon_frames or any(t in segs for segs in self._segs)

    def has_polygons(self, t=None):
        """True when frame t - without t: any frame - is read from polygon-only entries."""
        return bool(self._polygon_frames) if t is None else self._frame(t) in self._polygon_frames

    def _unmixed(self, t):
        if t in self._mixed:
            raise ValueError(f'TrackReader: frame {t} mixes polygon-only entries with counts entries; the two forms are not layered')
        return t

    def polygon_rows(self, t):
        """(rows, values) of a polygon frame for `polygons.fill_rows_host` / `ops.fill_polygons`: the `ring_rows` of every annotation;
        `values` holds every row's annotation (0-based), so a later annotation wins where tracks overlap, as with counts."""
        t = self._unmixed(self._frame(t))
        rows, owner = [], []
        for a, polys in enumerate(self._polys):
            rings = polys.get(t)
            if rings is None:
                continue
            for row in ring_rows(rings, self.fill):
                rows.append(row)
                owner.append(a)
        return rows, owner

    def frame_index(self, name_or_stem):
        """The index of the frame whose file name, or file name without extension, is given; None when there is none."""
        name = str(name_or_stem)
        if name in self.file_names:
            return self.file_names.index(name)
        return self._index.get(name, self._index.get(os.path.splitext(name)[0]))

    def mask_host(self, t):
        """uint8 [H, W] holding the annotations' labels, as `read_tracks` gives it; None for a frame without any entry."""
        t = self._unmixed(self._frame(t))
        if t in self._polygon_frames:
            from .polygons import fill_rows_host
            rows, owner = self.polygon_rows(t)
            return fill_rows_host(rows, self.height, self.width, values=[self.labels[a] for a in owner])
        mask = None
        for lab, segs in zip(self.labels, self._segs):
            if t in segs:
                if mask is None:
                    mask = np.zeros((self.height, self.width), np.uint8)
                mask[decode(segs[t], self.height, self.width)] = lab
        return mask

    def record(self, t):
        """(meta int32 [n, META], packed uint32 events) of frame t with one row per annotation, in the layout `ops.rle_encode`
        writes; of `meta` only field 0, the number of events, is filled."""
        t = self._unmixed(self._frame(t))
        if t in self._polygon_frames:
            raise ValueError(f'TrackReader: frame {t} holds polygons, not counts: it has no record (`masks_device` fills it)')
        meta = np.zeros((len(self.labels), META), np.int32)
        ev = []
        for a, segs in enumerate(self._segs):
            if t in segs:
                if (a, t) not in self._events:
                    self._events[(a, t)] = events_from_counts(segs[t], self.height, self.width)
                ev.append(self._events[(a, t)])
                meta[a, 0] = len(ev[-1])
        return meta, np.concatenate(ev) if ev else np.zeros(0, np.uint32)

    def masks_device(self, frames=None, device=None, values='label', batch=32):
        """(uint8 [n, H, W] on the device, present bool [n]) of `frames` (default: all), decoded in launches of `batch` frames.
        values='label': the annotations' labels; 'dense': 1..n in file order; or a list of one value in 0..255 per annotation.  A
        frame without any entry is all zero, not present.  Frames of polygon-only entries are filled by `ops.fill_polygons`."""
        import torch
        if isinstance(values, str):
            if values not in ('label', 'dense'):
                raise ValueError(f"values must be 'label', 'dense' or a list of one value per track, got {values!r}")
            per_track = list(self.labels) if values == 'label' else list(range(1, len(self.labels) + 1))
        else:
            per_track = [int(v) for v in values]
            if len(per_track) != len(self.labels) or any(not 0 <= v <= 255 for v in per_track):
                raise ValueError(f'values must be {len(self.labels)} integers in 0..255')
        frames = [self._unmixed(self._frame(t)) for t in (range(self.length) if frames is None else frames)]
        n_rows = len(self.labels)
        if n_rows > 254:
            raise ValueError(f'masks_device: {n_rows} tracks, at most 254 fit a launch')
        if not torch.cuda.is_available():
            raise RuntimeError('TrackReader.masks_device needs an MI355X (HIP) device - there is no CPU path')
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        present = np.array([self.has_mask(t) for t in frames], bool)
        out = torch.zeros((len(frames), self.height, self.width), dtype=torch.uint8, device=device)
        if n_rows == 0 or not frames:
            return out, present
        table = None if values == 'dense' else torch.tensor(per_track, dtype=torch.uint8, device=device)
        step = max(1, int(batch))
        with torch.cuda.device(device):
            for i in range(0, len(frames), step):
                chunk, dst = frames[i:i + step], out[i:i + step]
                comp = [j for j, t in enumerate(chunk) if self._all_compressed(t)]
                poly = [j for j, t in enumerate(chunk) if t in self._polygon_frames]
                plain = [j for j in range(len(chunk)) if j not in set(comp) | set(poly)]
                groups = ((plain, self._decode_lists, table), (comp, self._decode_strings, table), (poly, self._fill_polygons, per_track))
                for idx, decode_group, row_values in groups:
                    if not idx:
                        continue
                    whole = len(idx) == len(chunk)
                    got = decode_group([chunk[j] for j in idx], row_values, dst if whole else None)
                    if not whole:                                    # a batch that mixes both forms: each group lands in its frames
                        dst[torch.tensor(idx, device=device)] = got
        return out, present

    def _all_compressed(self, t):
        """True when frame t has an entry and every entry's counts are a string: the frame is decoded by `ops.rle_decompress`."""
        forms = [is_compressed(segs[t]) for segs in self._segs if t in segs]
        return bool(forms) and all(forms)

    def all_compressed(self):
        """True when the file has an entry with counts and all of them are strings: what is rewritten from it keeps that form."""
        forms = [is_compressed(c) for segs in self._segs for c in segs.values()]
        return bool(forms) and all(forms)

    def _decode_lists(self, frames, table, out):
        from . import ops
        records = [self.record(t) for t in frames]
        return ops.rle_decode((np.stack([m for m, _ in records]), [e for _, e in records]), self.height, self.width, len(self.labels),
                              values=table, out=out)

    def _decode_strings(self, frames, table, out):
        """The strings go up as they are - one byte buffer and an offsets table - and become the record on the device."""
        from . import ops
        n_rows = len(self.labels)
        record, status = ops.rle_decompress([[segs.get(t) for segs in self._segs] for t in frames], self.height, self.width, n_rows,
                                            check=False)
        bad = status.cpu().numpy().reshape(len(frames), n_rows)
        if bad.any():
            j, a = (int(v) for v in np.argwhere(bad)[0])
            raise ValueError(f'TrackReader: track {a + 1}, frame {frames[j]}: ' + STRING_STATUS[int(bad[j, a])])
        capacity = record.numel() // len(frames) - n_rows * META
        return ops.rle_decode(record, self.height, self.width, n_rows, capacity, values=table, out=out)

    def _fill_polygons(self, frames, per_track, out):
        """One `ops.fill_polygons` for the frames, every annotation owning a fixed run of rows (`pack_rows`); the host packs per vertex."""
        from . import ops
        rows, values = pack_rows([[polys.get(t) for t in frames] for polys in self._polys], per_track, self.fill)
        return ops.fill_polygons(rows, self.height, self.width, values=values, out=out)


# what `ops.rle_decompress` says about a row (include/xmem_hip.h, xmem_rle_decompress)
STRING_STATUS = {1: 'the compressed counts are malformed', 2: 'the counts do not describe a plane of the video\'s size',
                 3: 'the events of the frame do not fit the capacity'}


def _load_doc(tracks):
    """A tracks file, or a parsed document, -> a document that is the caller's to change."""
    if isinstance(tracks, dict):
        return json.loads(json.dumps(tracks))                        # a deep copy that keeps the order of the keys
    return read_json(tracks)


def recode_tracks(doc, counts):
    """A parsed tracks document with every entry's counts in the form `counts` ('list' | 'compressed'), by the host definitions, per
    count; everything else - and an entry that already has the form - is kept as it is."""
    check_count_form(counts)
    doc = _load_doc(doc)
    for ann in doc.get('annotations', []):
        for seg in ann.get('segmentations', []):
            if seg is None or 'counts' not in seg:                   # a polygon-only entry has nothing to recode
                continue
            have = seg['counts']
            if counts == 'compressed' and not is_compressed(have):
                seg['counts'] = compress_counts(have)
            elif counts == 'list' and is_compressed(have):
                seg['counts'] = decompress_counts(have)
    return doc


def _tracks_to_pngs_on_device(tracks, out_dir, palette_from, empty_frames, batch=32):
    """`tracks_to_pngs` with the masks decoded and the PNGs built on the device (`TrackReader.masks_device`, `ops.png_encode`): no mask
    plane reaches the host.  Mode L, or mode P with all 256 entries of the palette, the ones the palette PNG lacks being zeros."""
    import torch
    from . import ops
    reader = TrackReader(tracks)
    mode, table, palette = 'grey', None, None
    if palette_from is not None:
        from PIL import Image
        raw = Image.open(palette_from).convert('P').getpalette() or []
        pal = np.zeros(768, np.uint8)
        pal[:min(len(raw), 768)] = raw[:768]
        device = torch.device('cuda', torch.cuda.current_device())
        mode, table, palette = 'palette', torch.arange(256, device=device).to(torch.uint8), torch.from_numpy(pal.reshape(256, 3)).to(device)
    os.makedirs(out_dir, exist_ok=True)
    names, written = reader.frame_names(), []
    for frames in batches(range(len(reader)), batch):
        dev, present = reader.masks_device(frames, values='label', batch=max(1, int(batch)))
        for t, ok, data in zip(frames, present, ops.png_encode(dev, mode, table, palette)):
            if not ok and not empty_frames:
                continue
            path = os.path.join(out_dir, os.path.splitext(names[t])[0] + '.png')
            with open(path, 'wb') as fh:
                fh.write(data)
            written.append(path)
    return written


def tracks_to_pngs(tracks, out_dir, palette_from=None, empty_frames=True, png_on_device=False):
    """Write every frame of tracks.json as an index PNG `<out_dir>/<frame>.png` whose pixel values are the tracks' labels (mode P with
    the palette of the PNG `palette_from`, else mode L).  A frame without any entry is written all zero (`empty_frames`) or left out.
    `png_on_device`: decode and encode on the device; the files open to the same mode, size and pixels.  Returns the written paths."""
    if png_on_device:
        return _tracks_to_pngs_on_device(tracks, out_dir, palette_from, empty_frames)
    from PIL import Image
    video, masks = read_tracks(tracks)
    palette = None
    if palette_from is not None:
        palette = Image.open(palette_from).convert('P').getpalette()
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for name, m in zip(video['file_names'], masks):
        if m is None:
            if not empty_frames:
                continue
            m = np.zeros((video['height'], video['width']), np.uint8)
        img = Image.fromarray(m)
        if palette is not None:
            img.putpalette(palette)                                  # mode L becomes mode P: the pixel values are the indices
        path = os.path.join(out_dir, os.path.splitext(name)[0] + '.png')
        img.save(path)
        written.append(path)
    return written


def _rewrite_masks(reader, labels, values, op, batch, halo=0):
    """The pass behind the tools that change a file's masks -> document.  Per batch: `reader.masks_device` with the dense `values`
    (row v of the record is `labels[v - 1]`) -> `op`, label maps to label maps on the device -> `ops.rle_encode`; no mask plane
    reaches the host.  The counts are lists, or compressed strings when every entry of the input is one.
    `halo` > 0, for an `op` that looks along time: a batch is decoded with up to `halo` frames of the FILE on either side (fewer at
    the ends of the video) and `op(masks, present, at, n)` returns the new maps of the n frames from index `at` of what it was given."""
    from . import ops
    names, writer = reader.frame_names(), TrackWriter(reader.height, reader.width)
    k, step = len(labels), max(1, int(batch))
    for frames in batches(range(len(reader) if k else 0), step):
        if halo:
            span = list(range(max(0, frames[0] - halo), min(len(reader), frames[-1] + 1 + halo)))
            masks, around = reader.masks_device(span, values=values, batch=len(span))
            at = frames[0] - span[0]
            new, present = op(masks, around, at, len(frames)), around[at:at + len(frames)]
        else:
            masks, present = reader.masks_device(frames, values=values, batch=step)
            new = op(masks)
        meta, events = ops.rle_encode(new, k)
        for j, t in enumerate(frames):                               # without meta the frame has no mask
            writer.add_frame(names[t], meta[j] if present[j] else None, events[j], labels=labels)
    for t in range(len(writer.file_names), len(reader)):             # a file without tracks: its frames, nothing else
        writer.add_frame(names[t])
    for lab in labels:                                               # a track without any entry still has its (empty) row
        writer.open_track(lab)
    doc = writer.to_dict()
    return recode_tracks(doc, 'compressed') if reader.all_compressed() else doc


def clean_tracks(tracks, spec, batch=32):
    """A tracks file (or parsed document) with `ops.clean_masks` applied to every frame -> (document, totals of the four counters),
    by `_rewrite_masks` with dense ids in file order: boxes and areas are the encoder's, of the cleaned masks.  `spec`: what
    `mask_cleanup.parse_cleanup` returns."""
    import torch
    from . import ops
    from .mask_cleanup import STATS
    reader = TrackReader(tracks)
    reader.require_unique_labels('clean_tracks')
    counters = []                                                    # per batch, on the device: read when its record has arrived

    def clean(dense):
        cleaned, stats = ops.clean_masks(dense, **spec)
        counters.append(stats)
        return cleaned
    doc = _rewrite_masks(reader, reader.labels, 'dense', clean, batch)
    totals = sum((stats.sum(0, dtype=torch.int64).cpu() for stats in counters), torch.zeros(len(STATS), dtype=torch.int64))
    return doc, dict(zip(STATS, (int(v) for v in totals.tolist())))


def grow_tracks(tracks, r, batch=32):
    """A tracks file (or parsed document) with `ops.grow_masks` applied to every frame -> document: r > 0 grows every object by r
    pixels into the background, r < 0 shrinks it (`matte.grow_host` has the definition), by `_rewrite_masks`: counts, boxes and
    areas are the encoder's, of the grown masks.  The masks are decoded with dense ids in ascending order of the labels, so that a
    tie between two objects goes to the smaller LABEL as the definition says; the tracks come out in that order."""
    from . import ops
    reader = TrackReader(tracks)
    reader.require_unique_labels('grow_tracks')
    labels = sorted(reader.labels)
    return _rewrite_masks(reader, labels, [labels.index(lab) + 1 for lab in reader.labels], lambda masks: ops.grow_masks(masks, r), batch)


FRAME_SUFFIXES = ('.jpg', '.jpeg', '.png', '.bmp', '.tif', '.tiff', '.webp')


def frame_lumas(frames_dir, height, width, count):
    """`lumas(lo, hi)` -> uint8 [hi - lo, height, width]: `motion.luma_host` of the frames lo .. hi - 1 of a directory of images
    (FRAME_SUFFIXES; other files are ignored), in the order of their names, decoded with Pillow.  ValueError unless the directory
    holds exactly `count` frames, and for a frame of another size."""
    from PIL import Image
    from .motion import luma_host
    names = sorted(f for f in os.listdir(frames_dir) if f.lower().endswith(FRAME_SUFFIXES) and not f.startswith('.'))
    if len(names) != count:
        raise ValueError(f'{frames_dir}: {len(names)} frames, the tracks have {count}')

    def lumas(lo, hi):
        out = np.empty((hi - lo, height, width), np.uint8)
        for t in range(lo, hi):
            rgb = np.asarray(Image.open(os.path.join(frames_dir, names[t])).convert('RGB'), dtype=np.uint8)
            if rgb.shape[:2] != (height, width):
                raise ValueError(f'{names[t]} is {rgb.shape[:2]}, the tracks are {(height, width)}: the motion search runs at the masks\' size')
            out[t - lo] = luma_host(rgb)
        return out
    return lumas


def smooth_tracks(tracks, radius, locked=(), batch=32, motion=None, lumas=None):
    """A tracks file (or parsed document) with every mask replaced by the majority vote over the frames within `radius` of it
    (`temporal.mode_host` has the definition) -> (document, pixels changed per frame), by `_rewrite_masks` with dense ids in file
    order and a halo of `radius` frames round every batch, so that a batch boundary does not show.  `locked`: frame indices that
    vote but stay as they are (the annotated ones); a frame without a mask neither votes nor changes.
    `motion` (True or {'search', 'bias', 'max_sad'}): the motion-compensated vote, `temporal.mode_mc_host`, on the lumas
    `lumas(lo, hi)` -> uint8 [hi - lo, H, W] hands over (`frame_lumas` of a directory of frames, or that directory's path)."""
    import torch
    from . import ops
    from .temporal import MAX_R, frame_flags
    reader = TrackReader(tracks)
    if motion is not None:
        from .motion import parse_motion
        motion = parse_motion(motion, 'smooth_tracks: motion')
        if lumas is None:
            raise ValueError('smooth_tracks: motion needs the frames (lumas)')
        if isinstance(lumas, (str, os.PathLike)):
            lumas = frame_lumas(lumas, reader.height, reader.width, len(reader))
    reader.require_unique_labels('smooth_tracks')
    locked = sorted({int(t) for t in locked})
    if locked and not 0 <= locked[0] <= locked[-1] < len(reader):
        raise ValueError(f'smooth_tracks: locked frames {locked} outside 0..{len(reader) - 1}')
    radius = ops._int_arg('smooth_tracks', 'radius', radius, 1, MAX_R)
    is_locked = np.zeros(len(reader), bool)
    is_locked[locked] = True
    counters, first = [], []                                         # per batch, on the device: read when its record has arrived

    def vote(masks, present, at, n):
        start = sum(m for _, m in first)                             # the frame the batch starts at: batches come in order
        first.append((start, n))
        flags = torch.from_numpy(frame_flags(len(present), present, is_locked[start - at:start - at + len(present)])).to(masks.device)
        if motion is None:
            out, changed = ops.temporal_mode_ring(masks, len(present), at, n, radius, flags)
        else:
            luma = torch.from_numpy(lumas(start - at, start - at + len(present))).to(masks.device)
            out, changed = ops.temporal_mode_mc_ring(masks, luma, len(present), at, n, radius, flags, **motion)
        counters.append(changed)
        return out
    doc = _rewrite_masks(reader, reader.labels, 'dense', vote, batch, halo=radius)
    changed = [0] * len(reader)
    for (start, n), c in zip(first, counters):
        changed[start:start + n] = [int(v) for v in c.cpu().tolist()]
    return doc, changed


def polygon_tracks(tracks, spec=True, batch=32):
    """A tracks file (or parsed document) with the `polygons` key added to every entry (replaced where there was one) -> document.
    Per batch: `TrackReader.masks_device` (dense ids, one per track) -> `ops.mask_polygons`; no mask plane reaches the host.
    Everything else in the file - counts, boxes, areas, the order of the keys - is kept.  `spec`: config['tracks_polygons'].
    The frames are decoded as label maps, so where two tracks overlap the later one owns the pixels (as in `read_tracks`); the
    files this project writes have no overlap."""
    from . import ops
    from . import polygons as poly
    spec = poly.parse_polygons(spec)
    if spec is None:
        raise ValueError('polygon_tracks: the option is off')
    doc = _load_doc(tracks)
    reader = TrackReader(doc)
    reader.require_unique_labels('polygon_tracks')
    k, step = len(reader.labels), max(1, int(batch))
    for frames in batches(range(len(reader) if k else 0), step):
        dense, _ = reader.masks_device(frames, values='dense', batch=step)
        meta, words = ops.mask_polygons(dense, k)
        for j, t in enumerate(frames):
            for ann, rings in zip(doc['annotations'], poly.label_flat(meta[j], words[j], spec['tolerance'])):
                seg = ann['segmentations'][t]
                if seg is not None:
                    seg['polygons'] = rings
    doc['videos'][0]['polygons'] = {'tolerance': spec['tolerance'], 'fill': 'evenodd'}
    return doc


def verify_polygons(tracks, batch=32):
    """Do the `polygons` of a tracks file (or parsed document) describe its `counts`?  For the entries that have both keys, per
    batch: the polygons are filled (`ops.fill_polygons`, one dense id per track, by the file's fill rule) and the counts decoded
    (`TrackReader.masks_device`), both on the device, and scored with the J&F count kernel (`ops.jf_counts`); only the counts table
    reaches the host.  Returns {'tolerance': what the file says, 'tracks': [{'id', 'label', 'frames', 'differ', 'min_iou',
    'mean_iou'}], 'frames': compared, 'differ': frames in which any track differs}: the measurement of what a tolerance costs.
    Both sides are label maps, so where two tracks overlap the later one owns the pixels on either side."""
    import torch
    from . import ops
    doc = _load_doc(tracks)
    reader = TrackReader(doc)
    anns, k, step = doc['annotations'], len(reader.labels), max(1, int(batch))
    if k > 254:
        raise ValueError(f'verify_polygons: {k} tracks, at most 254 fit a launch')
    both = [[t for t, seg in enumerate(ann['segmentations']) if seg is not None and 'counts' in seg and 'polygons' in seg] for ann in anns]
    todo = sorted({t for ts in both for t in ts})
    ious = [[] for _ in anns]
    bad_frames = set()
    for frames in batches(todo, step):
        want, _ = reader.masks_device(frames, values='dense', batch=step)
        rows, values = pack_rows([[ann['segmentations'][t]['polygons'] if t in both[a] else None for t in frames] for a, ann in enumerate(anns)],
                                 range(1, k + 1), reader.fill, least=1)
        got = ops.fill_polygons(rows, reader.height, reader.width, values=values)
        counts = ops.jf_counts(want, got, 0)[:, 1:k + 1, :3].cpu().numpy().astype(np.int64)      # gt_area, pred_area, inter
        for j, t in enumerate(frames):
            for a in range(k):
                if t in both[a]:
                    g, p, n = (int(v) for v in counts[j, a])
                    ious[a].append(1.0 if g + p - n == 0 else n / (g + p - n))
                    if not (g == p == n):
                        bad_frames.add(t)
    tracks_out = []
    for ann, lab, v in zip(anns, reader.labels, ious):
        tracks_out.append({'id': ann.get('id'), 'label': lab, 'frames': len(v), 'differ': sum(x < 1.0 for x in v),
                           'min_iou': min(v) if v else None, 'mean_iou': float(np.mean(v)) if v else None})
    tolerance = (doc['videos'][0].get('polygons') or {}).get('tolerance')
    return {'tolerance': tolerance, 'fill': reader.fill, 'tracks': tracks_out, 'frames': len(todo), 'differ': len(bad_frames)}


def counts_from_polygons(tracks, batch=32):
    """A tracks file (or parsed document) with `counts` (lists), `size`, `bboxes` and `areas` written for every polygon-only entry ->
    document.  Per batch: `TrackReader.masks_device` (dense ids; the polygon frames are filled by `ops.fill_polygons`) ->
    `ops.rle_encode`; no mask plane reaches the host.  The `polygons` key and everything else is kept.  The frames are label maps, so
    where two tracks overlap the later one owns the pixels."""
    from . import ops
    doc = _load_doc(tracks)
    reader = TrackReader(doc)
    reader.require_unique_labels('counts_from_polygons')
    h, w, k, step = reader.height, reader.width, len(reader.labels), max(1, int(batch))
    for ann in doc['annotations']:
        for key in ('bboxes', 'areas'):
            if ann.get(key) is None:
                ann[key] = [None] * len(reader)
    for frames in batches([t for t in range(len(reader)) if reader.has_polygons(t)], step):
        dense, _ = reader.masks_device(frames, values='dense', batch=step)
        meta, events = ops.rle_encode(dense, k)
        for j, t in enumerate(frames):
            for ann, row, ev in zip(doc['annotations'], meta[j], label_events(meta[j], events[j])):
                seg = ann['segmentations'][t]
                if seg is None:
                    continue
                ann['segmentations'][t] = dict({'size': [h, w], 'counts': counts_from_events(ev, h, w)},
                                               **{key: v for key, v in seg.items() if key not in ('size', 'counts')})
                ann['bboxes'][t] = box_xywh(row) if int(row[1]) else [0, 0, 0, 0]
                ann['areas'][t] = int(row[1])
    return doc


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m xmem2_amd.rle',
                                 description='tracks.json -> index PNGs (one per frame), or - with --recode, --clean, --grow and / or --polygons - '
                                             'tracks.json with its counts in the other form, its masks cleaned, grown or shrunk on the device and / or '
                                             'their polygon outlines added')
    ap.add_argument('--tracks', default=None, help='the tracks.json of one video (counts as lists, compressed strings, or both; '
                                                   'entries may hold polygons alone)')
    ap.add_argument('--out', default=None, help='directory the PNGs are written to; with --recode, --clean, --grow, --polygons, --from-polygons '
                                                'or --from-labelme the file that is written')
    ap.add_argument('--verify-polygons', action='store_true',
                    help='write nothing: fill the polygons of every entry that has both keys and compare them with its counts, on the '
                         'device (needs the GPU); prints per track the minimum and mean IoU and the frames that differ, exit status 1 '
                         'when the file says tolerance 0 and a frame differs')
    ap.add_argument('--from-polygons', action='store_true',
                    help='write no PNGs: rewrite the file with counts, boxes and areas for every polygon-only entry, filled and encoded '
                         'on the device (needs the GPU); the count form is a list unless --recode names one')
    ap.add_argument('--from-labelme', default=None, metavar='DIR',
                    help='in place of --tracks: a directory of labelme per-frame JSON files; writes the polygon-only tracks file --out')
    ap.add_argument('--recode', default=None, choices=COUNT_FORMS,
                    help='write no PNGs: rewrite the file with every counts entry as a list or as the compressed COCO string')
    ap.add_argument('--clean', default=None, metavar='JSON',
                    help='write no PNGs: rewrite the file with every mask cleaned, e.g. \'{"min_area": 16, "max_hole": 16}\' '
                         '(keys min_area, max_hole, keep_largest; needs the GPU); the count form is kept unless --recode names one')
    ap.add_argument('--grow', default=None, type=float, metavar='R',
                    help='write no PNGs: rewrite the file with every object grown by R pixels into the background, or shrunk by -R '
                         '(1 <= |R| <= 127; needs the GPU); after --clean when both are given; counts, boxes and areas are those of '
                         'the new masks')
    ap.add_argument('--polygons', nargs='?', const=0.0, default=None, type=float, metavar='TOL',
                    help='write no PNGs: rewrite the file with the polygon outlines of every entry added (key "polygons"), traced on '
                         'the device (needs the GPU); TOL > 0 simplifies every ring (Ramer-Douglas-Peucker, lossy)')
    ap.add_argument('--smooth', default=None, type=int, metavar='R',
                    help='write no PNGs: rewrite the file with every mask replaced by the majority vote over the frames within R of it '
                         '(1 <= R <= 7; needs the GPU); a step of its own, not to be combined with the others')
    ap.add_argument('--lock', default=None, metavar='FRAMES',
                    help='with --smooth: frame indices, e.g. 0,17,40, that vote but are written as they are (the annotated frames)')
    ap.add_argument('--motion', default=None, metavar='FRAMES_DIR',
                    help='with --smooth: the motion-compensated vote; the directory of the video\'s frames, in frame order by name and of '
                         'the tracks\' size')
    ap.add_argument('--motion-search', default=None, type=int, metavar='S', help='with --motion: the search range in pixels (1..32, default 16)')
    ap.add_argument('--palette-from', default=None, help='a palette PNG (an annotation) whose palette the written PNGs take')
    ap.add_argument('--skip-empty', action='store_true', help='write no file for a frame without any track entry')
    ap.add_argument('--png-on-device', action='store_true', help='with --out DIR: decode the masks and build the PNG files on the device')
    args = ap.parse_args(argv)
    if args.polygons is not None and not (0 <= args.polygons < float('inf')):
        ap.error('--polygons: the tolerance must be a finite number >= 0')
    if (args.tracks is None) == (args.from_labelme is None):
        ap.error('exactly one of --tracks and --from-labelme is needed')
    if args.out is None and not args.verify_polygons:
        ap.error('--out is needed')
    if args.grow is not None and not 1 <= abs(args.grow) <= 127:
        ap.error('--grow: 1 <= |R| <= 127 is needed')
    if args.from_labelme is not None and (args.verify_polygons or args.from_polygons or args.clean or args.recode or args.polygons is not None
                                          or args.grow is not None):
        ap.error('--from-labelme writes the polygon-only file and nothing else: run the other steps on that file')
    if args.smooth is not None:
        from .temporal import MAX_R
        if not 1 <= args.smooth <= MAX_R:
            ap.error(f'--smooth: 1 <= R <= {MAX_R} is needed')
        if (args.verify_polygons or args.from_polygons or args.from_labelme is not None or args.clean or args.recode
                or args.polygons is not None or args.grow is not None):
            ap.error('--smooth is a step of its own: run --clean, --grow, --polygons, --recode and the polygon steps on the file it writes')
    if args.motion is not None and args.smooth is None:
        ap.error('--motion goes with --smooth')
    if args.motion_search is not None:
        from .motion import MAX_SEARCH
        if args.motion is None:
            ap.error('--motion-search goes with --motion')
        if not 1 <= args.motion_search <= MAX_SEARCH:
            ap.error(f'--motion-search: 1 <= S <= {MAX_SEARCH} is needed')
    if args.lock is not None:
        if args.smooth is None:
            ap.error('--lock goes with --smooth')
        try:
            args.lock = [int(v) for v in args.lock.split(',') if v.strip()]
        except ValueError:
            ap.error('--lock: frame indices separated by commas are needed, e.g. 0,17,40')
    if args.clean is not None:
        from .mask_cleanup import parse_cleanup
        try:
            args.clean = parse_cleanup(json.loads(args.clean))
        except ValueError as e:                                      # JSONDecodeError is one
            ap.error(f'--clean: {e}')
        if args.clean is None:
            ap.error('--clean: the options given change nothing')
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.verify_polygons:
        report = verify_polygons(args.tracks)
        print(json.dumps(report))
        return 1 if report['tolerance'] == 0 and report['differ'] else 0
    if args.from_labelme is not None:
        from .polygons import from_labelme
        doc = from_labelme(args.from_labelme)
        text = write_json(doc, args.out)
        print(json.dumps({'frames': doc['videos'][0]['length'], 'tracks': len(doc['annotations']), 'bytes': len(text), 'out': args.out}))
        return 0
    if args.smooth is not None:
        motion = None if args.motion is None else ({} if args.motion_search is None else {'search': args.motion_search})
        doc, changed = smooth_tracks(args.tracks, args.smooth, locked=args.lock or (), **({} if motion is None else
                                                                                       {'motion': motion, 'lumas': args.motion}))
        report = {'smooth': args.smooth, 'pixels_changed': sum(changed), 'frames_changed': sum(1 for c in changed if c)}
        if motion is not None:
            from .motion import parse_motion
            report['motion'] = parse_motion(motion, '--motion')
        print(json.dumps(dict(report, bytes=len(write_json(doc, args.out)), out=args.out)))
        return 0
    if args.recode is not None or args.clean is not None or args.polygons is not None or args.from_polygons or args.grow is not None:
        doc, report = _load_doc(args.tracks), {}
        if args.from_polygons:                                       # first: what follows reads counts
            doc = counts_from_polygons(doc)
            report['from_polygons'] = True
        if args.clean is not None:
            doc, report['clean'] = clean_tracks(doc, args.clean)
        if args.grow is not None:                                    # of the cleaned masks, when both are asked for
            doc = grow_tracks(doc, args.grow)
            report['grow'] = args.grow
        if args.polygons is not None:                                # of the cleaned masks, when both are asked for
            doc = polygon_tracks(doc, {'tolerance': args.polygons})
            report['polygons'] = doc['videos'][0]['polygons']
        if args.recode is not None:
            doc = recode_tracks(doc, args.recode)
            report['recode'] = args.recode
        print(json.dumps(dict(report, bytes=len(write_json(doc, args.out)), out=args.out)))
        return 0
    written = tracks_to_pngs(args.tracks, args.out, args.palette_from, empty_frames=not args.skip_empty, png_on_device=args.png_on_device)
    print(json.dumps({'frames': len(written), 'out': args.out}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
