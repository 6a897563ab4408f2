"""The frame loop of run_on_video / run_on_video_ensemble without a GPU: `_run_frame_loop` and `_FrameOutputs` driven with fakes (a
list-backed decoder, a fetcher and a track loop with AsyncMaskFetcher's depth rule, a saver that runs its jobs at once, recording
hint / prepare / frame callbacks) on frames of 16 x 32.  What is asserted follows from the loop's rules, not from a run of it:
which frames are hinted when, masks delivered behind the device and the rest by the drain, the tracks-only path that copies no
mask, what the saver is handed, and that an error still closes the decoder and the saver.  With every side output on (recording
fakes for the tracks, the mattes, the device's PNGs, the scorer and a confidence object): the order a frame is fed in, that a frame
arrives after its side records were finished, who gets a copy of a tensor the caller rewrites, and the drain and close order."""
from dataclasses import replace

import numpy as np
import pytest
import torch
from PIL import Image

from xmem2_amd import run_on_video as rov

H, W, DEPTH = 16, 32, 3


def _sample(t, mask=None):
    return rov.Sample(rgb_u8=torch.full((H, W, 3), t, dtype=torch.uint8), raw_image_pil=Image.new('RGB', (W, H), (t, t, t)),
                      frame=f'{t:04d}.jpg', save=True, shape=(H, W), need_resize=False, mask=mask)


class _Decoder:
    def __init__(self, samples, log):
        self.samples, self.log, self.closed = list(samples), log, False

    def get(self, n):
        out, self.samples = self.samples[:n], self.samples[n:]
        assert len(out) == n, 'the loop asked for more frames than the video has'
        return out

    def close(self):
        self.closed = True
        self.log.append(('decoder.close',))


class _Fetcher:
    """AsyncMaskFetcher's delivery rule without a device: an entry is handed back once DEPTH are pending."""

    def __init__(self, log, name):
        self.log, self.name, self.pending, self.submitted = log, name, [], []

    def submit(self, tag, mask):
        self.log.append((self.name + '.submit', tag.frame))
        self.submitted.append(mask)
        self.pending.append((tag, mask.numpy().copy()))
        ready = []
        while len(self.pending) >= DEPTH:
            ready.append(self.pending.pop(0))
        return ready

    def drain(self):
        self.log.append((self.name + '.drain',))
        out, self.pending = self.pending, []
        return out


def _frame_of(item):
    """the frame name of a side channel's arrived (tag, record) pair"""
    return item[0].frame


class _Side:
    """What the side channels have in common: the record travels through a fetcher of their own, and `finish` notes how many stats
    rows there were when the frame's record was finished."""
    rereads, every_frame = False, True

    def __init__(self, log, name):
        self.name, self.log, self.fetcher, self.finished, self.rows, self.fed = name, log, _Fetcher(log, name), [], (lambda: 0), []

    def _feed(self, tag, mask_dev):
        self.fed.append(mask_dev)
        return self.fetcher.submit(replace(tag, dev=(mask_dev,), room=(2048,)), torch.zeros(4, dtype=torch.uint8))

    def drain(self):
        return self.fetcher.drain()

    def _finish(self, item):
        self.finished.append(_frame_of(item))
        self.log.append((self.name + '.finish', _frame_of(item), self.rows()))


class _Tracks(_Side):
    """_TrackLoop's surface."""
    rereads = True

    def __init__(self, log):
        super().__init__(log, 'tracks')
        self.written, self.writer = [], self

    def submit(self, tag, mask_dev, mapper):
        return self._feed(tag, mask_dev)

    def finish(self, item, mapper):
        self._finish(item)

    def close(self):
        pass

    def set_confidence(self, entries):
        self.log.append(('tracks.set_confidence', entries))

    def write(self, path):
        self.log.append(('tracks.write', path))
        self.written.append(path)


class _Mattes(_Side):
    """_MatteLoop's surface, with writers of its own to close."""
    every_frame = False

    def __init__(self, log, close_error=None):
        super().__init__(log, 'mattes')
        self.close_error = close_error

    def submit(self, tag, mask_dev, mapper):
        return self._feed(tag, mask_dev)

    def finish(self, item, mapper):
        self._finish(item)

    def close(self):
        self.log.append(('mattes.close',))
        if self.close_error is not None:
            raise self.close_error


class _Pngs(_Side):
    """_PngLoop's surface: a finished frame is the bytes of its file."""
    rereads = True

    def __init__(self, log):
        super().__init__(log, 'pngs')
        self.files = {}

    def submit(self, tag, mask_dev, mapper):
        return self._feed(tag, mask_dev)

    def finish(self, item, mapper):
        self._finish(item)
        self.files[_frame_of(item)] = b'png of ' + _frame_of(item).encode()

    def close(self):
        pass


class _Confidence:
    """What the output side asks of a FrameConfidence: drained and closed with the loop, the tracks' scores at the end."""

    def __init__(self, log, close_error=None):
        self.log, self.close_error = log, close_error

    def drain(self):
        self.log.append(('confidence.drain',))

    def close(self):
        self.log.append(('confidence.close',))
        if self.close_error is not None:
            raise self.close_error

    def track_entries(self, mapper):
        return 'entries'


class _Scorer:
    def __init__(self, log):
        self.log = log

    def add(self, ti, gt, out_dev, mapper):
        self.log.append(('scorer.add', f'{ti:04d}.jpg'))


class _Saver:
    def __init__(self, log):
        self.log, self.files, self.closed = log, [], False

    def submit(self, job):
        files = [(sub, name, getattr(img, 'size', img)) for img, sub, name in job()]      # finished files: their bytes
        self.log.append(('finish', files[0][1][:-4] + '.jpg'))
        self.files.append(files)

    def close(self):
        self.closed = True
        self.log.append(('saver.close',))


class _Reader:
    @staticmethod
    def map_the_colors_back(pil):
        return pil.convert('RGB')


class _Mapper:
    labels = [1]

    @staticmethod
    def remap_index_mask(m):
        return m


def _vote(ring, T, t0, n, radius, flags, changed=None):
    """a delay line's vote that hands every frame on as it came"""
    return ring[t0 % ring.shape[0]][None], changed


def _outputs(log, n=None, *, fetcher=None, saver=False, tracks=False, mattes=False, pngs=False, conf=None, scorer=False, delay=False, **kw):
    """-> (the _FrameOutputs, what the loop drives: behind a delay line of one frame with `delay`)"""
    on = lambda made, want: made(log) if want is True else (want or None)
    out = rov._FrameOutputs(_Reader(), _Mapper(), fetcher or _Fetcher(log, 'mask'), saver=on(_Saver, saver), tracks=on(_Tracks, tracks),
                            mattes=on(_Mattes, mattes), pngs=on(_Pngs, pngs), scorer=on(_Scorer, scorer), confidence=conf,
                            masks_out_path='out', **kw)
    for side in (out.tracks, out.mattes, out.pngs):
        if side is not None:
            side.rows = lambda: len(out.stats)
    loop = out
    if delay:
        from xmem2_amd.temporal import DelayLine
        loop = DelayLine(out, {'radius': 1}, n, 'cpu', vote=_vote)
    return out, loop


def _run(n, key_batch, *, masks=None, given=(0,), out_masks=None, log=None, **kw):
    """One run of the loop on n fake frames -> everything the assertions read.  `log`: the list a fake of the caller's writes to."""
    log = [] if log is None else log
    samples = [_sample(t, (masks or {}).get(t)) for t in range(n)]
    decoder, fetcher = _Decoder(samples, log), _Fetcher(log, 'mask')
    outputs, loop = _outputs(log, n, fetcher=fetcher, **kw)

    def hint(smps):
        log.append(('hint', [int(s.frame[:4]) for s in smps]))
        return [('input', s.frame) for s in smps]

    def prepare(ti, sample):
        return 'annotation' if ti in given else None

    def frame(ti, sample, inputs, prepared):
        log.append(('frame', ti, sample.frame, inputs, prepared, len(outputs.stats)))
        out = (out_masks or {}).get(ti, np.zeros((H, W), np.uint8))
        return prepared is not None, torch.from_numpy(out)

    times = rov._run_frame_loop(n, key_batch, decoder, loop, hint, prepare, frame)
    return dict(log=log, outputs=outputs, decoder=decoder, fetcher=fetcher, times=times)


def _first(log, *head):
    return next(i for i, e in enumerate(log) if e[:len(head)] == head)


# ---- 1. which frames are hinted when ---------------------------------------------------------------------------------------
def test_hint_schedule_and_frame_order():
    r = _run(10, 4)
    log = r['log']
    assert [e[1] for e in log if e[0] == 'hint'] == [[0, 1, 2, 3], [4, 5, 6, 7], [8], [9]]
    assert _first(log, 'hint', [4, 5, 6, 7]) < _first(log, 'frame', 1)          # fewer than a batch pending after frame 0
    assert _first(log, 'frame', 0) < _first(log, 'hint', [4, 5, 6, 7])
    assert _first(log, 'frame', 4) < _first(log, 'hint', [8]) < _first(log, 'frame', 5)     # the tail: frame by frame
    assert _first(log, 'frame', 5) < _first(log, 'hint', [9]) < _first(log, 'frame', 6)
    frames = [e for e in log if e[0] == 'frame']
    assert [e[1] for e in frames] == list(range(10))
    for e in frames:                                                             # its own sample, the input its hint returned
        assert e[2] == f'{e[1]:04d}.jpg' and e[3] == ('input', e[2])
        assert e[4] == ('annotation' if e[1] == 0 else None)
    assert len(r['times']) == 3 and all(t >= 0 for t in r['times']) and r['times'][1] <= r['times'][2]

    short = _run(3, 4)
    assert [e[1] for e in short['log'] if e[0] == 'hint'] == [[0], [1], [2]]
    assert [e[1] for e in short['log'] if e[0] == 'frame'] == [0, 1, 2]


# ---- 2. stats rows, one frame behind, the rest by the drain ----------------------------------------------------------------
def test_stats_rows_and_delivery_order():
    left_half, left_quarter = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    left_half[:, :16], left_quarter[:, :8] = 1, 1
    n = 7
    r = _run(n, 4, masks={0: left_half, 3: left_half}, given=(0,), compute_iou=True, saver=True, out_masks={0: left_half, 3: left_quarter})
    stats, log = r['outputs'].stats, r['log']
    assert [s['frame'] for s in stats] == [f'{t:04d}.jpg' for t in range(n)]
    assert all(list(s) == ['frame', 'mask_provided', 'iou'] for s in stats)
    assert [s['mask_provided'] for s in stats] == [True] + [False] * (n - 1)
    assert stats[0]['iou'] == -1                                                 # a given mask is not scored
    assert stats[3]['iou'] == pytest.approx(0.5, abs=1e-6)                       # 128 of the 256 ground-truth pixels
    assert all(stats[t]['iou'] == -1 for t in (1, 2, 4, 5, 6))                   # no ground truth
    for t in range(n - 1):                                                       # never before the next frame is on its way
        assert _first(log, 'frame', t + 1) < _first(log, 'finish', f'{t:04d}.jpg')
    for e in log:
        if e[0] == 'frame':                                                      # rows seen by frame ti: those the depth rule released
            assert e[5] == max(0, e[1] - (DEPTH - 1))
    drain = _first(log, 'mask.drain')
    assert [e[1] for e in log[drain:] if e[0] == 'finish'] == [f'{t:04d}.jpg' for t in range(n - (DEPTH - 1), n)]
    assert drain < _first(log, 'decoder.close')

    plain = _run(4, 4)                                                           # without compute_iou: no iou column
    assert all(list(s) == ['frame', 'mask_provided'] for s in plain['outputs'].stats) and len(plain['outputs'].stats) == 4


# ---- 3. tracks ------------------------------------------------------------------------------------------------------------
def test_tracks_only_copies_no_mask():
    n = 6
    r = _run(n, 4, tracks=True)
    out = r['outputs']
    assert not out.need_mask and r['fetcher'].submitted == [] and not any(e[0].startswith('mask.') for e in r['log'])
    assert [s['frame'] for s in out.stats] == [f'{t:04d}.jpg' for t in range(n)]
    assert out.tracks.finished == [f'{t:04d}.jpg' for t in range(n)] and out.tracks.written == ['out']


def test_tracks_and_saver_are_both_fed_tracks_first():
    n = 6
    r = _run(n, 4, tracks=True, saver=True)
    out = r['outputs']
    assert out.need_mask
    submits = [e for e in r['log'] if e[0] in ('tracks.submit', 'mask.submit')]
    assert submits == [(k, f'{t:04d}.jpg') for t in range(n) for k in ('tracks.submit', 'mask.submit')]
    assert out.tracks.finished == [f'{t:04d}.jpg' for t in range(n)] and out.tracks.written == ['out']
    assert len(out.saver.files) == n and len(out.stats) == n
    assert _run(3, 4, tracks=True, compute_iou=True)['outputs'].need_mask        # compute_iou reads the mask on the host too


def test_reused_output_is_copied_for_the_track_loop_only():
    log = []
    buf = torch.zeros((H, W), dtype=torch.uint8)
    for reused, tracks in ((True, _Tracks(log)), (False, _Tracks(log)), (True, None)):
        fetcher = _Fetcher(log, 'mask')
        out, _ = _outputs(log, fetcher=fetcher, saver=True, tracks=tracks, reused_output=reused)
        out.submit(0, _sample(0), False, buf)
        assert fetcher.submitted[0] is buf
        if tracks is not None:
            assert (tracks.fetcher.pending[0][0].dev[0] is buf) == (not reused)


# ---- 4. the saver's files; an error closes what was opened ------------------------------------------------------------------
@pytest.mark.parametrize('save_overlay', [True, False])
def test_saver_files(save_overlay):
    r = _run(5, 4, saver=True, save_overlay=save_overlay)
    want = [[('masks', f'{t:04d}.png', (W, H))] + ([('overlay', f'{t:04d}.jpg', (W, H))] if save_overlay else []) for t in range(5)]
    assert r['outputs'].saver.files == want
    assert r['outputs'].saver.closed and r['decoder'].closed


def test_an_error_in_frame_closes_decoder_and_saver():
    log = []
    decoder, saver = _Decoder([_sample(t) for t in range(6)], log), _Saver(log)
    outputs, _ = _outputs(log, saver=saver)

    def frame(ti, sample, inputs, prepared):
        if ti == 2:
            raise ZeroDivisionError('frame failed')
        return False, torch.zeros((H, W), dtype=torch.uint8)

    with pytest.raises(ZeroDivisionError, match='frame failed'):
        rov._run_frame_loop(6, 4, decoder, outputs, lambda smps: [None] * len(smps), lambda ti, sample: None, frame)
    assert decoder.closed and saver.closed


# ---- 5. every side output at once: feed order, arrival, copies, drain and close order --------------------------------------------------
ALL = dict(saver=True, tracks=True, mattes=True, pngs=True, scorer=True)
GT = {t: np.ones((H, W), np.uint8) for t in range(8)}


def test_feed_order_per_frame():
    n = 5
    log = _run(n, 4, masks=GT, **ALL)['log']
    fed = [e for e in log if e[0] in ('scorer.add', 'tracks.submit', 'mattes.submit', 'pngs.submit', 'mask.submit')]
    assert fed == [(k, f'{t:04d}.jpg') for t in range(n) for k in ('scorer.add', 'tracks.submit', 'mattes.submit', 'pngs.submit', 'mask.submit')]


@pytest.mark.parametrize('delay', [False, True])
def test_a_frame_arrives_after_its_side_records_were_finished(delay):
    n = 7
    r = _run(n, 4, masks=GT, delay=delay, **ALL)
    log, out = r['log'], r['outputs']
    assert [s['frame'] for s in out.stats] == [f'{t:04d}.jpg' for t in range(n)]
    for t in range(n):
        name = f'{t:04d}.jpg'
        for side in ('tracks', 'mattes', 'pngs'):
            done = log[_first(log, side + '.finish', name)]
            assert done[2] <= t, f'{side}: the row of frame {t} was there before its record was finished'
            assert _first(log, side + '.finish', name) < _first(log, 'finish', name)
    for side in (out.tracks, out.mattes, out.pngs):
        assert side.finished == [f'{t:04d}.jpg' for t in range(n)]
    # the mask file is the device's, the overlay is made from the mask that travelled
    assert out.saver.files == [[('masks', f'{t:04d}.png', b'png of ' + f'{t:04d}.jpg'.encode()), ('overlay', f'{t:04d}.jpg', (W, H))]
                               for t in range(n)]


def test_reused_output_is_copied_for_who_may_read_it_again():
    buf = torch.zeros((H, W), dtype=torch.uint8)
    for reused in (True, False):
        log, fetcher = [], _Fetcher([], 'mask')
        out, _ = _outputs(log, fetcher=fetcher, reused_output=reused, **ALL)
        out.submit(0, _sample(0), False, buf)
        assert fetcher.submitted[0] is buf and out.mattes.fed[0] is buf
        for side in (out.tracks, out.pngs):
            assert (side.fed[0] is buf) == (not reused)
            assert torch.equal(side.fed[0], buf)
        assert out.tracks.fed[0] is not out.pngs.fed[0] or not reused


def test_pngs_without_overlays_copy_no_mask():
    n = 6
    r = _run(n, 4, saver=True, pngs=True, save_overlay=False)
    out = r['outputs']
    assert not out.need_mask and r['fetcher'].submitted == [] and not any(e[0].startswith('mask.') for e in r['log'])
    assert [s['frame'] for s in out.stats] == [f'{t:04d}.jpg' for t in range(n)]
    assert out.saver.files == [[('masks', f'{t:04d}.png', b'png of ' + f'{t:04d}.jpg'.encode())] for t in range(n)]
    assert _run(3, 4, saver=True, pngs=True, save_overlay=True)['outputs'].need_mask
    assert _run(3, 4, saver=True, pngs=True, save_overlay=False, compute_iou=True)['outputs'].need_mask
    assert _run(3, 4, saver=True, tracks=True, pngs=True, save_overlay=False)['fetcher'].submitted == []
    assert not _run(3, 4, tracks=True, mattes=True)['outputs'].need_mask     # save_masks=False: the tracks' frames stand in


@pytest.mark.parametrize('delay', [False, True])
def test_the_confidence_planes_are_drained_last_and_closed_first(delay):
    n = 6
    log = []
    r = _run(n, 4, conf=_Confidence(log), log=log, delay=delay, **ALL)
    drains = [e[0] for e in r['log'] if e[0].endswith('.drain')]
    assert sorted(drains[:-1]) == ['mask.drain', 'mattes.drain', 'pngs.drain', 'tracks.drain'] and drains[-1] == 'confidence.drain'
    assert _first(r['log'], 'confidence.drain') < _first(r['log'], 'tracks.set_confidence')
    closes = [e[0] for e in r['log'] if e[0].endswith('.close') and e[0] != 'decoder.close']
    assert closes == ['confidence.close', 'mattes.close', 'saver.close']
    assert _first(r['log'], 'decoder.close') < _first(r['log'], 'confidence.close')


@pytest.mark.parametrize('who', ['confidence', 'mattes'])
def test_an_error_in_an_earlier_close_still_closes_the_saver_and_is_raised(who):
    log, err = [], KeyError('a writer failed')
    conf = _Confidence(log, err if who == 'confidence' else None)
    out, loop = _outputs(log, conf=conf, saver=True, mattes=_Mattes(log, err if who == 'mattes' else None))
    with pytest.raises(KeyError) as caught:
        loop.close()
    assert caught.value is err
    assert [e[0] for e in log] == ['confidence.close', 'mattes.close', 'saver.close'] and out.saver.closed


@pytest.mark.parametrize('delay', [False, True])
def test_the_end_of_the_loop_sets_the_confidence_then_writes_once(delay):
    log = []
    r = _run(5, 4, conf=_Confidence(log), log=log, delay=delay, tracks=True, saver=True)
    tail = [e for e in r['log'] if e[0] in ('tracks.set_confidence', 'tracks.write')]
    assert tail == [('tracks.set_confidence', 'entries'), ('tracks.write', 'out')]
    assert r['outputs'].tracks.finished == [f'{t:04d}.jpg' for t in range(5)]
    assert r['log'].index(tail[0]) > max(i for i, e in enumerate(r['log']) if e[0] == 'tracks.finish')
    plain = _run(5, 4, tracks=True, saver=True)                                  # without the option: written all the same, no scores
    assert [e[0] for e in plain['log'] if e[0].startswith('tracks.') and e[0] not in ('tracks.submit', 'tracks.finish', 'tracks.drain')] == ['tracks.write']
