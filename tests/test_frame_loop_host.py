"""The frame loop of run_on_video / run_on_video_ensemble without a GPU: `_run_frame_loop` and `_FrameOutputs` driven with fakes (a
list-backed decoder, a fetcher and a track loop with AsyncMaskFetcher's depth rule, a saver that runs its jobs at once, recording
hint / prepare / frame callbacks) on frames of 16 x 32.  What is asserted follows from the loop's rules, not from a run of it:
which frames are hinted when, masks delivered behind the device and the rest by the drain, the tracks-only path that copies no
mask, what the saver is handed, and that an error still closes the decoder and the saver."""
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
        self.log.append((self.name + '.submit', tag[0].frame if isinstance(tag[0], rov.Sample) else tag[0][0].frame))
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


class _Tracks:
    """_TrackLoop's surface: the record travels through a fetcher of its own, tagged (tag, mask, k, capacity)."""

    def __init__(self, log):
        self.fetcher, self.finished, self.written = _Fetcher(log, 'tracks'), [], []

    def submit(self, tag, mask_dev, k):
        return self.fetcher.submit((tag, mask_dev, k, 2048), torch.zeros(4, dtype=torch.uint8))

    def drain(self):
        return self.fetcher.drain()

    def finish(self, item, name, mapper):
        assert item[0][0][0].frame == name
        self.finished.append(name)

    def write(self, path):
        self.written.append(path)


class _Saver:
    def __init__(self, log):
        self.log, self.files, self.closed = log, [], False

    def submit(self, job):
        files = [(sub, name, img.size) for img, sub, name in job()]
        self.log.append(('finish', files[0][1][:-4] + '.jpg'))
        self.files.append(files)

    def close(self):
        self.closed = True


class _Reader:
    @staticmethod
    def map_the_colors_back(pil):
        return pil.convert('RGB')


class _Mapper:
    labels = [1]

    @staticmethod
    def remap_index_mask(m):
        return m


def _run(n, key_batch, *, masks=None, given=(0,), saver=False, tracks=False, compute_iou=False, save_overlay=True,
         out_masks=None):
    """One run of the loop on n fake frames -> everything the assertions read."""
    log = []
    samples = [_sample(t, (masks or {}).get(t)) for t in range(n)]
    decoder, fetcher = _Decoder(samples, log), _Fetcher(log, 'mask')
    outputs = rov._FrameOutputs(_Reader(), _Mapper(), fetcher, saver=_Saver(log) if saver else None, tracks=_Tracks(log) if tracks else None,
                                compute_iou=compute_iou, save_overlay=save_overlay, masks_out_path='out')

    def hint(smps):
        log.append(('hint', [int(s.frame[:4]) for s in smps]))
        return [('input', s.frame) for s in smps]

    def prepare(ti, sample):
        return 'annotation' if ti in given else None

    def frame(ti, sample, inputs, prepared):
        log.append(('frame', ti, sample.frame, inputs, prepared, len(outputs.stats)))
        out = (out_masks or {}).get(ti, np.zeros((H, W), np.uint8))
        return prepared is not None, torch.from_numpy(out)

    times = rov._run_frame_loop(n, key_batch, decoder, outputs, hint, prepare, frame)
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
        out = rov._FrameOutputs(_Reader(), _Mapper(), fetcher, saver=_Saver(log), tracks=tracks, reused_output=reused)
        out.submit(0, _sample(0), False, buf)
        assert fetcher.submitted[0] is buf
        if tracks is not None:
            assert (tracks.fetcher.pending[0][0][1] is buf) == (not reused)


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
    outputs = rov._FrameOutputs(_Reader(), _Mapper(), _Fetcher(log, 'mask'), saver=saver)

    def frame(ti, sample, inputs, prepared):
        if ti == 2:
            raise ZeroDivisionError('frame failed')
        return False, torch.zeros((H, W), dtype=torch.uint8)

    with pytest.raises(ZeroDivisionError, match='frame failed'):
        rov._run_frame_loop(6, 4, decoder, outputs, lambda smps: [None] * len(smps), lambda ti, sample: None, frame)
    assert decoder.closed and saver.closed
