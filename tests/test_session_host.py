"""VideoSession without a GPU: argument validation, reference bookkeeping on a stub core, the arithmetic of `propagate`'s visit order
and key batches, the 'files' mask table against `_pil_to_tensor01`, the C-ABI surface of the new entry point and the launcher's
network sharing rules."""
import argparse
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a session on stubs --------------------------------------------------------------------------------------------------
class _StubMemory:
    def __init__(self):
        self.saved = []                                      # frame ids in store order

    def frame_already_saved(self, t):
        return t in self.saved


class _StubCore:
    """Records what a session asks of its InferenceCore."""

    def __init__(self):
        self.memory = _StubMemory()
        self.calls = []
        self.labels = None

    def set_all_labels(self, labels):
        self.labels = list(labels)

    def put_to_permanent_memory(self, image, mask, ti=None):
        self.calls.append(('put', ti, tuple(mask.shape)))
        update = ti in self.memory.saved
        if not update:
            self.memory.saved.append(ti)
        return update

    def clear_memory(self, keep_permanent=False):
        self.calls.append(('clear', keep_permanent))


class _StubReader:
    def resize_mask(self, m):
        return m


def _stub_session(n=6, hw=(8, 10), monkeypatch=None):
    from xmem2_amd import session as S
    from xmem2_amd.mask_mapper import MaskMapper
    s = object.__new__(S.VideoSession)
    s.device = torch.device('cpu')
    s.core, s.mapper, s.reader = _StubCore(), MaskMapper(), _StubReader()
    s.shape = hw
    s.frames = []
    for t in range(n):
        f = object.__new__(S._Frame)
        gt = np.zeros(hw, np.uint8); gt[2:5, 1 + t % 3:6] = 1
        f.frame, f.shape, f.need_resize, f.raw_image_pil, f.mask = f'{t:05d}.jpg', hw, False, None, (gt if t != 4 else None)
        s.frames.append(f)
    s.n_device_frames = n
    s._dev_frames = torch.zeros((n,) + hw + (3,), dtype=torch.uint8)
    s._host_frames = None
    s.masks = torch.zeros((n,) + hw, dtype=torch.uint8)
    s._present = [False] * n
    s._refs = {}
    s.key_batch = 4
    if monkeypatch is not None:                              # the removal edits a real store: record it instead
        monkeypatch.setattr(S, '_remove_permanent_frame',
                            lambda core, t, pos: (core.calls.append(('remove', t, pos)), core.memory.saved.remove(t)))
    return s


def test_constructor_validates_its_arguments(tmp_path):
    from xmem2_amd.session import VideoSession
    with pytest.raises(NotADirectoryError):
        VideoSession(str(tmp_path / 'nowhere'))
    (tmp_path / 'imgs').mkdir()
    with pytest.raises(NotADirectoryError):
        VideoSession(str(tmp_path / 'imgs'), str(tmp_path / 'nomasks'))
    with pytest.raises(TypeError):
        VideoSession(str(tmp_path / 'imgs'), None, overwrite_config=[('size', -1)])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            VideoSession(str(tmp_path / 'imgs'))


def test_reference_bookkeeping_on_a_stub_core(monkeypatch):
    s = _stub_session(monkeypatch=monkeypatch)
    assert len(s) == 6 and s.references == [] and not s.all_masks_present() and s.mask(0) is None
    assert s.save_reference(0) is False and s.references == [0]
    assert s.core.calls[-1] == ('put', 0, (1, 8, 10)) and s.core.labels == [1]
    # an index array, a tensor and the replacement of an existing reference
    m = np.zeros((8, 10), np.uint8); m[1:3, 1:3] = 1
    assert s.save_reference(5, m) is False and s.references == [0, 5]
    assert s.save_reference(5, torch.from_numpy(m)) is True and s.references == [0, 5]
    assert s.core.calls[-2:] == [('remove', 5, 1), ('put', 5, (1, 8, 10))]     # a replacement: taken out at its true position, put again
    # a reference in front of existing ones: those are taken out and put again behind it - the store stays in frame order
    s.core.calls.clear()
    assert s.save_reference(3) is False and s.references == [0, 3, 5]
    assert [c[:2] for c in s.core.calls] == [('remove', 5), ('put', 3), ('put', 5)] and s.core.memory.saved == [0, 3, 5]
    assert s.core.calls[0] == ('remove', 5, 1)                # the TRUE position of frame 5 in the store, not the memory's table
    s.remove_reference(3)
    assert s.references == [0, 5] and s.core.memory.saved == [0, 5]
    with pytest.raises(KeyError):
        s.remove_reference(3)
    for bad in (-1, 6, 1.0, True):
        with pytest.raises(IndexError):
            s.save_reference(bad)
    with pytest.raises(FileNotFoundError):
        s.save_reference(4)                                  # no annotation file for frame 4
    with pytest.raises(ValueError, match='shape'):
        s.save_reference(1, np.zeros((4, 4), np.uint8))
    # [K+1, H, W] with one plane is that plane; a second object extends the label list
    two = np.zeros((8, 10), np.uint8); two[0:2] = 1; two[5:7] = 2
    assert s.save_reference(2, torch.from_numpy(two)[None]) is False and s.core.labels == [1, 2]


def test_empty_first_annotation_is_skipped(monkeypatch):
    s = _stub_session(monkeypatch=monkeypatch)
    with pytest.warns(UserWarning, match='empty'):
        assert s.save_reference(0, np.zeros((8, 10), np.uint8)) is False
    assert s.references == [] and s.core.calls == []


def test_candidates_and_propagation_refuse_without_masks_or_references(monkeypatch):
    s = _stub_session(monkeypatch=monkeypatch)
    with pytest.raises(ValueError, match='No valid masks'):
        s.propagate()
    with pytest.raises(ValueError, match='No valid masks'):
        s.full_propagation()
    s.save_reference(0)
    with pytest.raises(RuntimeError, match='Run propagation on all frames first'):
        s.candidates(2)
    s._present = [True] * 5 + [False]
    with pytest.raises(RuntimeError, match='first: 5'):
        s.candidates(2)
    s._present = [True] * 6
    s.remove_reference(0)
    with pytest.raises(RuntimeError, match='at least one reference'):
        s.candidates(2)
    s.save_reference(0)
    for kw in (dict(k=0), dict(alpha=1.5), dict(min_mask_presence_percent=-1), dict(mask_form='probabilities')):
        with pytest.raises(ValueError):
            s.candidates(**{**dict(k=2), **kw})
    assert s.all_masks_present() and torch.equal(s.mask(1), s.masks[1])


def test_visit_order_direction_and_stop():
    from xmem2_amd.session import visit_order
    assert visit_order(5) == [0, 1, 2, 3, 4]
    assert visit_order(5, 2) == [2, 3, 4]
    assert visit_order(5, 1, 'forward', 3) == [1, 2, 3]
    assert visit_order(5, 4, 'backward') == [4, 3, 2, 1, 0]
    assert visit_order(5, 3, 'backward', 1) == [3, 2, 1]
    assert visit_order(5, 2, 'forward', 2) == [2] == visit_order(5, 2, 'backward', 2)
    for args in ((5, 5), (5, -1), (5, 0, 'forward', 5), (5, 3, 'forward', 1), (5, 1, 'backward', 3), (5, 0, 'sideways'), (0,),
                 (5, 1.5), (5, True)):
        with pytest.raises(ValueError):
            visit_order(*args)


def test_key_batches_follow_the_direction_and_the_tail_goes_frame_by_frame():
    from xmem2_amd.session import hinted, visit_order
    for order, kb, want in (
            (visit_order(10), 4, [[0, 1, 2, 3], [4, 5, 6, 7], [8], [9]]),
            (visit_order(10, 9, 'backward'), 4, [[9, 8, 7, 6], [5, 4, 3, 2], [1], [0]]),         # the next frames DOWNWARDS
            (visit_order(8, 7, 'backward'), 4, [[7, 6, 5, 4], [3, 2, 1, 0]]),
            (visit_order(10, 6, 'backward', 1), 4, [[6, 5, 4, 3], [2], [1]]),
            (visit_order(3), 4, [[0], [1], [2]]),
            (visit_order(5), 1, [[0], [1], [2], [3], [4]])):
        batches = []
        seen = []

        def prefetch(batch):
            batches.append(list(batch))
            return [('dev', t) for t in batch]
        for t, dev in hinted(order, kb, prefetch):
            assert dev == ('dev', t)
            seen.append(t)
        assert seen == order and batches == want
    # the hints run ahead exactly as run_on_video's loop lets them: a new batch whenever fewer than key_batch frames are pending
    t_now, calls = [None], []
    gen = hinted(list(range(12)), 4, lambda b: (calls.append((t_now[0], list(b))), b)[1])
    for i in range(12):
        t_now[0] = i
        next(gen)
    assert calls == [(0, [0, 1, 2, 3]), (1, [4, 5, 6, 7]), (5, [8, 9, 10, 11])]


def _label_images():
    """One 256-pixel image per mode the harness reads masks in; pixel v stands for label v."""
    from PIL import Image
    ramp = np.arange(256, dtype=np.uint8)[None]
    pal = Image.fromarray(ramp, mode='P')
    pal.putpalette([(37 * i + c * 11) % 256 for i in range(256) for c in range(3)])
    rgb = np.zeros((1, 256, 3), np.uint8); rgb[0, 1:] = 255                     # the single-object writer: any object white
    v = np.arange(256)
    colours = np.stack([(v * 7) % 256, (v * 3 + 5) % 256, 255 - v], -1)[None].astype(np.uint8)
    one = Image.fromarray((ramp > 0)).convert('1')
    return dict(palette=pal, rgb_white=Image.fromarray(rgb), rgb_colours=Image.fromarray(colours), mode_1=one, grey=Image.fromarray(ramp))


@pytest.mark.parametrize('name', ['palette', 'rgb_white', 'rgb_colours', 'mode_1', 'grey'])
def test_files_table_is_pil_to_tensor01_bit_for_bit(name):
    from xmem2_amd.run_on_video import _pil_to_tensor01
    from xmem2_amd.session import files_table
    pic = _label_images()[name]
    table = files_table(pic)
    assert table.dtype == torch.float32 and tuple(table.shape) == (256,)
    want = _pil_to_tensor01(pic)                                                # C x 1 x 256
    for v in range(256):
        m = want[:, 0, v].max()
        assert table[v].view(torch.int32).item() == m.view(torch.int32).item(), (name, v)
    if name == 'palette':                                                       # the quirk: a palette mask feeds id / 255 to the selector
        assert torch.equal(table, torch.arange(256, dtype=torch.float32).div(255))
        assert table[1].item() == np.float32(1) / np.float32(255) and table[1].item() < 0.5
    if name in ('rgb_white', 'mode_1'):
        assert table[0].item() == 0.0 and bool((table[1:] == 1.0).all())
    with pytest.raises(ValueError):
        files_table(pic.resize((10, 1)))


def test_objects_table():
    from xmem2_amd.session import objects_table
    t = objects_table()
    assert t.dtype == torch.float32 and t[0].item() == 0.0 and bool((t[1:] == 1.0).all()) and t.numel() == 256


def test_new_symbol_is_declared_and_exported_and_the_abi_version_stays_5():
    from xmem2_amd import _lib, ops
    lib = _lib.load()
    assert hasattr(lib, 'xmem_selector_prepare_u8') and lib.xmem_version() == 5 == _lib.ABI_VERSION
    assert lib.xmem_selector_prepare_u8(None, None, None, None, 4, 4, 2, 2, 64, 0.5, 0.5, 0.5, None, None, None, None, None) != 0   # bad args, no launch
    assert callable(ops.selector_prepare_u8)


def _launch_args(**over):
    a = dict(device='cuda', fresh_network_per_video=False)
    a.update(over)
    return argparse.Namespace(**a)


def test_launcher_shares_a_network_only_with_runners_that_take_one(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import stub_runner
    from xmem2_amd import launch
    from xmem2_amd.run_on_video import run_on_video, run_on_video_ensemble, select_k_next_best_annotation_candidates
    for fn in (run_on_video, run_on_video_ensemble, select_k_next_best_annotation_candidates):
        assert inspect.signature(fn).parameters['network'].default is None
    assert 'network' not in inspect.signature(stub_runner.run).parameters
    built = []
    import xmem2_amd.network as N
    monkeypatch.setattr(N.XMem, '__init__', lambda self, *a, **k: built.append(1))
    assert launch.rank_network(_launch_args(), stub_runner.run, {}) is None                      # no `network` parameter
    assert launch.rank_network(_launch_args(device='cpu'), run_on_video, {}) is None             # launcher tests on the CPU
    assert launch.rank_network(_launch_args(fresh_network_per_video=True), run_on_video, {}) is None
    assert built == []


def test_launch_worker_with_the_stub_runner_passes_no_network(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import stub_runner
    from xmem2_amd import launch
    for sub, ext in (('JPEGImages', '.jpg'), ('Annotations', '.png')):
        d = tmp_path / sub / 'vid0'
        d.mkdir(parents=True)
        for t in range(3):
            (d / f'{t:05d}{ext}').write_bytes(b'x')
    seen = []

    def run(imgs_in_path, masks_in_path, masks_out_path, frames_with_masks=(0,), compute_iou=False, print_progress=True,
            overwrite_config=None, **kwargs):
        seen.append(dict(kwargs))
        return stub_runner.run(imgs_in_path, masks_in_path, masks_out_path, frames_with_masks, compute_iou, print_progress,
                               overwrite_config, **kwargs)
    monkeypatch.setattr(launch, '_resolve', lambda spec: run)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    args = argparse.Namespace(out=str(tmp_path / 'out'), videos=str(tmp_path / 'JPEGImages'), masks=str(tmp_path / 'Annotations'),
                              device='cpu', runner='stub_runner:run', config='{"size": -1}', frames_with_masks='0',
                              compute_iou=False, compute_jf=False, threads_per_rank=8, fresh_network_per_video=False)
    assert launch.worker(args) == 0
    assert seen == [{}] and os.path.exists(tmp_path / 'out' / 'vid0' / 'masks' / '00000.png')

    # the same through `worker` on a (pretended) GPU device: the runner WITHOUT a `network` parameter is still left alone, the one
    # WITH it receives the rank's one network for every video
    import xmem2_amd.network as N
    built = []

    class _Net:
        def __init__(self, config, model_path=None, **kw):
            built.append(model_path)

        def to(self, device):
            return self

        def eval(self):
            return self
    monkeypatch.setattr(N, 'XMem', _Net)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'device_count', lambda: 1)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    for sub, ext in (('JPEGImages', '.jpg'), ('Annotations', '.png')):
        d = tmp_path / sub / 'vid1'
        d.mkdir(parents=True)
        (d / f'00000{ext}').write_bytes(b'x')
    args.device, args.config = 'cuda', '{"size": -1, "model": "weights.pth"}'
    seen.clear()
    assert launch.worker(args) == 0 and seen == [{}, {}] and built == []

    def run_with_network(imgs_in_path, masks_in_path, masks_out_path, frames_with_masks=(0,), compute_iou=False, print_progress=True,
                         overwrite_config=None, network=None, **kwargs):
        seen.append(network)
        return stub_runner.run(imgs_in_path, masks_in_path, masks_out_path, frames_with_masks, compute_iou, print_progress, overwrite_config)
    monkeypatch.setattr(launch, '_resolve', lambda spec: run_with_network)
    seen.clear()
    assert launch.worker(args) == 0
    assert built == ['weights.pth'] and len(seen) == 2 and isinstance(seen[0], _Net) and seen[0] is seen[1]
    args.fresh_network_per_video = True
    seen.clear()
    assert launch.worker(args) == 0 and seen == [None, None] and built == ['weights.pth']


def test_launch_parses_fresh_network_per_video(monkeypatch):
    from xmem2_amd import launch
    got = []
    monkeypatch.setattr(launch, 'worker', lambda args: got.append(args) or 0)
    monkeypatch.setenv('WORLD_SIZE', '1')
    base = ['--gpus', '1', '--videos', 'v', '--out', 'o', '--as-worker']
    assert launch.main(base) == 0 and got[-1].fresh_network_per_video is False
    assert launch.main(base + ['--fresh-network-per-video']) == 0 and got[-1].fresh_network_per_video is True


def test_session_cli_parses_and_validates():
    from xmem2_amd import session
    a = session.parse_args(['--images', 'i', '--masks', 'm', '--out', 'o', '--rounds', '2', '--k', '3'])
    assert (a.rounds, a.k, a.first, a.mask_form, a.overlay) == (2, 3, '0', 'objects', False)
    for bad in (['--rounds', '0'], ['--k', '0'], ['--mask-form', 'soft']):
        with pytest.raises(SystemExit):
            session.parse_args(['--images', 'i', '--masks', 'm', '--out', 'o'] + bad)


def test_propagate_on_a_stub_core_fills_the_arenas_and_makes_run_on_videos_calls(monkeypatch, tmp_path):
    """The frame loop on stubs: which frames are hinted and stepped in which order with which flags, what lands in the arenas, and what
    stats() / save() make of it (a real reader over a tiny clip for the writer)."""
    from PIL import Image
    import xmem2_amd.run_on_video as rv
    from xmem2_amd.run_on_video import VideoReader
    n, hw, ck, grid = 6, (16, 32), 4, (1, 2)
    imgs, msks = tmp_path / 'i', tmp_path / 'm'
    imgs.mkdir(); msks.mkdir()
    s = _stub_session(n, hw, monkeypatch)
    for t in range(n):
        Image.fromarray(np.full(hw + (3,), 10 * t, np.uint8)).save(imgs / f'{t:05d}.png')
        if s.frames[t].mask is not None:
            im = Image.fromarray(s.frames[t].mask, mode='P'); im.putpalette([0, 0, 0, 9, 8, 7] + [0] * 762); im.save(msks / f'{t:05d}.png')
        s.frames[t].frame, s.frames[t].raw_image_pil = f'{t:05d}.png', Image.open(imgs / f'{t:05d}.png').convert('RGB')
    s.reader = VideoReader('', str(imgs), str(msks), size=-1, use_all_masks=True)
    s.grid_hw = grid
    s.key = torch.zeros(n, 2, ck); s.shrinkage = torch.zeros(n, 2); s.selection = torch.zeros(n, 2, ck)
    for t in range(n):
        s._dev_frames[t] = t                                  # a frame is recognised by its value
    log = []

    def prefetch_keys(images, inputs_complete=False):
        log.append(('hint', [int(im[0, 0, 0]) for im in images], inputs_complete))
        return list(images)

    def step(image, mask, labels, end=False, manually_curated_masks=False, do_not_add_mask_to_memory=False, return_key_and_stuff=False):
        t = int(image[0, 0, 0])
        log.append(('step', t, None if mask is None else tuple(mask.shape), None if labels is None else list(labels), end,
                    do_not_add_mask_to_memory, return_key_and_stuff))
        prob = torch.zeros((2,) + hw); prob[1, :, :t + 1] = 1.0; prob[0, :, t + 1:] = 1.0      # object 1 in the first t + 1 columns
        key = torch.full((1, 2, ck), float(t)).view(1, 1, 2, ck).permute(0, 3, 1, 2)           # NHWC-strided views, as the core's
        sel = torch.arange(2 * ck, dtype=torch.float32).view(1, 1, 2, ck).permute(0, 3, 1, 2) + 100 * t
        return prob, key, torch.full((1, 1, 1, 2), t + 0.5), sel
    s.core.prefetch_keys, s.core.step = prefetch_keys, step
    monkeypatch.setattr(rv, '_post_process_gpu', lambda sample, prob: prob.argmax(0).to(torch.uint8))
    s.save_reference(0); s.save_reference(3)
    assert s.full_propagation() == list(range(n)) and s.core.calls[-1] == ('clear', True)
    assert [e for e in log if e[0] == 'hint'] == [('hint', [0, 1, 2, 3], True), ('hint', [4], True), ('hint', [5], True)]
    steps = [e for e in log if e[0] == 'step']
    assert [e[1] for e in steps] == list(range(n))
    for e in steps:
        ref = e[1] in (0, 3)
        assert e[2] == ((1,) + hw if ref else None) and e[3] == ([1] if ref else None) and e[5] is ref and e[6] is True
        assert e[4] is (e[1] == n - 1)                        # end=True on the last visited frame only
    assert s.all_masks_present()
    for t in range(n):
        assert bool((s.key[t] == t).all()) and bool((s.shrinkage[t] == t + 0.5).all())
        assert torch.equal(s.selection[t], torch.arange(2 * ck, dtype=torch.float32).view(2, ck) + 100 * t)
        assert int(s.masks[t].sum()) == hw[0] * (t + 1) and torch.equal(s.mask(t), s.masks[t])
    # backward over a part of the clip: the batch is the next frames downwards, the last visited frame carries end=True
    log.clear()
    assert s.propagate(4, 'backward', 0) == [4, 3, 2, 1, 0]
    assert [e[1] for e in log if e[0] == 'hint'] == [[4, 3, 2, 1], [0]]
    assert [(e[1], e[4]) for e in log if e[0] == 'step'] == [(4, False), (3, False), (2, False), (1, False), (0, True)]
    # stats: run_on_video's columns; iou only where a ground truth exists and no mask was given
    df = s.stats(compute_iou=True)
    assert list(df.columns) == ['frame', 'mask_provided', 'iou'] and list(df['frame']) == [f'{t:05d}.png' for t in range(n)]
    assert list(df['mask_provided']) == [t in (0, 3) for t in range(n)]
    assert df['iou'][0] == -1 and df['iou'][3] == -1 and df['iou'][4] == -1 and 0.0 <= df['iou'][1] <= 1.0
    assert list(s.stats().columns) == ['frame', 'mask_provided']
    # save: run_on_video's layout and colours
    s.save(tmp_path / 'out', save_overlay=True)
    assert sorted(os.listdir(tmp_path / 'out' / 'masks')) == [f'{t:05d}.png' for t in range(n)]
    assert sorted(os.listdir(tmp_path / 'out' / 'overlay')) == [f'{t:05d}.jpg' for t in range(n)]
    got = np.array(Image.open(tmp_path / 'out' / 'masks' / '00002.png').convert('RGB'))
    assert tuple(got[0, 0]) == (9, 8, 7) and tuple(got[0, 3]) == (0, 0, 0)
    # the 'files' table of this palette: max(9, 8, 7) / 255 for the object
    table = s.mask_table('files')
    assert table[1].item() == (torch.tensor(9, dtype=torch.float32) / 255).item() and table[0].item() == 0.0
    assert torch.equal(s.mask_table('objects')[:3], torch.tensor([0.0, 1.0, 1.0]))


def test_taking_a_frame_out_needs_one_object_group(monkeypatch):
    """An object that first appeared in a later reference opens a second object group in the store: removal, replacement and a
    reference in front of existing ones raise before anything is changed; appending still works."""
    s = _stub_session(monkeypatch=monkeypatch)
    s.save_reference(0); s.save_reference(3)

    class _TwoGroups:
        num_groups = 2
    s.core.memory.permanent_work_mem = _TwoGroups()
    before = list(s.core.calls)
    for call in (lambda: s.remove_reference(3), lambda: s.save_reference(3), lambda: s.save_reference(1)):
        with pytest.raises(NotImplementedError, match='object groups'):
            call()
    assert s.core.calls == before and s.references == [0, 3]
    assert s.save_reference(5) is False and s.references == [0, 3, 5]
