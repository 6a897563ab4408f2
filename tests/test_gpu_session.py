"""VideoSession on the device: the label-plane selector kernel against the float one, a forward propagation against `run_on_video`,
the annotate -> propagate loop without re-decoding, candidates without a second encoder pass, backward propagation against the oracle,
and the network that outlives a call (run_on_video, the ensemble, the launcher, the command line).

One network per module (built from a checkpoint FILE of the synthetic weights, so that child processes and `network=None` calls load
the same weights quickly); the clips are 9 frames of 96 x 128; every `run_on_video` result is computed once and shared."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

T_CLIP, HW = 9, (96, 128)
PALETTES = {1: [0, 0, 0, 255, 255, 255], 2: [0, 0, 0, 200, 0, 0, 0, 200, 0]}


@pytest.fixture(scope='module')
def checkpoint(synth_sd, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt') / 'XMem_synth.pth'
    torch.save(synth_sd, path)
    return str(path)


@pytest.fixture(scope='module')
def cfg(checkpoint):
    return {'model': checkpoint, 'size': -1, 'mem_every': 2}


@pytest.fixture(scope='module')
def net(checkpoint):
    from xmem2_amd.network import XMem
    return XMem({'precision': 'fp32'}, checkpoint).to('cuda').eval()


def _write_clip(root, n_obj, seed=1234, hw=HW, t=T_CLIP, second_object_from=0):
    from PIL import Image
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    imgs, msks = root / 'JPEGImages', root / 'Annotations'
    imgs.mkdir(parents=True); msks.mkdir(parents=True)
    frames, masks = synthetic_frames(t, *hw, seed=seed), synthetic_masks(t, n_obj, *hw)
    pal = PALETTES[n_obj] + [0] * (768 - len(PALETTES[n_obj]))
    for i in range(t):
        rgb = np.clip((frames[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(imgs / f'frame_{i:06d}.png')
        idx = sum(masks[i, o] * (o + 1) for o in range(n_obj) if o == 0 or i >= second_object_from).astype(np.uint8)
        im = Image.fromarray(idx, mode='P'); im.putpalette(pal); im.save(msks / f'frame_{i:06d}.png')
    return str(imgs), str(msks)


@pytest.fixture(scope='module')
def clips(tmp_path_factory):
    root = tmp_path_factory.mktemp('clips')
    return {1: _write_clip(root / 'one', 1), 2: _write_clip(root / 'two', 2), 'other': _write_clip(root / 'other', 1, seed=77),
            'small': _write_clip(root / 'small', 1, hw=(80, 112)), 'late': _write_clip(root / 'late', 2, second_object_from=3)}


def _mask_bytes(out_dir):
    d = os.path.join(str(out_dir), 'masks')
    return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}


@pytest.fixture(scope='module')
def rov(clips, cfg, net, tmp_path_factory):
    """run_on_video(frames_with_masks=refs, network=net) on a clip, once per (clip, refs): (mask PNG bytes by name, stats)."""
    from xmem2_amd.run_on_video import run_on_video
    cache = {}

    def get(which, refs):
        key = (which, tuple(refs))
        if key not in cache:
            out = tmp_path_factory.mktemp('rov')
            imgs, msks = clips[which]
            stats = run_on_video(imgs, msks, str(out), frames_with_masks=list(refs), compute_iou=True, print_progress=False,
                                 overwrite_config=dict(cfg), save_overlay=False, network=net)
            cache[key] = (_mask_bytes(out), stats)
        return cache[key]
    return get


def _session(clips, cfg, net, which, refs=()):
    from xmem2_amd.session import VideoSession
    s = VideoSession(*clips[which], overwrite_config=dict(cfg), network=net)
    for t in refs:
        s.save_reference(t)
    return s


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
def _tables():
    g = torch.Generator().manual_seed(5)
    objects = torch.ones(256); objects[0] = 0
    return {'objects': objects, 'files': torch.arange(256, dtype=torch.float32).div(255), 'random': torch.rand(256, generator=g)}


@pytest.mark.parametrize('form', ['objects', 'files', 'random'])
@pytest.mark.parametrize('H,W,h,w,ck', [(1, 1, 1, 1, 64), (5, 7, 2, 3, 64), (97, 131, 7, 9, 64), (3, 4, 6, 8, 64), (5, 7, 2, 3, 8),
                                        (97, 131, 7, 9, 8)])
def test_selector_prepare_u8_is_bit_identical_to_the_float_kernel(form, H, W, h, w, ck):
    from xmem2_amd import ops
    g = torch.Generator().manual_seed(H * 1000 + W + ck)
    lut = _tables()[form].cuda()
    key = torch.randn(h * w, ck, generator=g).cuda()
    sel = torch.rand(h * w, ck, generator=g).cuda()
    special = torch.tensor([0, 1, 127, 128, 255], dtype=torch.uint8)
    planes = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
    planes.view(-1)[:min(5, H * W)] = special[:min(5, H * W)]
    planes[0, -1, -1] = 255                                  # the far corner, where the source index is clamped
    planes[1] = 0                                            # presence exactly 0 (every table has lut[0] <= eps ... see below)
    planes[2] = 255                                          # presence exactly H * W when lut[255] > eps
    planes = planes.cuda()                                   # plane 1 and 2 start at H*W and 2*H*W bytes: odd sizes are unaligned
    for i, alpha in ((0, 0.5), (1, 0.3), (2, 1.0)):
        u8 = planes[i]
        fm = lut[u8.long()][None].contiguous()
        outs = []
        for run in ('u8', 'float'):
            Mexp = torch.full((h * w, 2 * ck), float('nan'), device='cuda'); Qexp = torch.full_like(Mexp, float('nan'))
            bsq = torch.full((h * w,), float('nan'), device='cuda'); pres = torch.full((1,), -7, dtype=torch.int32, device='cuda')
            if run == 'u8':
                ops.selector_prepare_u8(key, sel, u8, lut, h, w, alpha, 0.5, Mexp, Qexp, bsq, pres)
            else:
                ops.selector_prepare(key, sel, fm, h, w, alpha, 0.5, Mexp, Qexp, bsq, pres)
            outs.append((Mexp, Qexp, bsq, pres))
        for a, b, name in zip(outs[0], outs[1], ('Mexp', 'Qexp', 'bsq', 'presence')):
            assert torch.equal(a, b), f'{name} of plane {i}'
            assert not bool(torch.isnan(a.float()).any()), name
        want = int((lut[u8.long()] > 0.5).sum())
        assert int(outs[0][3]) == want
        if i == 1 and float(lut[0]) <= 0.5:
            assert want == 0
        if i == 2 and float(lut[255]) > 0.5:
            assert want == H * W


def test_selector_prepare_u8_rejects_bad_arguments():
    from xmem2_amd import ops
    key = torch.zeros(6, 64, device='cuda'); out = torch.zeros(6, 128, device='cuda'); b = torch.zeros(6, device='cuda')
    p = torch.zeros(1, dtype=torch.int32, device='cuda'); lut = torch.zeros(256, device='cuda')
    u8 = torch.zeros(5, 7, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError):
        ops.selector_prepare_u8(key, key, u8, lut, 2, 2, 0.5, 0.5, out, out, b, p)          # rows != h * w
    with pytest.raises(ValueError):
        ops.selector_prepare_u8(key, key, u8, lut[:255], 2, 3, 0.5, 0.5, out, out, b, p)
    with pytest.raises(RuntimeError):
        ops.selector_prepare_u8(key, key, u8.float(), lut, 2, 3, 0.5, 0.5, out, out, b, p)  # a float mask is the other entry point
    with pytest.raises(ValueError):
        ops.selector_prepare_u8(key, key, u8[None], lut, 2, 3, 0.5, 0.5, out, out, b, p)


# ---- 2. forward == run_on_video --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_obj', [1, 2])
@pytest.mark.parametrize('refs', [(0,), (0, 5)])
def test_full_propagation_writes_what_run_on_video_writes(clips, cfg, net, rov, tmp_path, n_obj, refs):
    import pandas as pd
    want_bytes, want_stats = rov(n_obj, refs)
    s = _session(clips, cfg, net, n_obj, refs)
    assert s.references == list(refs) and len(s) == T_CLIP and not s.all_masks_present()
    assert s.full_propagation() == list(range(T_CLIP)) and s.all_masks_present()
    s.save(tmp_path / 'out', save_overlay=True)
    assert _mask_bytes(tmp_path / 'out') == want_bytes
    assert len(os.listdir(tmp_path / 'out' / 'overlay')) == T_CLIP
    pd.testing.assert_frame_equal(s.stats(compute_iou=True), want_stats)
    m = s.mask(3)
    assert m.is_cuda and m.dtype == torch.uint8 and tuple(m.shape) == HW and set(np.unique(m.cpu().numpy())) <= set(range(n_obj + 1))


# ---- 3. iteration ----------------------------------------------------------------------------------------------------------
def test_iteration_reuses_frames_network_and_gives_run_on_video_results(clips, cfg, net, rov, tmp_path, monkeypatch):
    """save_reference with a device mask + a second propagation == run_on_video with that frame added, with no decode, frame upload or
    new network in between; remove_reference + propagation gives the first result back."""
    from PIL import Image
    from xmem2_amd.inference_core import InferenceCore
    from xmem2_amd.network import XMem
    s = _session(clips, cfg, net, 2, (0,))
    s.full_propagation()
    s.save(tmp_path / 'a', save_overlay=False)
    first = _mask_bytes(tmp_path / 'a')
    assert first == rov(2, (0,))[0]
    gt5 = np.array(Image.open(os.path.join(clips[2][1], 'frame_000005.png')).convert('P'), dtype=np.uint8)

    events = []
    orig_open, orig_init = Image.open, XMem.__init__
    monkeypatch.setattr(Image, 'open', lambda *a, **k: (events.append('Image.open'), orig_open(*a, **k))[1])
    monkeypatch.setattr(XMem, '__init__', lambda self, *a, **k: (events.append('XMem.__init__'), orig_init(self, *a, **k))[1])
    for name in ('step', 'put_to_permanent_memory'):
        orig = getattr(InferenceCore, name)

        def spy(self, image, *a, _orig=orig, _name=name, **k):
            if not image.is_cuda:
                events.append(f'host frame into {_name}')
            return _orig(self, image, *a, **k)
        monkeypatch.setattr(InferenceCore, name, spy)
    orig_pf = InferenceCore.prefetch_keys

    def spy_pf(self, images, *a, **k):
        if not all(im.is_cuda for im in images):
            events.append('host frame into prefetch_keys')
        return orig_pf(self, images, *a, **k)
    monkeypatch.setattr(InferenceCore, 'prefetch_keys', spy_pf)

    assert s.save_reference(5, torch.from_numpy(gt5).cuda()) is False and s.references == [0, 5]
    s.full_propagation()
    assert events == []                                      # no decode, no frame upload, no new network between the propagations
    monkeypatch.undo()
    s.save(tmp_path / 'b', save_overlay=False)
    assert _mask_bytes(tmp_path / 'b') == rov(2, (0, 5))[0]
    s.remove_reference(5)
    assert s.references == [0]
    s.full_propagation()
    s.save(tmp_path / 'c', save_overlay=False)
    assert _mask_bytes(tmp_path / 'c') == first


def test_a_reference_in_front_of_the_others_gives_the_run_on_video_memory(clips, cfg, net, rov, tmp_path):
    """References saved out of frame order: the permanent memory is rebuilt in frame order, removing the middle one takes exactly its
    elements out."""
    s = _session(clips, cfg, net, 1, (5,))
    s.save_reference(0)
    assert s.references == [0, 5] and s.core.permanent_memory_frames == [0, 5]
    s.full_propagation()
    s.save(tmp_path / 'a', save_overlay=False)
    assert _mask_bytes(tmp_path / 'a') == rov(1, (0, 5))[0]
    s.save_reference(3)
    assert s.core.memory.frame_id_to_permanent_mem_idx == {0: 0, 3: 1, 5: 2}          # true positions
    s.remove_reference(3)
    assert s.core.permanent_memory_frames == [0, 5] and s.core.memory.frame_id_to_permanent_mem_idx == {0: 0, 5: 1}
    s.full_propagation()
    s.save(tmp_path / 'b', save_overlay=False)
    assert _mask_bytes(tmp_path / 'b') == rov(1, (0, 5))[0]
    # replacing a reference's mask and putting the original back: frame 5's entry is the one rewritten, frame 0's stays
    other = np.zeros(HW, np.uint8); other[10:40, 20:70] = 1
    assert s.save_reference(5, other) is True and s.references == [0, 5]
    s.full_propagation()
    s.save(tmp_path / 'c', save_overlay=False)
    assert _mask_bytes(tmp_path / 'c') != rov(1, (0, 5))[0]
    assert s.save_reference(5) is True
    s.full_propagation()
    s.save(tmp_path / 'd', save_overlay=False)
    assert _mask_bytes(tmp_path / 'd') == rov(1, (0, 5))[0]


def test_an_object_that_first_appears_in_a_later_reference(clips, cfg, net, rov, tmp_path):
    """Frame 0 shows object 1, frame 5 objects 1 and 2: appended in frame order the session builds run_on_video's two object groups;
    taking a frame out of such a store is refused before anything changes."""
    s = _session(clips, cfg, net, 'late', (0, 5))
    assert s.core.memory.permanent_work_mem.num_groups == 2
    s.full_propagation()
    s.save(tmp_path / 'a', save_overlay=False)
    want = rov('late', (0, 5))[0]
    assert _mask_bytes(tmp_path / 'a') == want
    for call in (lambda: s.remove_reference(5), lambda: s.remove_reference(0), lambda: s.save_reference(5), lambda: s.save_reference(2)):
        with pytest.raises(NotImplementedError, match='object groups'):
            call()
    assert s.references == [0, 5] and s.core.memory.frame_id_to_permanent_mem_idx == {0: 0, 5: 1}
    s.full_propagation()
    s.save(tmp_path / 'b', save_overlay=False)
    assert _mask_bytes(tmp_path / 'b') == want
    s.save_reference(7)                                      # appending goes on working
    s.full_propagation()
    s.save(tmp_path / 'c', save_overlay=False)
    assert _mask_bytes(tmp_path / 'c') == rov('late', (0, 5, 7))[0]


def test_session_without_a_mask_directory_and_probability_masks(clips, cfg, net, tmp_path):
    """masks_in_path=None (the reader set up by hand) and an annotation given as [K+1, H, W] probabilities: the same device masks as the
    session that reads the annotation file; the written PNGs use the grey-ramp palette."""
    from PIL import Image
    from xmem2_amd.session import VideoSession
    want = _session(clips, cfg, net, 2, (0,))
    want.full_propagation()
    gt = torch.from_numpy(np.array(Image.open(os.path.join(clips[2][1], 'frame_000000.png')).convert('P'), dtype=np.uint8))
    prob = torch.stack([(gt == c).float() * 0.9 + 0.05 for c in range(3)]).cuda()
    s = VideoSession(clips[2][0], None, overwrite_config=dict(cfg), network=net)
    with pytest.raises(FileNotFoundError):
        s.save_reference(0)                                  # there is no annotation file to fall back on
    assert s.save_reference(0, prob) is False
    s.full_propagation()
    assert torch.equal(s.masks, want.masks)
    s.save(tmp_path / 'out', save_overlay=True)
    got = np.array(Image.open(tmp_path / 'out' / 'masks' / 'frame_000000.png').convert('RGB'))
    assert np.array_equal(got[..., 0], gt.numpy()) and np.array_equal(got[..., 0], got[..., 2])      # label v -> grey v
    assert len(os.listdir(tmp_path / 'out' / 'overlay')) == T_CLIP
    assert list(s.stats()['mask_provided']) == [True] + [False] * (T_CLIP - 1)


# ---- 4. candidates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_obj', [1, 2])
def test_candidates_use_the_keys_of_the_propagation_and_agree_with_the_file_api(clips, cfg, net, tmp_path, monkeypatch, n_obj):
    from PIL import Image
    from xmem2_amd import frame_selection
    from xmem2_amd.frame_selection import select_next_candidates
    from xmem2_amd.inference_core import InferenceCore
    from xmem2_amd.run_on_video import select_k_next_best_annotation_candidates
    k = 3
    s = _session(clips, cfg, net, n_obj, (0,))
    got_keys = []
    orig_step = InferenceCore.step

    def step(self, *a, **kw):
        out = orig_step(self, *a, **kw)
        if kw.get('return_key_and_stuff'):
            got_keys.append(tuple(t.clone() for t in out[1:]))
        return out
    monkeypatch.setattr(InferenceCore, 'step', step)
    s.full_propagation()
    monkeypatch.undo()
    assert len(got_keys) == T_CLIP

    calls = []
    orig_open = Image.open
    monkeypatch.setattr(Image, 'open', lambda *a, **kw: (calls.append('Image.open'), orig_open(*a, **kw))[1])
    monkeypatch.setattr(InferenceCore, 'encode_frame_key', lambda self, *a, **kw: calls.append('encode_frame_key'))
    monkeypatch.setattr(frame_selection, 'extract_keys', lambda *a, **kw: calls.append('extract_keys'))
    got = s.candidates(k)
    got_trace = [t.copy() for t in select_next_candidates.last_scores]
    got_files = s.candidates(k, mask_form='files')
    files_trace = [t.copy() for t in select_next_candidates.last_scores]
    assert calls == []
    monkeypatch.undo()
    assert len(got) == k and not set(got) & set(s.references)

    # the same function of the same tensors: what step() returned and the float masks the table stands for
    keys, shrs, sels = (torch.cat([g[i] for g in got_keys]) for i in range(3))
    for form, mine, trace in (('objects', got, got_trace), ('files', got_files, files_trace)):
        lut = s.mask_table(form).cuda()
        masks = [lut[s.masks[t].long()][None] for t in range(T_CLIP)]
        want = select_next_candidates(keys, shrs, sels, masks, k, previously_chosen_candidates=s.references, device='cuda:0')
        assert mine == want, form
        for a, b in zip(trace, select_next_candidates.last_scores):
            assert np.array_equal(a, b), form

    # the file API on the PNGs save() wrote (its own key pass, masks read back from the files)
    s.save(tmp_path / 'out', save_overlay=False)
    by_files = select_k_next_best_annotation_candidates(clips[n_obj][0], clips[n_obj][1], str(tmp_path / 'out'), k=k, print_progress=False,
                                                        previously_chosen_candidates=[0], use_previously_predicted_masks=True,
                                                        overwrite_config=dict(cfg), network=net)
    api_trace = select_next_candidates.last_scores
    for it, (a, b) in enumerate(zip(files_trace, api_trace)):
        diff = float(np.abs(a - b).max())
        top = np.sort(a)[::-1]
        print(f'{n_obj} object(s), round {it}: best - second = {top[0] - top[1]:.3e}, largest difference between the paths = {diff:.3e}')
        assert top[0] - top[1] > diff, f'round {it}: a tie could hide a fault (gap {top[0] - top[1]:.3e} <= path difference {diff:.3e})'
    assert got_files == by_files


# ---- 5. backward -----------------------------------------------------------------------------------------------------------
def test_backward_propagation_vs_oracle(clips, cfg, net, ref_net, monkeypatch):
    """propagate(start=last, direction='backward') against oracle.cpu_ref's core stepped over the same frames in the same order; the
    per-frame gates are those of tests/test_gpu_e2e.py::test_update_schedules_vs_oracle (mean |dp| < 3e-4, argmax mismatch < 1e-3),
    the clip-level comparison is clip_util.compare."""
    from clip_util import compare, fmt
    from oracle import cpu_ref as R
    from xmem2_amd.inference_core import InferenceCore
    from xmem2_amd.run_on_video import IM_MEAN, IM_STD
    last = T_CLIP - 1
    s = _session(clips, cfg, net, 1, (last,))
    probs = []
    orig_step = InferenceCore.step
    monkeypatch.setattr(InferenceCore, 'step', lambda self, *a, **kw: (lambda out: (probs.append(out[0].cpu()), out)[1])(orig_step(self, *a, **kw)))
    order = s.propagate(start=last, direction='backward')
    monkeypatch.undo()
    assert order == list(range(last, -1, -1)) and s.all_masks_present()

    ref = R.RefCore(ref_net, dict(s.config))
    ref.set_all_labels([1])
    frames = [torch.from_numpy(np.ascontiguousarray(((s.frame_u8(t).cpu().numpy().astype(np.float32) / 255.0 - IM_MEAN) / IM_STD).transpose(2, 0, 1)))
              for t in range(T_CLIP)]
    raw = torch.from_numpy(s._refs[last].astype(np.int64))
    onehot = (raw == 1)[None].float()
    ref.put_to_permanent_memory(frames[last], onehot)
    want = []
    for i, t in enumerate(order):
        mk = onehot.clone() if t == last else None
        q = ref.step(frames[t], mk, [1] if mk is not None else None, end=(i == len(order) - 1), do_not_add_mask_to_memory=(mk is not None))
        want.append(torch.argmax(q, 0).numpy().astype(np.uint8))
        d = (probs[i] - q).abs()
        mism = float((probs[i].argmax(0) != q.argmax(0)).float().mean())
        assert float(d.mean()) < 3e-4 and mism < 1e-3, f'frame {t}: mean |dp| {float(d.mean()):.2e}, argmax mismatch {mism:.2e}'
    got = [s.masks[t].cpu().numpy() for t in order]
    c = compare(got, want, [1])
    print('backward vs oracle:', fmt(c))
    assert c['mismatch'] / c['pixels'] < 1e-3


def test_partial_propagation_visits_only_the_range(clips, cfg, net):
    s = _session(clips, cfg, net, 1, (4,))
    assert s.propagate(4, 'forward', 6) == [4, 5, 6]
    assert [t for t in range(T_CLIP) if s.mask(t) is not None] == [4, 5, 6]
    assert s.propagate(4, 'backward', 2) == [4, 3, 2]
    assert [t for t in range(T_CLIP) if s.mask(t) is not None] == [2, 3, 4, 5, 6]
    with pytest.raises(RuntimeError, match='Run propagation on all frames first'):
        s.candidates(1)


def test_frames_beyond_the_byte_cap_stay_in_pinned_host_memory(clips, cfg, net, rov, tmp_path):
    from xmem2_amd.session import VideoSession
    per_frame = HW[0] * HW[1] * 3
    s = VideoSession(*clips[1], overwrite_config=dict(cfg, session_device_frame_bytes=5 * per_frame), network=net)
    assert s.n_device_frames == 5 and s.frame_u8(4).is_cuda and not s.frame_u8(5).is_cuda and s.frame_u8(5).is_pinned()
    s.save_reference(0)
    s.full_propagation()
    s.save(tmp_path / 'out', save_overlay=False)
    assert _mask_bytes(tmp_path / 'out') == rov(1, (0,))[0]


# ---- 6. the network outlives a call ----------------------------------------------------------------------------------------
def _count_network_work(monkeypatch):
    from xmem2_amd.network import XMem
    counts = dict(init=0, upload=0, graphs=0)
    orig_init, orig_upload, orig_graph = XMem.__init__, XMem._upload, torch.cuda.CUDAGraph
    monkeypatch.setattr(XMem, '__init__', lambda self, *a, **k: (counts.__setitem__('init', counts['init'] + 1), orig_init(self, *a, **k))[1])
    monkeypatch.setattr(XMem, '_upload', lambda self: (counts.__setitem__('upload', counts['upload'] + 1), orig_upload(self))[1])
    monkeypatch.setattr(torch.cuda, 'CUDAGraph', lambda *a, **k: (counts.__setitem__('graphs', counts['graphs'] + 1), orig_graph(*a, **k))[1])
    return counts


@pytest.mark.parametrize('runner_name,extra', [('run_on_video', {}), ('run_on_video_ensemble', {'ensemble': [[-1, False]]})])
def test_a_given_network_is_reused_across_calls(clips, cfg, checkpoint, tmp_path, monkeypatch, runner_name, extra):
    import xmem2_amd.run_on_video as rv
    from xmem2_amd.network import XMem
    runner = getattr(rv, runner_name)
    over = dict(cfg, **extra)
    counts = _count_network_work(monkeypatch)
    mine = XMem({'precision': 'fp32'}, checkpoint).to('cuda').eval()
    assert counts['init'] == 1
    uploads = counts['upload']

    def run(which, out, network):
        runner(*clips[which], str(tmp_path / out), frames_with_masks=[0, 5], print_progress=False, overwrite_config=dict(over),
               save_overlay=False, network=network)
        return _mask_bytes(tmp_path / out)
    a = run(1, 'a', mine)
    stages, graphs = len(mine._stages), counts['graphs']
    assert stages > 0 and graphs > 0
    b = run('other', 'b', mine)                              # same geometry, same object count: replayed, nothing captured
    assert counts['init'] == 1 and counts['upload'] == uploads
    assert len(mine._stages) == stages and counts['graphs'] == graphs
    c = run('small', 'c', mine)                              # another geometry: new stages, same network
    assert counts['init'] == 1 and counts['upload'] == uploads and len(mine._stages) > stages
    # byte-identical to the path that builds a network per call
    assert run(1, 'a0', None) == a and run('other', 'b0', None) == b and run('small', 'c0', None) == c
    assert counts['init'] == 4
    with pytest.raises(ValueError, match='model'):
        runner(*clips[1], str(tmp_path / 'x'), overwrite_config=dict(over, model=None), network=mine)
    with pytest.raises(ValueError, match='precision'):
        runner(*clips[1], str(tmp_path / 'x'), overwrite_config=dict(over, precision='fp16'), network=mine)


def test_stage_cache_stays_bounded_with_a_shared_network(clips, cfg, checkpoint, tmp_path, monkeypatch):
    """A rank that sees several geometries: at MAX_STAGES the least recently replayed stages (an earlier video's) are dropped and
    captured again on demand; the masks do not change."""
    import xmem2_amd.network as N
    from xmem2_amd.run_on_video import run_on_video
    mine = N.XMem({'precision': 'fp32'}, checkpoint).to('cuda').eval()

    def run(which, out):
        run_on_video(*clips[which], str(tmp_path / out), frames_with_masks=[0], print_progress=False, overwrite_config=dict(cfg),
                     save_overlay=False, network=mine)
        return _mask_bytes(tmp_path / out)
    a = run(1, 'a')
    cap = len(mine._stages)
    monkeypatch.setattr(N, 'MAX_STAGES', cap)                # room for one geometry's stages
    evicted = []
    orig = N.XMem._evict_lru
    monkeypatch.setattr(N.XMem, '_evict_lru', lambda self: (evicted.append(1), orig(self))[1])
    run('small', 'b')
    assert evicted and len(mine._stages) <= cap
    assert run(1, 'a2') == a and len(mine._stages) <= cap


# ---- 7. the launcher -------------------------------------------------------------------------------------------------------
def test_launcher_builds_one_network_per_rank(cfg, tmp_path, monkeypatch):
    import argparse
    from xmem2_amd import launch
    chair = os.path.join(GOLDEN, 'chair')
    names = sorted(os.listdir(os.path.join(chair, 'JPEGImages')))
    for vid, part in (('chair_a', names[:5]), ('chair_b', names[5:])):
        for sub in ('JPEGImages', 'Annotations'):
            (tmp_path / sub / vid).mkdir(parents=True)
        for nm in part:
            shutil.copy(os.path.join(chair, 'JPEGImages', nm), tmp_path / 'JPEGImages' / vid / nm)
            shutil.copy(os.path.join(chair, 'Annotations', nm[:-4] + '.png'), tmp_path / 'Annotations' / vid / (nm[:-4] + '.png'))
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    counts = _count_network_work(monkeypatch)
    results = {}
    for mode, fresh in (('shared', False), ('fresh', True)):
        before = counts['init']
        args = argparse.Namespace(out=str(tmp_path / mode), videos=str(tmp_path / 'JPEGImages'), masks=str(tmp_path / 'Annotations'),
                                  device='cuda', runner='xmem2_amd.run_on_video:run_on_video', config=json.dumps(dict(cfg, size=96)),
                                  frames_with_masks='0', compute_iou=False, compute_jf=False, threads_per_rank=8,
                                  fresh_network_per_video=fresh)
        assert launch.worker(args) == 0
        results[mode] = {v: _mask_bytes(tmp_path / mode / v) for v in ('chair_a', 'chair_b')}
        assert counts['init'] - before == (2 if fresh else 1), mode
        assert all(len(results[mode][v]) == 5 for v in results[mode])
    assert results['shared'] == results['fresh']


# ---- 8. the command line ---------------------------------------------------------------------------------------------------
def test_session_cli_two_rounds(clips, cfg, rov, tmp_path):
    imgs, msks = clips[2]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    p = subprocess.run([sys.executable, '-m', 'xmem2_amd.session', '--images', imgs, '--masks', msks, '--out', str(tmp_path / 'out'),
                        '--rounds', '2', '--k', '2', '--config', json.dumps(cfg)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    rounds = [json.loads(line) for line in p.stdout.splitlines() if line.startswith('{')]
    assert [r['round'] for r in rounds] == [0, 1]
    for r in rounds:
        assert len(r['chosen']) == 2 and not set(r['chosen']) & set(r['references'])
    assert rounds[0]['references'] == [0] and rounds[1]['references'] == sorted([0] + rounds[0]['chosen'])
    assert _mask_bytes(tmp_path / 'out') == rov(2, tuple(rounds[1]['references']))[0]
