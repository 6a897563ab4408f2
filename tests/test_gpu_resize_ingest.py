"""Frame ingest on the device: the working-size resize of decoded frames by `ops.resize_u8` (csrc/resize_u8.hip).

The kernel restates the host library's 8-bit antialiased bilinear resize in its own integer arithmetic, so everything here is checked by
EQUALITY, not by a tolerance:

1. `ops.resize_u8` against Pillow, byte for byte;
2. `InferenceCore.prefetch_keys(..., working_size=...)`: same tensors, same probabilities, nothing on the caller's stream;
3. `run_on_video` with `resize_on_device` on and off: the same written masks (also with the augmented preload);
4. `run_on_video_ensemble` likewise, and one upload per frame;
5. `select_k_next_best_annotation_candidates` picks the same frames."""
import os

import numpy as np
import pytest
import torch

from test_gpu_ensemble import _read_written_masks, _write_synthetic_clip

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _pillow(a, th, tw, flip=False):
    from PIL import Image
    r = np.array(Image.fromarray(a).resize((tw, th), Image.BILINEAR), dtype=np.uint8)
    return np.ascontiguousarray(r[:, ::-1]) if flip else r


def _images(hw, seed):
    g = np.random.default_rng(seed)
    return {'noise': g.integers(0, 256, size=hw + (3,), dtype=np.uint8),
            'binary': (g.integers(0, 2, size=hw + (3,), dtype=np.uint8) * 255).astype(np.uint8)}


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [
    ((37, 53), (16, 22)),         # both axes down, odd sizes
    ((16, 22), (37, 53)),         # both axes up, 3 taps
    ((5, 7), (5, 3)),             # one axis only
    ((1, 9), (4, 3)),             # a single source row
    ((100, 100), (1, 1)),         # 201 taps
    ((216, 384), (48, 85)),       # ratio 4.5: the tap count of 2160p -> 480p
    ((270, 480), (120, 213)),     # ratio 2.25: 1080p -> 480p
    ((96, 128), (96, 128)),       # copy, and mirror with flip
]


@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
@pytest.mark.parametrize('src,dst', KERNEL_CASES, ids=[f'{s[0]}x{s[1]}_to_{d[0]}x{d[1]}' for s, d in KERNEL_CASES])
def test_resize_u8_equals_pillow(src, dst, flip):
    from xmem2_amd import ops
    for kind, a in _images(src, seed=src[1] * 977 + dst[0]).items():
        want = _pillow(a, *dst, flip=flip)
        dev = T(a).cuda()
        got = ops.resize_u8(dev, dst, flip=flip)
        assert got.dtype == torch.uint8 and tuple(got.shape) == dst + (3,) and got.is_contiguous()
        bad = int((got.cpu().numpy() != want).sum())
        assert bad == 0, f'{kind}: {bad} of {want.size} bytes differ from Pillow'
        assert np.array_equal(dev.cpu().numpy(), a), 'the source frame is read only'


@pytest.mark.parametrize('src,dst', KERNEL_CASES[:2], ids=['down', 'up'])
def test_resize_u8_into_a_frame_of_a_batch_buffer(src, dst):
    from xmem2_amd import ops
    a = _images(src, seed=11)['noise']
    batch = torch.full((3,) + dst + (3,), 7, dtype=torch.uint8, device='cuda')
    res = ops.resize_u8(T(a).cuda(), dst, out=batch[1])
    assert res.data_ptr() == batch[1].data_ptr()
    got = batch.cpu().numpy()
    assert np.array_equal(got[1], _pillow(a, *dst))
    assert (got[0] == 7).all() and (got[2] == 7).all(), 'the neighbouring frames of the batch buffer were written'


def test_resize_u8_rejects_wrong_tensors():
    from xmem2_amd import ops
    ok = torch.zeros((8, 10, 3), dtype=torch.uint8, device='cuda')
    for bad in (ok.float(),                                                  # dtype
                torch.zeros((3, 8, 10), dtype=torch.uint8, device='cuda'),   # channels first
                torch.zeros((8, 10), dtype=torch.uint8, device='cuda'),      # no channel axis
                torch.zeros((8, 10, 4), dtype=torch.uint8, device='cuda'),   # RGBA
                ok.cpu(),                                                    # host tensor
                torch.zeros((8, 20, 3), dtype=torch.uint8, device='cuda')[:, ::2]):   # not contiguous
        with pytest.raises(RuntimeError):
            ops.resize_u8(bad, (4, 5))
    for out in (torch.zeros((4, 6, 3), dtype=torch.uint8, device='cuda'),    # shape
                torch.zeros((4, 5, 3), dtype=torch.int8, device='cuda'),     # dtype
                torch.zeros((4, 5, 3), dtype=torch.uint8),                   # host
                torch.zeros((4, 10, 3), dtype=torch.uint8, device='cuda')[:, ::2]):   # not contiguous
        with pytest.raises(RuntimeError):
            ops.resize_u8(ok, (4, 5), out=out)
    with pytest.raises(RuntimeError):
        ops.resize_u8(ok, (0, 5))
    with pytest.raises(RuntimeError):
        ops.resize_u8(ok, (8, 10), flip=True, out=ok)                        # in place
    base = torch.zeros(400, dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError):
        ops.resize_u8(base[:240].view(8, 10, 3), (4, 5), out=base[200:260].view(4, 5, 3))   # out overlaps the tail of the input
    with pytest.raises(RuntimeError, match='status -2'):
        ops.resize_u8(ok, (4, 16385))                                        # beyond the supported side


# ---- 2. prefetch_keys with a working size -------------------------------------------------------------------------------------------
SRC_HW, WORK_HW = (150, 200), (96, 128)


def _source_frames(t, seed=1234):
    """uint8 H x W x 3 frames of the synthetic clip at the source size, as the clip writer quantises them"""
    from xmem2_amd.synth import synthetic_frames
    f = synthetic_frames(t, *SRC_HW, seed=seed)
    return [np.ascontiguousarray(np.clip((f[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)) for i in range(t)]


class _StreamSpy:
    """Records the stream every image-side launch and every host-to-device copy of a frame runs on."""

    def __init__(self, monkeypatch):
        from xmem2_amd import ops
        self.launches, self.uploads = [], []
        resize, pack, to = ops.resize_u8, ops.pack_image_u8, torch.Tensor.to

        def resize_spy(*a, **k):
            self.launches.append(('resize_u8', torch.cuda.current_stream().cuda_stream))
            return resize(*a, **k)

        def pack_spy(*a, **k):
            self.launches.append(('pack_image_u8', torch.cuda.current_stream().cuda_stream))
            return pack(*a, **k)

        def to_spy(t, *a, **k):
            if not t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3:
                self.uploads.append((tuple(t.shape), torch.cuda.current_stream().cuda_stream))
            return to(t, *a, **k)

        monkeypatch.setattr(ops, 'resize_u8', resize_spy)
        monkeypatch.setattr(ops, 'pack_image_u8', pack_spy)
        monkeypatch.setattr(torch.Tensor, 'to', to_spy)


@pytest.mark.parametrize('where', ['pinned', 'device'])
def test_prefetch_keys_resizes_on_the_side_stream(hip_net, monkeypatch, where):
    from conftest import base_config
    from xmem2_amd import ops
    from xmem2_amd.inference_core import InferenceCore
    from xmem2_amd.synth import synthetic_masks
    t = 5
    src = _source_frames(t)
    host_resized = [T(_pillow(a, *WORK_HW)).cuda() for a in src]
    mask0 = T(synthetic_masks(1, 1, *WORK_HW)[0]).cuda()
    cfg = base_config(mem_every=10 ** 9)
    torch.cuda.synchronize()

    def run(make_hint):
        core = InferenceCore(hip_net, cfg)
        core.set_all_labels([1])
        core.put_to_permanent_memory(host_resized[0], mask0)
        devs = make_hint(core)
        probs = [core.step(d, None, None).clone() for d in devs]
        core.cancel_prefetch()
        return devs, probs

    _, want = run(lambda core: core.prefetch_keys(host_resized[1:], inputs_complete=True))

    inputs = [T(a).pin_memory() if where == 'pinned' else T(a).cuda() for a in src[1:]]
    torch.cuda.synchronize()
    main = torch.cuda.current_stream().cuda_stream
    with monkeypatch.context() as m:
        spy = _StreamSpy(m)
        devs, got = run(lambda core: core.prefetch_keys(inputs, working_size=WORK_HW))
    for i, d in enumerate(devs):
        assert d.is_cuda and d.dtype == torch.uint8 and tuple(d.shape) == WORK_HW + (3,)
        assert torch.equal(d, ops.resize_u8(T(src[i + 1]).cuda(), WORK_HW)), f'frame {i + 1}: not the resize of the source frame'
        assert torch.equal(d, host_resized[i + 1]), f'frame {i + 1}: not the host resize'
    for i, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), f'frame {i + 1}: probabilities differ from the host-resized stream (max {float((a - b).abs().max()):.2e})'
    # the source frames are copied, resized and packed on the side stream only (the preload's pack is the one main-stream launch)
    hinted = [(k, s) for k, s in spy.launches if not (k == 'pack_image_u8' and s == main)]
    assert sum(k == 'resize_u8' for k, _ in spy.launches) == t - 1
    assert len([1 for k, s in spy.launches if k == 'pack_image_u8' and s == main]) == 1, 'only the preload packs on the main stream'
    assert len(hinted) == 2 * (t - 1) and all(s != main for _, s in hinted), f'image-side launches on the main stream: {spy.launches}'
    if where == 'pinned':
        assert [shape for shape, _ in spy.uploads] == [SRC_HW + (3,)] * (t - 1)
        assert all(s != main for _, s in spy.uploads), 'a source frame was copied on the main stream'


def test_prefetch_keys_mirrors_and_passes_through(hip_net):
    """flip makes the mirrored variant; a frame that already has the working size and is not mirrored is handed on as it is."""
    from conftest import base_config
    from xmem2_amd.inference_core import InferenceCore
    src = _source_frames(2)
    core = InferenceCore(hip_net, base_config())
    dev = [T(a).cuda() for a in src]
    torch.cuda.synchronize()
    same = core.prefetch_keys(dev, working_size=SRC_HW)
    assert [d.data_ptr() for d in same] == [d.data_ptr() for d in dev]
    core.cancel_prefetch()
    flipped = core.prefetch_keys(dev, working_size=WORK_HW, flip=True)
    core.cancel_prefetch()
    torch.cuda.synchronize()
    for a, d in zip(src, flipped):
        assert np.array_equal(d.cpu().numpy(), _pillow(a, *WORK_HW, flip=True))
    with pytest.raises(ValueError):
        core.prefetch_keys(dev, flip=True)


# ---- 3. - 5. the harness on a synthetic clip ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def checkpoint_mo(synth_sd_mo, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt_resize') / 'XMem_synth_mo.pth'
    torch.save(synth_sd_mo, path)
    return str(path)


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    """6 PNG frames of 150 x 200, 2 objects, frame 0 annotated"""
    return _write_synthetic_clip(tmp_path_factory.mktemp('clip_resize'), 6, SRC_HW, 2, {0: 2})


def _link_first(tmp_path, clip, n):
    imgs, msks, names = clip
    di, dm = tmp_path / 'JPEGImages', tmp_path / 'Annotations'
    di.mkdir(); dm.mkdir()
    for nm in names[:n]:
        os.symlink(os.path.join(imgs, nm), di / nm)
    os.symlink(os.path.join(msks, names[0]), dm / names[0])
    return str(di), str(dm), names[:n]


class _CoreSpy:
    """Records what every core is fed and what it answers: the image of each `put_to_permanent_memory` and `step` call (kept by
    reference and read after the run - at the call a hinted frame may still be in flight on the side stream) and a clone of each
    step's probabilities.  The written masks alone would not do: the synthetic checkpoint loses the objects after the annotated frame on
    this small clip, so most masks are empty whatever the frames hold, while the probabilities are functions of every frame's bytes
    and - through the memory readout - of every preloaded frame's bytes."""

    def __init__(self, monkeypatch):
        from xmem2_amd.inference_core import InferenceCore
        self.calls = []
        step, put = InferenceCore.step, InferenceCore.put_to_permanent_memory

        def step_spy(core, image, *a, **k):
            prob = step(core, image, *a, **k)
            self.calls.append(('step', image, prob.clone()))
            return prob

        def put_spy(core, image, *a, **k):
            self.calls.append(('perm', image, None))
            return put(core, image, *a, **k)

        monkeypatch.setattr(InferenceCore, 'step', step_spy)
        monkeypatch.setattr(InferenceCore, 'put_to_permanent_memory', put_spy)

    def host(self):
        torch.cuda.synchronize()
        return [(kind, img.cpu().numpy(), None if prob is None else prob.cpu().numpy()) for kind, img, prob in self.calls]


def _same_feed_and_answers(on, off):
    """Every image handed to a core is the same bytes with the option on and off, and every step answers with the same bits."""
    assert [k for k, _, _ in on] == [k for k, _, _ in off]
    for i, ((kind, a, p), (_, b, q)) in enumerate(zip(on, off)):
        assert a.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b), \
            f'call {i} ({kind}): the device-resized frame differs from the host-resized one ({a.shape} vs {b.shape})'
        if kind == 'step':
            assert p.shape == q.shape and np.array_equal(p, q), f'call {i}: probabilities differ (max {np.abs(p - q).max():.2e})'


def _decoded(imgs, names):
    from PIL import Image
    return [np.array(Image.open(os.path.join(imgs, n)).convert('RGB'), dtype=np.uint8) for n in names]


@pytest.mark.parametrize('augment', [False, True], ids=['plain', 'augmented_preload'])
def test_run_on_video_same_masks_with_device_resize(checkpoint_mo, clip, tmp_path, monkeypatch, augment):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = _link_first(tmp_path, clip, 3) if augment else clip
    ref_png = os.path.join(msks, names[0])
    got, stats, calls = {}, {}, {}
    for tag, on in (('off', False), ('on', True)):
        out = tmp_path / tag
        with monkeypatch.context() as m:
            spy = _CoreSpy(m)
            stats[tag] = run_on_video(imgs, msks, str(out), frames_with_masks=[0], compute_iou=True, print_progress=False,
                                      augment_images_with_masks=augment, save_overlay=False,
                                      overwrite_config={'model': checkpoint_mo, 'size': 96, 'mem_every': 2, 'resize_on_device': on})
            calls[tag] = spy.host()
        got[tag] = _read_written_masks(str(out), names, ref_png)
    assert got['off'].shape == (len(names),) + SRC_HW
    n = int((got['on'] != got['off']).sum())
    assert n == 0, f'{n} mask pixels differ between the device and the host resize'
    assert stats['on'].equals(stats['off']) and list(stats['on']['frame']) == names
    # the masks are mostly empty on this clip (see _CoreSpy): what the comparison rests on is the feed and the probabilities
    perm = [c for c in calls['on'] if c[0] == 'perm']
    steps = [c for c in calls['on'] if c[0] == 'step']
    assert len(perm) == (12 if augment else 1) and len(steps) == len(names)          # the frame and its 11 'best_all' augmentations
    decoded = _decoded(imgs, names)
    for i, (_, img, prob) in enumerate(steps):
        assert np.array_equal(img, _pillow(decoded[i], *WORK_HW)), f'frame {i}: the core was not fed the Pillow resize of the file'
        assert prob.shape[1:] == WORK_HW
    assert np.array_equal(perm[0][1], _pillow(decoded[0], *WORK_HW))
    if augment:
        assert all(a[1].shape == WORK_HW + (3,) for a in perm)
        assert len({a[1].tobytes() for a in perm}) >= 6, 'the augmented preload frames must differ from each other'
    _same_feed_and_answers(calls['on'], calls['off'])
    # ... and the probabilities do see the frames: no two steps answer alike
    assert len({p.tobytes() for _, _, p in steps[1:]}) == len(names) - 1, 'the probabilities do not tell the frames apart'


ENSEMBLE_PASSES = [[96, False], [96, True], [-1, True], [128, False]]
ENSEMBLE_HW = [WORK_HW, WORK_HW, SRC_HW, (128, 170)]


def test_ensemble_same_masks_and_one_upload_per_frame(checkpoint_mo, clip, tmp_path, monkeypatch):
    from xmem2_amd.run_on_video import run_on_video_ensemble
    imgs, msks, names = clip
    ref_png = os.path.join(msks, names[0])
    got, stats, uploads, calls = {}, {}, {}, {}
    for tag, on in (('off', False), ('on', True)):
        out = tmp_path / tag
        with monkeypatch.context() as m:
            spy, cores = _StreamSpy(m), _CoreSpy(m)
            stats[tag] = run_on_video_ensemble(imgs, msks, str(out), frames_with_masks=[0], print_progress=False, save_overlay=False,
                                               overwrite_config={'model': checkpoint_mo, 'mem_every': 2, 'ensemble': ENSEMBLE_PASSES,
                                                                 'resize_on_device': on})
            calls[tag] = cores.host()
        uploads[tag] = [shape for shape, _ in spy.uploads]
        got[tag] = _read_written_masks(str(out), names, ref_png)
    n = int((got['on'] != got['off']).sum())
    assert n == 0, f'{n} merged mask pixels differ between the device and the host resize'
    assert stats['on'].equals(stats['off'])
    # on: every frame goes up once at the source size (frame 0 once more for the preload), and nothing else does;
    # off: one upload per pass and frame, each at its own working size
    assert uploads['on'] == [SRC_HW + (3,)] * (len(names) + 1), uploads['on']
    assert len(uploads['off']) == len(ENSEMBLE_PASSES) * (len(names) + 1)
    # every pass of every frame is fed its own variant - the Pillow resize of the file, mirrored for a flipped pass - and the
    # probabilities (which, unlike the mostly empty masks of this clip, depend on every frame's bytes) are the same bits
    P = len(ENSEMBLE_PASSES)
    perm = [c for c in calls['on'] if c[0] == 'perm']
    steps = [c for c in calls['on'] if c[0] == 'step']
    assert len(perm) == P and len(steps) == P * len(names)
    decoded = _decoded(imgs, names)
    for i, (_, img, prob) in enumerate(perm + steps):
        f, p = max(i - P, 0) // P, i % P                                   # the preload feeds frame 0, pass by pass
        want = _pillow(decoded[f], *ENSEMBLE_HW[p], flip=ENSEMBLE_PASSES[p][1])
        assert img.shape == want.shape and np.array_equal(img, want), f'frame {f}, pass {ENSEMBLE_PASSES[p]}: not the variant of the file'
    _same_feed_and_answers(calls['on'], calls['off'])
    assert len({p.tobytes() for _, _, p in steps[P:]}) == P * (len(names) - 1), 'the probabilities do not tell frames and passes apart'


def test_select_k_same_candidates_with_device_resize(checkpoint_mo, clip, tmp_path):
    """Same candidates, and the same per-iteration scores bit for bit, with the option on and off.  The synthetic checkpoint loses the
    objects after the annotated frame on this small clip (5 of 6 predicted masks are empty), and the default mask-presence test then zeroes
    every score but frame 0's - the comparison would not see the frames at all.  `min_mask_presence_percent=0` keeps every frame a
    candidate, so the scores are functions of the keys of all six resized frames: a single differing byte of a resized frame shows."""
    from xmem2_amd.frame_selection import select_next_candidates
    from xmem2_amd.run_on_video import select_k_next_best_annotation_candidates
    imgs, msks, names = clip
    picked, scores = {}, {}
    for tag, on in (('off', False), ('on', True)):
        picked[tag] = select_k_next_best_annotation_candidates(
            imgs, msks, str(tmp_path / tag), k=2, print_progress=False, previously_chosen_candidates=[0],
            use_previously_predicted_masks=False, save_overlay=False, min_mask_presence_percent=0.0,
            overwrite_config={'model': checkpoint_mo, 'size': 96, 'mem_every': 2, 'resize_on_device': on})
        scores[tag] = [s.copy() for s in select_next_candidates.last_scores]
    print('candidates', picked, 'scores of the first iteration', scores['off'][0])
    # a frame's dissimilarity to itself is the smallest there is: new candidates are new, distinct frames
    assert len(set(picked['off'])) == 2 and all(0 < p < len(names) for p in picked['off'])
    assert len(np.unique(scores['off'][0])) == len(names), 'the scores do not tell the frames apart'
    assert picked['on'] == picked['off']
    assert len(scores['on']) == len(scores['off']) == 2
    for a, b in zip(scores['on'], scores['off']):
        assert np.array_equal(a, b), f'scores differ between the device and the host resize: {a} vs {b}'
