"""GPU tests of the test-time ensemble (eval.py --size S [--flip] --save_scores, merged by merge_multi_scale.py):

1. `ops.ensemble_accumulate` bit-identical to the numpy restatement of tests/test_ensemble_host.py applied to `ops.resize_bilinear`;
2. `run_on_video_ensemble` on the chair files against one oracle `RefCore` per pass + the numpy merge;
3. two identical passes on one network give the merged masks of one pass (no shared static buffers, no shared hints);
4. a late object and several objects on a synthetic clip, against the oracle;
5. one network for all passes, no capture in the steady state and no eviction of captured stages."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import cpu_ref as R
from test_ensemble_host import ensemble_merge_reference, interp_reference

pytestmark = pytest.mark.gpu
T = torch.from_numpy
CHAIR = os.path.join(GOLDEN, 'chair')
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


@pytest.fixture(scope='module')
def checkpoint(synth_sd, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt') / 'XMem_synth.pth'
    torch.save(synth_sd, path)
    return str(path)


@pytest.fixture(scope='module')
def checkpoint_mo(synth_sd_mo, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt_mo') / 'XMem_synth_mo.pth'
    torch.save(synth_sd_mo, path)
    return str(path)


# ---- the gates of tests/test_gpu_harness.py::test_run_on_video_resized_vs_oracle, restated ------------------------------------------
def _compare(got, want, what):
    ious = [R.compute_array_iou(got[i], want[i]) for i in range(len(want))]
    n_mism = int((got != want).sum())
    mism = n_mism / want.size
    clip = ((got > 0) & (want > 0)).sum() / max(((got > 0) | (want > 0)).sum(), 1)
    print(f'{what}: clip IoU {clip:.5f}, min frame IoU {min(ious):.5f}, argmax mismatch {n_mism} px = {mism:.2e}')
    assert clip >= 0.999 and min(ious) >= 0.995, f'{what}: IoU {clip:.5f} / {min(ious):.5f}'
    assert mism < 1e-4, f'{what}: mismatch {mism:.2e}'


def _read_written_masks(out_dir, names, ref_png):
    """The harness writes RGB PNGs in the annotation's palette colours: map them back to label ids."""
    from PIL import Image
    pal = np.array(Image.open(ref_png).convert('P').getpalette()[:3 * 256], np.int64).reshape(-1, 3)
    lut = {tuple(c): i for i, c in reversed(list(enumerate(pal.tolist())))}       # lowest index wins
    out = []
    for n in names:
        rgb = np.array(Image.open(os.path.join(out_dir, 'masks', n[:-4] + '.png')).convert('RGB'), np.int64)
        ids = np.full(rgb.shape[:2], 255, np.uint8)
        for c in np.unique(rgb.reshape(-1, 3), axis=0):
            ids[(rgb == c).all(-1)] = lut[tuple(c.tolist())]
        out.append(ids)
    return np.stack(out)


def _link_chair(tmp_path, n):
    names = sorted(os.listdir(os.path.join(CHAIR, 'JPEGImages')))[:n]
    imgs, msks = tmp_path / 'JPEGImages', tmp_path / 'Annotations'
    imgs.mkdir(); msks.mkdir()
    for nm in names:
        os.symlink(os.path.join(CHAIR, 'JPEGImages', nm), imgs / nm)
        os.symlink(os.path.join(CHAIR, 'Annotations', nm[:-4] + '.png'), msks / (nm[:-4] + '.png'))
    return str(imgs), str(msks), names


def _write_synthetic_clip(tmp_path, t, hw, n_obj, annotated):
    """Frames of xmem2_amd.synth as PNG files; index-mask PNGs for the `annotated` frames: {frame: number of objects in it}."""
    from PIL import Image
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    imgs, msks = tmp_path / 'JPEGImages', tmp_path / 'Annotations'
    imgs.mkdir(); msks.mkdir()
    frames, masks = synthetic_frames(t, *hw), synthetic_masks(t, n_obj, *hw)
    palette = [0, 0, 0, 200, 0, 0, 0, 200, 0, 0, 0, 200] + [0] * (256 * 3 - 12)
    names = [f'frame_{i:06d}.png' for i in range(t)]
    for i in range(t):
        rgb = np.clip((frames[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(imgs / names[i])
        if i in annotated:
            idx = np.zeros(hw, np.uint8)
            for k in range(annotated[i]):
                idx[masks[i, k] > 0] = k + 1
            im = Image.fromarray(idx, mode='P'); im.putpalette(palette); im.save(msks / names[i])
    return str(imgs), str(msks), names


def _oracle_ensemble(ref_net, cfg, imgs, msks, names, passes, fm):
    """What eval.py --size S [--flip] --save_scores + merge_multi_scale.py compute, with the oracle's RefCore per pass, driven the way
    run_on_video drives a core (all annotated frames preloaded into permanent memory, then the loop); inputs are the same decoded,
    PIL-resized, mirrored arrays; masks mirrored BEFORE convert_mask and the nearest resize (eval.py:191-200)."""
    from PIL import Image
    pil = [Image.open(os.path.join(imgs, n)).convert('RGB') for n in names]
    H, W = pil[0].size[1], pil[0].size[0]
    raw = {j: np.array(Image.open(os.path.join(msks, names[j][:-4] + '.png')).convert('P'), np.uint8) for j in fm}
    fm = sorted(fm)
    per_pass, mappers = [], []
    for s, flip in passes:
        if s < 0:
            work = (H, W)
        else:
            sc = s / min(H, W)
            work = (s, int(W * sc)) if H <= W else (int(H * sc), s)

        def rgb(i, work=work, flip=flip):
            im = pil[i] if work == (H, W) else pil[i].resize((work[1], work[0]), Image.BILINEAR)
            a = np.array(im, np.uint8)
            if flip:
                a = np.ascontiguousarray(a[:, ::-1])
            x = T(a).permute(2, 0, 1).to(torch.float32).div(255)
            return ((x - T(MEAN)[:, None, None]) / T(STD)[:, None, None]).contiguous()

        core, mapper = R.RefCore(ref_net, cfg), R.RefMaskMapper()

        def mask(j, work=work, flip=flip, mapper=mapper):
            m = np.ascontiguousarray(raw[j][:, ::-1]) if flip else raw[j]
            msk, labels = mapper.convert_mask(m, exhaustive=True)
            msk = torch.Tensor(msk)
            if work != (H, W):                                      # video_reader.py:148-153: nearest
                msk = torch.nn.functional.interpolate(msk.unsqueeze(0), work, mode='nearest')[0]
            return msk, labels

        for j in fm:
            msk, _ = mask(j)
            core.set_all_labels(list(mapper.remappings.values()))
            core.put_to_permanent_memory(rgb(j), msk)
        scores = []
        for ti in range(len(names)):
            msk = labels = None
            if ti in fm:
                msk, labels = mask(ti)
                core.set_all_labels(list(mapper.remappings.values()))
            p = core.step(rgb(ti), msk, labels, end=(ti == len(names) - 1), do_not_add_mask_to_memory=(msk is not None))
            scores.append(interp_reference(p.numpy(), (H, W)))
        per_pass.append(scores)
        mappers.append(mapper)
    for m in mappers[1:]:
        assert m.remappings == mappers[0].remappings
    want = []
    for ti in range(len(names)):
        _, merged = ensemble_merge_reference([sc[ti] for sc in per_pass], [f for _, f in passes])
        want.append(mappers[0].remap_index_mask(merged))
    return np.stack(want)


def _oracle_cfg(over, n_frames):
    from xmem2_amd.configuration import VIDEO_INFERENCE_CONFIG
    cfg = dict(VIDEO_INFERENCE_CONFIG); cfg.update(over)
    cfg['enable_long_term_count_usage'] = (cfg['enable_long_term'] and                      # run_on_video.py:190-196
                                           n_frames / (cfg['max_mid_term_frames'] - cfg['min_mid_term_frames']) * cfg['num_prototypes']
                                           >= cfg['max_long_term_elements'])
    return cfg


# ---- 1. the merge kernel ------------------------------------------------------------------------------------------------------------
def _boundary_probs(C, hw, seed):
    """Random per-pixel-normalised probabilities with injected boundary values: one-hot pixels (p = 1.0), exact ties between channels,
    and channel 0 exactly at k/255 (the rest shared evenly)."""
    g = np.random.default_rng(seed)
    p = g.random((C,) + hw, dtype=np.float32) + np.float32(1e-3)
    p /= p.sum(0, keepdims=True)
    H, W = hw
    sel = g.random(hw) < 0.05
    p[:, sel] = 0.0
    p[g.integers(0, C), sel] = 1.0
    tie = g.random(hw) < 0.05
    p[:, tie] = np.float32(1.0 / C)
    kk = g.random(hw) < 0.05
    k = g.integers(0, 256, size=int(kk.sum())).astype(np.float32)
    p[0, kk] = (k / np.float32(255)).astype(np.float32)
    p[1:, kk] = ((1 - p[0, kk]) / np.float32(C - 1))[None]
    return np.ascontiguousarray(p, dtype=np.float32)


KERNEL_CASES = [
    # (C, original H x W, working sizes cycled over the passes, passes)
    (2, (480, 720), [(480, 720), (600, 900), (240, 360)], 6),
    (6, (480, 720), [(600, 900), (480, 720), (240, 360)], 4),
    (6, (128, 171), [(97, 131), (128, 171), (64, 86), (200, 285)], 16),
    (2, (128, 171), [(97, 131)], 16),
]


@pytest.mark.parametrize('C,hw,sizes,n_pass', KERNEL_CASES, ids=[f'C{c[0]}_{c[1][0]}x{c[1][1]}_{c[3]}p' for c in KERNEL_CASES])
def test_ensemble_accumulate_bit_exact(C, hw, sizes, n_pass):
    from xmem2_amd import ops
    H, W = hw
    acc = torch.empty((C, H, W), dtype=torch.uint16, device='cuda')
    out = torch.full((H, W), 77, dtype=torch.uint8, device='cuda')
    scores, mirrors = [], []
    for i in range(n_pass):
        work = sizes[i % len(sizes)]
        mirror = bool((i // len(sizes)) % 2) if len(sizes) > 1 else bool(i % 2)     # every size both ways
        prob = T(_boundary_probs(C, work, seed=1000 * C + i)).cuda()
        last = i == n_pass - 1
        res = ops.ensemble_accumulate(prob, (H, W), mirror, acc, first=(i == 0), out=out if last else None)
        assert res is (out if last else acc)
        resized = ops.resize_bilinear(prob, (H, W)) if work != (H, W) else prob
        scores.append(resized.cpu().numpy()); mirrors.append(mirror)
        want_acc, want_mask = ensemble_merge_reference(scores, mirrors)
        got_acc = acc.cpu().numpy()
        assert got_acc.dtype == np.uint16
        bad = int((got_acc != want_acc).sum())
        assert bad == 0, f'pass {i} ({work}, mirror={mirror}): {bad} accumulator values differ'
        if not last:
            assert int((out.cpu().numpy() != 77).sum()) == 0, 'out written by a pass that does not close the frame'
    got_mask = out.cpu().numpy()
    assert np.array_equal(got_mask, want_mask), f'{int((got_mask != want_mask).sum())} merged labels differ'


def test_ensemble_accumulate_rejects_wrong_buffers():
    from xmem2_amd import ops
    prob = torch.rand(2, 8, 8, device='cuda')
    with pytest.raises(RuntimeError):
        ops.ensemble_accumulate(prob, (8, 8), False, torch.empty((2, 8, 8), dtype=torch.int16, device='cuda'), True)
    with pytest.raises(RuntimeError):
        ops.ensemble_accumulate(prob, (8, 8), False, torch.empty((3, 8, 8), dtype=torch.uint16, device='cuda'), True)
    with pytest.raises(RuntimeError):
        ops.ensemble_accumulate(prob, (8, 8), False, torch.empty((2, 8, 8), dtype=torch.uint16, device='cuda'), True,
                                out=torch.empty((8, 8), dtype=torch.uint8))


# ---- 2. chair clip against the oracle -------------------------------------------------------------------------------------------
CHAIR_PASSES = [[480, False], [480, True], [600, False], [600, True]]


def test_ensemble_chair_vs_oracle(checkpoint, ref_net, tmp_path):
    from xmem2_amd.run_on_video import run_on_video, run_on_video_ensemble
    imgs, msks, names = _link_chair(tmp_path, 6)
    over = {'model': checkpoint, 'mem_every': 2}
    out = tmp_path / 'ens'
    stats = run_on_video_ensemble(imgs, msks, str(out), frames_with_masks=[0], compute_iou=True, print_progress=False,
                                  overwrite_config=dict(over, ensemble=CHAIR_PASSES))
    single = run_on_video(imgs, msks, str(tmp_path / 'single'), frames_with_masks=[0], compute_iou=True, print_progress=False,
                          overwrite_config=dict(over))
    assert list(stats.columns) == list(single.columns)
    assert list(stats['frame']) == names == list(single['frame'])
    assert list(stats['mask_provided']) == list(single['mask_provided'])
    assert stats['iou'][0] == -1 and all(0.0 <= v <= 1.0 for v in stats['iou'][1:])
    assert sorted(os.listdir(out / 'masks')) == [n[:-4] + '.png' for n in names] and len(os.listdir(out / 'overlay')) == len(names)
    got = _read_written_masks(str(out), names, os.path.join(msks, names[0][:-4] + '.png'))
    want = _oracle_ensemble(ref_net, _oracle_cfg(over, len(names)), imgs, msks, names,
                            [tuple(p) for p in CHAIR_PASSES], [0])
    assert got.shape == want.shape == (6, 480, 720)
    _compare(got, want, 'chair ensemble {480, 600} x flip')


# ---- 3. passes are independent --------------------------------------------------------------------------------------------------
def test_duplicate_passes_equal_one_pass(checkpoint, tmp_path):
    from xmem2_amd.run_on_video import run_on_video_ensemble
    imgs, msks, names = _link_chair(tmp_path, 6)
    ref_png = os.path.join(msks, names[0][:-4] + '.png')
    got = {}
    for tag, passes in (('one', [[480, False]]), ('two', [[480, False], [480, False]])):
        out = tmp_path / tag
        run_on_video_ensemble(imgs, msks, str(out), frames_with_masks=[0], print_progress=False,
                              overwrite_config={'model': checkpoint, 'mem_every': 2, 'ensemble': passes})
        got[tag] = _read_written_masks(str(out), names, ref_png)
    n = int((got['one'] != got['two']).sum())
    print(f'duplicate passes: {n} labels differ from one pass')
    assert n == 0


# ---- 4. late object, several objects ---------------------------------------------------------------------------------------------
def test_ensemble_late_object_vs_oracle(checkpoint_mo, ref_net_mo, tmp_path):
    from xmem2_amd.run_on_video import run_on_video_ensemble
    t, hw = 8, (96, 128)
    imgs, msks, names = _write_synthetic_clip(tmp_path, t, hw, 3, {0: 2, 3: 3})
    passes = [[96, False], [96, True], [128, False], [128, True]]      # native-size passes and 128 x 170 passes
    over = {'model': checkpoint_mo, 'mem_every': 2}
    out = tmp_path / 'out'
    stats = run_on_video_ensemble(imgs, msks, str(out), frames_with_masks=[0, 3], print_progress=False,
                                  overwrite_config=dict(over, ensemble=passes))
    assert list(stats['mask_provided']) == [i in (0, 3) for i in range(t)]
    got = _read_written_masks(str(out), names, os.path.join(msks, names[0][:-4] + '.png'))
    want = _oracle_ensemble(ref_net_mo, _oracle_cfg(over, t), imgs, msks, names, [tuple(p) for p in passes], [0, 3])
    _compare(got, want, 'late object, 3 objects, {96, 128} x flip')


# ---- 5. one network, steady state --------------------------------------------------------------------------------------------------
def _spied_run(monkeypatch, run, n_pass):
    """Run `run()` with spies on XMem.__init__, stage captures (a new entry in the network's stage cache), XMem._evict_lru and
    InferenceCore.step; captures are binned by the frame of the latest step() begun (-1: before the first one - the preload and the
    first key hints; the hints of a later key batch land in the frame before it, in every run alike)."""
    from xmem2_amd import inference_core, network
    nets, captures, evictions, steps = [], {}, [], [0]           # steps: step() calls begun
    init, run_stage, evict, step = network.XMem.__init__, network.XMem._run_stage, network.XMem._evict_lru, inference_core.InferenceCore.step

    def init_spy(self, *a, **k):
        nets.append(self)
        return init(self, *a, **k)

    def run_stage_spy(self, *a, **k):
        n0 = len(self._stages)
        r = run_stage(self, *a, **k)
        if len(self._stages) > n0:
            f = (steps[0] - 1) // n_pass if steps[0] else -1
            captures[f] = captures.get(f, 0) + len(self._stages) - n0
        return r

    def evict_spy(self):
        evictions.append(len(self._stages))
        return evict(self)

    def step_spy(self, *a, **k):
        steps[0] += 1
        return step(self, *a, **k)

    with monkeypatch.context() as m:
        m.setattr(network.XMem, '__init__', init_spy)
        m.setattr(network.XMem, '_run_stage', run_stage_spy)
        m.setattr(network.XMem, '_evict_lru', evict_spy)
        m.setattr(inference_core.InferenceCore, 'step', step_spy)
        run()
    return nets, captures, evictions


def test_one_network_no_steady_state_capture(checkpoint, tmp_path, monkeypatch):
    from xmem2_amd.network import MAX_STAGES
    from xmem2_amd.run_on_video import run_on_video_ensemble
    t, hw = 12, (96, 128)
    imgs, msks, names = _write_synthetic_clip(tmp_path, t, hw, 1, {0: 1})
    passes = [[96, False], [96, True], [128, False], [128, True]]
    runs = {}
    for tag, ps in (('one', passes[:1]), ('four', passes)):
        runs[tag] = _spied_run(monkeypatch, lambda ps=ps, tag=tag: run_on_video_ensemble(
            imgs, msks, str(tmp_path / tag), frames_with_masks=[0], print_progress=False,
            overwrite_config={'model': checkpoint, 'mem_every': 4, 'ensemble': ps}), len(ps))
    nets, captures, evictions = runs['four']
    per_frame = [captures.get(f, 0) for f in range(t)]
    single = [runs['one'][1].get(f, 0) for f in range(t)]
    print(f'4 passes: {len(nets[0]._stages)} captured stages (MAX_STAGES {MAX_STAGES}); captures by frame {per_frame} '
          f'(preload {captures.get(-1, 0)}); one pass: {single} (preload {runs["one"][1].get(-1, 0)}); evictions {evictions}')
    assert len(nets) == 1, f'{len(nets)} XMem instances for one ensemble'
    assert not evictions, f'captured stages evicted at {evictions} (MAX_STAGES = {MAX_STAGES})'
    # every pass captures what one pass alone captures, at the same frames: nothing is re-captured because the passes share a network
    assert per_frame == [len(passes) * c for c in single]
    # the key-batch groups and their slots are all captured within the first key batches: frames 9 and 10 replay only
    assert per_frame[9] == per_frame[10] == 0
