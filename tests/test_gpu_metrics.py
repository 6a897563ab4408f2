"""GPU tests of DAVIS J&F (`xmem_jf_counts`, xmem2_amd/metrics.py, compute_jf in the video loop, the launcher's --compute-jf):

1. the kernel's counts equal the numpy restatement of tests/test_metrics_host.py exactly, over random label maps, shapes 1x1 ... 300x517,
   radii 0 ... 63, 1-12 labels, with and without the LUT;
2. batched_jaccard / batched_f_measure equal the reference's values in tests/golden/jf.npz bit for bit;
3. compute_metrics over PNG files equals the reference's per-video means;
4. run_on_video / run_on_video_ensemble with compute_jf=True on the chair clip agree with scoring the masks they wrote;
5. compute_jf is off by default; the launcher's --compute-jf fills summary.json."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_metrics_host import golden_cases, jf_counts_reference

pytestmark = pytest.mark.gpu
CHAIR = os.path.join(GOLDEN, 'chair')
DEFAULT_CASES = ('multi', 'late_vanish', 'empty_pred', 'absent_void', 'odd', 'row_1xW', 'col_Hx1', 'tiny_2x2', 'p480', 'p1080',
                 'chair_shift', 'chair_erode')


@pytest.fixture(scope='module')
def checkpoint(synth_sd, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt') / 'XMem_synth.pth'
    torch.save(synth_sd, path)
    return str(path)


def _random_labels(rng, shape, ids, kind):
    H, W = shape
    if kind == 'noise':                                             # every pixel its own coin: boundaries everywhere
        return rng.choice(np.r_[[0], ids].astype(np.uint8), size=shape)
    yy, xx = np.mgrid[:H, :W]
    lab = np.zeros(shape, np.uint8)
    for k in ids:
        for _ in range(2):
            cy, cx = rng.uniform(-0.2, 1.2) * H, rng.uniform(-0.2, 1.2) * W
            ry, rx = rng.uniform(0.05, 0.5) * H + 0.6, rng.uniform(0.05, 0.5) * W + 0.6
            lab[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = k
    if kind == 'blobs_void':
        lab[rng.random(shape) < 0.02] = 255
    return lab


SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (3, 130), (63, 65), (64, 64), (65, 129), (128, 200), (131, 64), (300, 517)]
RADII = [0, 1, 7, 8, 18, 63]


def test_kernel_counts_equal_the_restatement():
    from xmem2_amd import ops
    rng = np.random.default_rng(7)
    n = 0
    for si, shape in enumerate(SHAPES):
        for ri, r in enumerate(RADII):
            if shape == (300, 517) and r not in (8, 63):
                continue
            nl = int(rng.integers(1, 13))
            ids = rng.choice(np.arange(1, 255), size=nl, replace=False)
            kind = ('blobs', 'noise', 'blobs_void')[(si + ri) % 3]
            B = 1 + (si + ri) % 3
            gt = np.stack([_random_labels(rng, shape, ids, kind) for _ in range(B)])
            use_lut = (si + ri) % 2 == 1
            if use_lut:                                             # pred in dense ids 1..nl, the LUT maps them back (MaskMapper)
                lut = np.zeros(256, np.uint8)
                lut[1:nl + 1] = ids
                dense = np.stack([_random_labels(rng, shape, np.arange(1, nl + 1), kind) for _ in range(B)])
                pred_dev, lut_dev = torch.from_numpy(dense).cuda(), torch.from_numpy(lut).cuda()
                want = jf_counts_reference(gt, dense, r, lut=lut)
            else:
                pred = np.stack([_random_labels(rng, shape, ids, kind) for _ in range(B)])
                pred_dev, lut_dev = torch.from_numpy(pred).cuda(), None
                want = jf_counts_reference(gt, pred, r)
            got = ops.jf_counts(torch.from_numpy(gt).cuda(), pred_dev, r, lut=lut_dev)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            assert got.shape == (B, 256, 7)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f'shape {shape} r {r} B {B} {kind} lut {use_lut}: first mismatches {bad[:5].tolist()} ' \
                                  f'got {got[tuple(bad[0][:2])].tolist()} want {want[tuple(bad[0][:2])].tolist()}'
            n += 1
    assert n >= 50


def test_kernel_counts_of_a_2d_pair_and_reuse_of_out():
    from xmem2_amd import ops
    rng = np.random.default_rng(3)
    gt = _random_labels(rng, (90, 150), [1, 2], 'blobs')
    pred = _random_labels(rng, (90, 150), [2, 9], 'blobs')
    out = torch.full((1, 256, 7), 12345, dtype=torch.int32, device='cuda')     # zeroed by the entry point before the counts
    ops.jf_counts(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), 5, out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), jf_counts_reference(gt, pred, 5))


def test_reference_values_bit_for_bit():
    from xmem2_amd import ops
    from xmem2_amd.metrics import batched_f_measure, batched_jaccard, bound_pix, jf
    for name, c in golden_cases().items():
        gt, pred, nb, bt = c['gt'], c['pred'], c['nb_objects'], c['bound_th']
        for avg, tag in ((False, 'obj'), (True, 'avg')):
            J = batched_jaccard(gt, pred, average_over_objects=avg, nb_objects=nb)
            F = batched_f_measure(gt, pred, average_over_objects=avg, nb_objects=nb, bound_th=bt)
            assert J.dtype == F.dtype == np.float64
            np.testing.assert_array_equal(J, c[f'J_{tag}'], err_msg=f'{name} J {tag}')
            np.testing.assert_array_equal(F, c[f'F_{tag}'], err_msg=f'{name} F {tag}')
        Jd, Fd = jf(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), nb_objects=nb, bound_th=bt)   # device inputs
        np.testing.assert_array_equal(Jd, c['J_avg'], err_msg=name)
        np.testing.assert_array_equal(Fd, c['F_avg'], err_msg=name)
        counts = ops.jf_counts(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), bound_pix(bt, gt.shape[1:]))
        np.testing.assert_array_equal(counts.cpu().numpy(), c['counts'], err_msg=name)


def _palette():
    """256 distinct colours (the DAVIS bit-interleaved palette): a P-mode PNG round-trips through RGB + quantize exactly."""
    pal = []
    for i in range(256):
        r = g = b = 0
        c = i
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        pal += [r, g, b]
    assert len({tuple(pal[3 * i:3 * i + 3]) for i in range(256)}) == 256
    return pal


def _write_pngs(d, frames, pal):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    for t, a in enumerate(frames):
        im = Image.fromarray(a, mode='P')
        im.putpalette(pal)
        im.save(os.path.join(d, f'{t:05d}.png'))


def test_compute_metrics_on_files(tmp_path):
    from xmem2_amd.metrics import compute_metrics
    cases, pal = golden_cases(), _palette()
    for name in DEFAULT_CASES:
        _write_pngs(tmp_path / 'gt' / name, cases[name]['gt'], pal)
        _write_pngs(tmp_path / 'pred' / name / 'masks', cases[name]['pred'], pal)
    (tmp_path / 'pred' / 'summary.json').write_text('{}')               # the launcher's files next to the videos are skipped
    df = compute_metrics(tmp_path / 'gt', tmp_path / 'pred')
    assert list(df.index) == sorted(DEFAULT_CASES) and list(df.columns) == ['iou', 'f', 'jf']
    for name in DEFAULT_CASES:
        assert df.loc[name, 'iou'] == float(cases[name]['J_avg'].mean(axis=0)), name
        assert df.loc[name, 'f'] == float(cases[name]['F_avg'].mean(axis=0)), name
        assert df.loc[name, 'jf'] == (df.loc[name, 'iou'] + df.loc[name, 'f']) / 2
    # the command line prints the same table
    root = os.path.dirname(os.path.dirname(GOLDEN))
    p = subprocess.run([sys.executable, '-m', 'xmem2_amd.evaluate', '--gt', str(tmp_path / 'gt'), '--pred', str(tmp_path / 'pred'),
                        '--csv', str(tmp_path / 'scores.csv')], cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert 'mean' in p.stdout and all(n in p.stdout for n in DEFAULT_CASES)
    import pandas as pd
    back = pd.read_csv(tmp_path / 'scores.csv', index_col='video_name')
    np.testing.assert_allclose(back['iou'].to_numpy(), df['iou'].to_numpy(), rtol=1e-12)
    # a frame count mismatch is an error
    os.remove(tmp_path / 'pred' / 'multi' / 'masks' / '00000.png')
    with pytest.raises(ValueError):
        compute_metrics(tmp_path / 'gt', tmp_path / 'pred')


def _chair(tmp_path, n=10):
    names = sorted(os.listdir(os.path.join(CHAIR, 'JPEGImages')))[:n]
    imgs, msks = tmp_path / 'JPEGImages' / 'chair', tmp_path / 'Annotations' / 'chair'
    imgs.mkdir(parents=True); msks.mkdir(parents=True)
    for nm in names:
        os.symlink(os.path.join(CHAIR, 'JPEGImages', nm), imgs / nm)
        os.symlink(os.path.join(CHAIR, 'Annotations', nm[:-4] + '.png'), msks / (nm[:-4] + '.png'))
    return str(imgs), str(msks), names


@pytest.mark.parametrize('runner', ['run_on_video', 'run_on_video_ensemble'])
def test_in_loop_jf_equals_scoring_the_written_masks(runner, checkpoint, tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from xmem2_amd import run_on_video as rov
    from xmem2_amd.metrics import batched_f_measure, batched_jaccard, compute_metrics, load_video
    imgs, msks, names = _chair(tmp_path)
    out = tmp_path / 'pred' / 'chair'
    over = {'model': checkpoint, 'mem_every': 2}
    if runner == 'run_on_video_ensemble':
        over['ensemble'] = [[480, False], [480, True]]
    stats = getattr(rov, runner)(imgs, msks, str(out), frames_with_masks=[0], compute_iou=True, compute_jf=True,
                                 print_progress=False, overwrite_config=over)
    assert list(stats.columns) == ['frame', 'mask_provided', 'iou', 'J', 'F']
    assert list(stats['frame']) == names
    with ThreadPoolExecutor(4) as pool:
        gts, preds = load_video(msks, str(out / 'masks'), pool)
    J, F = stats['J'].to_numpy(), stats['F'].to_numpy()
    np.testing.assert_array_equal(J, batched_jaccard(gts, preds))
    np.testing.assert_array_equal(F, batched_f_measure(gts, preds))
    assert 0.0 <= J.min() and J.max() <= 1.0 and 0.0 <= F.min() and F.max() <= 1.0
    df = compute_metrics(str(tmp_path / 'Annotations'), str(tmp_path / 'pred'))
    assert df.loc['chair', 'iou'] == float(np.mean(J)) and df.loc['chair', 'f'] == float(np.mean(F))


def test_in_loop_jf_nan_without_ground_truth(checkpoint, tmp_path):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = _chair(tmp_path, 6)
    for nm in names[3:5]:
        os.remove(os.path.join(msks, nm[:-4] + '.png'))
    stats = run_on_video(imgs, msks, str(tmp_path / 'out'), frames_with_masks=[0], compute_jf=True, print_progress=False,
                         overwrite_config={'model': checkpoint})
    assert list(stats.columns) == ['frame', 'mask_provided', 'J', 'F']
    J, F = stats['J'].to_numpy(), stats['F'].to_numpy()
    assert np.isnan(J[3:5]).all() and np.isnan(F[3:5]).all()
    assert not np.isnan(J[[0, 1, 2, 5]]).any() and not np.isnan(F[[0, 1, 2, 5]]).any()


def test_jf_is_off_by_default(checkpoint, tmp_path):
    from xmem2_amd.run_on_video import run_on_video, run_on_video_ensemble
    imgs, msks, _ = _chair(tmp_path, 3)
    over = {'model': checkpoint}
    assert list(run_on_video(imgs, msks, str(tmp_path / 'a'), print_progress=False, overwrite_config=dict(over)).columns) == \
        ['frame', 'mask_provided']
    assert list(run_on_video(imgs, msks, str(tmp_path / 'b'), compute_iou=True, print_progress=False,
                             overwrite_config=dict(over)).columns) == ['frame', 'mask_provided', 'iou']
    assert list(run_on_video_ensemble(imgs, msks, str(tmp_path / 'c'), compute_iou=True, print_progress=False,
                                      overwrite_config=dict(over)).columns) == ['frame', 'mask_provided', 'iou']


def test_launcher_compute_jf(checkpoint, tmp_path):
    from xmem2_amd.metrics import compute_metrics
    names = sorted(os.listdir(os.path.join(CHAIR, 'JPEGImages')))
    for vid, sel in (('short', names[:4]), ('long', names[:7])):
        for sub, ext in (('JPEGImages', '.jpg'), ('Annotations', '.png')):
            d = tmp_path / sub / vid
            d.mkdir(parents=True)
            for n in sel:
                os.symlink(os.path.join(CHAIR, sub, n[:-4] + ext), d / (n[:-4] + ext))
    out = tmp_path / 'out'
    root = os.path.dirname(os.path.dirname(GOLDEN))
    cmd = [sys.executable, '-m', 'xmem2_amd.launch', '--gpus', '1', '--videos', str(tmp_path / 'JPEGImages'),
           '--masks', str(tmp_path / 'Annotations'), '--out', str(out), '--frames-with-masks', '0', '--compute-jf',
           '--config', json.dumps({'model': checkpoint})]
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    summ = json.load(open(out / 'summary.json'))
    df = compute_metrics(str(tmp_path / 'Annotations'), str(out))
    for v in summ['videos']:
        assert v['mean_J'] == pytest.approx(df.loc[v['name'], 'iou'], abs=1e-12)
        assert v['mean_F'] == pytest.approx(df.loc[v['name'], 'f'], abs=1e-12)
        assert v['mean_JF'] == pytest.approx((v['mean_J'] + v['mean_F']) / 2, abs=1e-15)
    for key in ('mean_J', 'mean_F', 'mean_JF'):
        assert summ[key] == pytest.approx(np.mean([v[key] for v in summ['videos']]), abs=1e-12)
