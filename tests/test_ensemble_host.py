"""Test-time ensemble (`run_on_video_ensemble`, `ops.ensemble_accumulate`) without a GPU: the pass list, the C ABI's argument checks,
and a numpy restatement of the per-pass post-processing + merge of eval.py:208-225 and merge_multi_scale.py:44-57 that the GPU tests
(tests/test_gpu_ensemble.py) compare the kernel against."""
import numpy as np
import pytest
import torch


def interp_reference(prob, shape):
    """eval.py:208-210 on the host: F.interpolate(prob.unsqueeze(1), shape, mode='bilinear', align_corners=False), only when the
    working size differs from the original."""
    prob = torch.as_tensor(np.asarray(prob, np.float32))
    if tuple(prob.shape[-2:]) == tuple(shape):
        return prob.numpy()
    return torch.nn.functional.interpolate(prob.unsqueeze(1), tuple(shape), mode='bilinear', align_corners=False)[:, 0].numpy()


def quantise_reference(score, mirror):
    """eval.py:217-225: torch.flip(prob, dims=[-1]) of a flipped pass, then (prob * 255).astype(np.uint8) - an fp32 multiply and a
    truncation (probabilities lie in [0, 1]; the clip only pins what an out-of-range float would do)."""
    s = np.asarray(score, np.float32)
    if mirror:
        s = s[:, :, ::-1]
    return np.clip(s * np.float32(255), 0, 255).astype(np.uint8)


def ensemble_merge_reference(scores, mirrors):
    """merge_multi_scale.py:44-57 over passes whose scores are already at the original resolution: exact integer sum of the uint8
    scores (the reference sums in float32, exact below 2^24), then np.argmax (first maximal index wins).
    Returns (sum as uint16 [C,H,W], merged index mask uint8 [H,W])."""
    acc = None
    for s, m in zip(scores, mirrors):
        q = quantise_reference(s, m).astype(np.uint16)
        acc = q if acc is None else acc + q
    return acc, np.argmax(acc, axis=0).astype(np.uint8)


def test_merge_restatement_on_a_hand_built_case():
    f = np.float32
    below = np.nextafter(f(3 / 255), f(0))
    # pass A (not flipped), 2 classes x 1 x 4
    a = np.array([[[1.0, f(3 / 255), below, 0.5]],
                  [[0.0, f(252 / 255), f(100 / 255), 0.5]]], np.float32)
    # pass B (flipped): given in its mirrored working frame; after the flip class 0 is [1, 25/255, 0, 0], class 1 is [0, 0, .5, 0]
    b = np.array([[[0.0, 0.0, f(25 / 255), 1.0]],
                  [[0.0, 0.5, 0.0, 0.0]]], np.float32)
    qa = quantise_reference(a, False)
    assert qa[0, 0].tolist() == [255, 3, 2, 127]          # p = 1.0 -> 255; exactly k/255 -> k; one ulp below -> k - 1; .5 -> 127
    assert qa[1, 0].tolist() == [0, 252, 100, 127]
    assert quantise_reference(b, True)[:, 0].tolist() == [[255, 25, 0, 0], [0, 0, 127, 0]]
    acc, mask = ensemble_merge_reference([a, b], [False, True])
    assert acc.dtype == np.uint16 and acc[:, 0].tolist() == [[510, 28, 2, 127], [0, 252, 227, 127]]
    assert mask[0].tolist() == [0, 1, 1, 0]               # the last pixel is an exact tie: the first class wins
    # the bilinear step is F.interpolate itself, and only when the size differs
    assert np.array_equal(interp_reference(a, (1, 4)), a)
    up = interp_reference(a, (2, 8))
    assert up.shape == (2, 2, 8) and np.allclose(up[:, 0], up[:, 1], atol=1e-7)  # one source row: both output rows read it
    assert np.allclose(up[:, 0, 0], a[:, 0, 0], atol=1e-7)                       # src x = -0.25 clamps to the first sample


def test_ensemble_pass_list_parsing():
    from xmem2_amd.run_on_video import MAX_ENSEMBLE_PASSES, parse_ensemble
    assert parse_ensemble(None, 480) == ((480, False), (480, True))
    assert parse_ensemble(None, -1) == ((-1, False), (-1, True))
    assert parse_ensemble([[480, False], [480, True], [600, False], [600, True]], 480) == \
        ((480, False), (480, True), (600, False), (600, True))
    assert parse_ensemble([[480, False], [480, False]], 240) == ((480, False), (480, False))     # duplicates are passes too
    assert parse_ensemble(([-1, 1], [240, 0]), 480) == ((-1, True), (240, False))
    assert len(parse_ensemble([[480, False]] * MAX_ENSEMBLE_PASSES, 480)) == MAX_ENSEMBLE_PASSES == 16
    for bad in ([], [[480, False]] * 17, [[0, False]], [[-2, True]], [[480.0, False]], [['480', False]], [[True, False]],
                [[480]], [480, False], [[480, 'yes']], [[480, 2]], 'flip'):
        with pytest.raises(ValueError):
            parse_ensemble(bad, 480)


def test_ensemble_rejects_bad_config_before_touching_the_gpu(tmp_path):
    from xmem2_amd.run_on_video import run_on_video_ensemble
    with pytest.raises(ValueError):
        run_on_video_ensemble(str(tmp_path), str(tmp_path), str(tmp_path / 'out'), overwrite_config={'ensemble': []})
    with pytest.raises(NotImplementedError):
        run_on_video_ensemble(str(tmp_path), str(tmp_path), str(tmp_path / 'out'), augment_images_with_masks=True)


def test_ensemble_accumulate_abi_rejects_bad_arguments_without_touching_the_gpu():
    import ctypes
    from xmem2_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)                         # never dereferenced: every call below fails its argument check first
    f = lib.xmem_ensemble_accumulate
    assert f(None, 2, 8, 8, 0, p, 8, 8, 1, None, None) == -1            # prob NULL
    assert f(p, 2, 8, 8, 0, None, 8, 8, 1, p, None) == -1               # acc NULL
    assert f(p, 0, 8, 8, 0, p, 8, 8, 1, None, None) == -1               # C <= 0
    assert f(p, 256, 8, 8, 0, p, 8, 8, 1, None, None) == -1             # C > 255
    for hi, wi, h, w in ((0, 8, 8, 8), (8, -1, 8, 8), (8, 8, 0, 8), (8, 8, 8, -3)):
        assert f(p, 2, hi, wi, 1, p, h, w, 0, p, None) == -1


def test_ensemble_accumulate_binding_rejects_cpu_tensors():
    from xmem2_amd import ops
    prob = torch.zeros(2, 4, 4)
    with pytest.raises(RuntimeError):
        ops.ensemble_accumulate(prob, (4, 4), False, torch.zeros(2, 4, 4, dtype=torch.uint16), True)
