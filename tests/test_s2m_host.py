"""CPU: scribble-to-mask (S2M) surface - state-dict spec, synthetic weights, the input pack restated in numpy, argument checks,
CLI parsing and file pairing, exported symbols."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

_spec = importlib.util.spec_from_file_location('make_s2m_goldens', os.path.join(GOLDEN, 'make_s2m_goldens.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def test_state_dict_spec_matches_reference():
    from xmem2_amd.s2m import state_dict_spec
    gd = load_golden('s2m')
    spec = state_dict_spec()
    assert len(spec) == 368
    assert list(spec) == gd['spec_names'].tolist()
    assert [str(tuple(v)) for v in spec.values()] == gd['spec_shapes'].tolist()


def test_synthetic_weights_deterministic():
    from xmem2_amd.s2m import state_dict_spec
    from xmem2_amd.synth import synthetic_s2m_state_dict
    a, b = synthetic_s2m_state_dict(0, as_torch=False), synthetic_s2m_state_dict(0, as_torch=False)
    c = synthetic_s2m_state_dict(1, as_torch=False)
    spec = state_dict_spec()
    assert list(a) == list(spec) and all(a[k].shape == tuple(spec[k]) for k in a)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a['backbone.conv1.weight'], c['backbone.conv1.weight'])
    assert all(np.isfinite(v).all() for v in a.values())


@pytest.mark.parametrize('case', [0, 1, 2])
def test_pack_restatement_matches_recorded_inputs(case):
    """the reference's per-object binary channels, restated in numpy, equal the recorded ones (padding / ignore / label > K)"""
    name, H, W, K, seed = G.CASES[case]
    gd = load_golden('s2m')
    image, prev, scr = G.case_inputs(H, W, K, seed)
    got = G.pack_channels(prev, scr, K)
    assert np.array_equal(got, gd[f'{name}_channels'])
    if K >= 3:
        assert not got[2, 1].any(), 'object 3 must have no positive stroke'
        assert (scr == K + 1).any() and (scr == 255).any() and (scr == 0).any()
        assert got[:, 2][:, scr == K + 1].all(), 'a label > K is a negative stroke for every object'


def test_padding_geometry():
    from xmem2_amd.s2m import pad_divide_by_16
    assert pad_divide_by_16(480, 854) == (480, 864, 0, 5)
    assert pad_divide_by_16(200, 300) == (208, 304, 4, 2)
    assert pad_divide_by_16(64, 96) == (64, 96, 0, 0)


def test_argument_checks(tmp_path):
    from xmem2_amd.s2m import S2M, S2MController
    with pytest.raises(ValueError):
        S2MController(object(), 0)
    with pytest.raises(ValueError):
        S2MController(object(), 255)
    ctl = S2MController(object(), 2, device='cpu')
    with pytest.raises(ValueError):
        ctl._inputs(torch.zeros(1, 3, 8, 8), torch.zeros(8, 9), np.zeros((8, 8), np.uint8))
    with pytest.raises(ValueError):
        ctl._inputs(torch.zeros(1, 3, 8, 8), torch.zeros(8, 8), np.zeros((7, 8), np.uint8))
    with pytest.raises(ValueError):
        ctl._inputs(torch.zeros(2, 3, 8, 8), torch.zeros(8, 8), np.zeros((8, 8), np.uint8))
    with pytest.raises(FileNotFoundError):
        S2M(model_path=str(tmp_path / 'missing.pth'), device='cpu')
    net = S2M(device='cpu')
    with pytest.raises(RuntimeError, match='missing'):
        net.load_state_dict({'backbone.conv1.weight': torch.zeros(64, 6, 7, 7)})
    with pytest.raises(RuntimeError, match='no weights'):
        net.features(None)


def test_cli_parsing(tmp_path):
    from xmem2_amd.scribble import parse_args
    a = parse_args(['--images', 'i', '--scribbles', 's', '--out', 'o', '--synthetic-seed', '3'])
    assert a.synthetic_seed == 3 and a.model is None and a.ignore_class == 255 and a.num_objects is None and a.prev_masks is None
    with pytest.raises(SystemExit):
        parse_args(['--images', 'i', '--scribbles', 's', '--out', 'o'])                          # no weights
    with pytest.raises(SystemExit):
        parse_args(['--images', 'i', '--scribbles', 's', '--out', 'o', '--model', str(tmp_path / 'none.pth')])
    with pytest.raises(SystemExit):
        parse_args(['--images', 'i', '--scribbles', 's', '--out', 'o', '--synthetic-seed', '0', '--num-objects', '0'])
    with pytest.raises(SystemExit):
        parse_args(['--images', 'i', '--scribbles', 's', '--out', 'o', '--synthetic-seed', '0', '--model', 'x'])


def test_file_pairing(tmp_path):
    from xmem2_amd.scribble import frame_number, pair_files
    assert frame_number('frame_000123.jpg') == 123 and frame_number('a7b9.png') == 7 and frame_number('none.png') is None
    (tmp_path / 'img').mkdir(); (tmp_path / 'scr').mkdir(); (tmp_path / 'prev').mkdir()
    for n in (0, 5, 10):
        (tmp_path / 'img' / f'frame_{n:06d}.jpg').write_bytes(b'')
    (tmp_path / 'img' / 'notes.txt').write_bytes(b'')
    (tmp_path / 'scr' / 'scribble_10.png').write_bytes(b'')
    (tmp_path / 'scr' / 'scribble_0.png').write_bytes(b'')
    (tmp_path / 'prev' / '10.png').write_bytes(b'')
    pairs = pair_files(str(tmp_path / 'img'), str(tmp_path / 'scr'), str(tmp_path / 'prev'))
    assert pairs == [(0, 'frame_000000.jpg', 'scribble_0.png', None), (10, 'frame_000010.jpg', 'scribble_10.png', '10.png')]
    (tmp_path / 'scr' / 'scribble_3.png').write_bytes(b'')
    with pytest.raises(FileNotFoundError):
        pair_files(str(tmp_path / 'img'), str(tmp_path / 'scr'))
    (tmp_path / 'scr' / 'scribble_3.png').unlink()
    (tmp_path / 'scr' / 'x_010.png').write_bytes(b'')
    with pytest.raises(ValueError):
        pair_files(str(tmp_path / 'img'), str(tmp_path / 'scr'))


def test_new_symbols_exported():
    from xmem2_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in ('xmem_conv2d_nhwc_dilated', 'xmem_conv2d_dilated_workspace_bytes', 'xmem_s2m_pack', 'xmem_channel_mean',
                     'xmem_broadcast_channels', 'xmem_resize_bilinear_nhwc', 'xmem_s2m_output', 'xmem_aggregate_wbg'):
            assert hasattr(lib, name)
