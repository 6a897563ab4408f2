"""Host tests of the compressed COCO string form of the track counts (xmem2_amd/rle.py `compress_counts` / `decompress_counts`, the
`xmem_rle_compress` / `xmem_rle_decompress` symbols, config['tracks_counts']):

1. the definition: literal vectors of the public format in both directions, round trips over every length class and both signs, every
   refusal of the reader;
2. every consumer of counts takes a string where it takes a list: `decode`, `events_from_counts`, `TrackWriter(strings=)`, `TrackReader`,
   `read_tracks`, files mixing both forms, `--recode` there and back;
3. the new symbols, the config key, and bad arguments answered without touching the GPU."""
import json

import numpy as np
import pytest


# worked out with a straight port of rleToString / rleFrString of the public COCO mask API
VECTORS = [([5, 3], '53'), ([16], '`0'), ([0, 7, 1], '071'), ([3, 4, 5, 6], '3452'), ([44], '\\1'),
           ([10, 2, 3, 1, 40, 2, 900], ':23OU11lj0'), ([0, 268435456], '0PPPPP8'),
           ([100, 31, 32, 15, 16, 1000, 1, 17], 'T3o0P1@@in0AYQO')]
RUNS = [1, 2, 15, 16, 17, 511, 512, 600, 20000, 1 << 20]


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counts,string', VECTORS)
def test_literal_vectors_in_both_directions(counts, string):
    from xmem2_amd.rle import compress_counts, decompress_counts
    assert compress_counts(counts) == string
    assert decompress_counts(string) == counts
    assert decompress_counts(string.encode('ascii')) == counts
    assert all(48 <= ord(ch) <= 111 for ch in string)


def _value_length(x):
    """characters of a value: the least k with -2^(5k-1) <= x < 2^(5k-1)"""
    return next(k for k in range(1, 8) if -(1 << (5 * k - 1)) <= x < (1 << (5 * k - 1)))


def test_round_trip_over_every_length_class_and_both_signs():
    from xmem2_amd.rle import compress_counts, decompress_counts
    rng = np.random.default_rng(7)
    seen = set()
    for trial in range(200):
        counts = [int(v) for v in rng.choice(RUNS, size=int(rng.integers(1, 40)))]
        if trial % 4 == 0:
            counts.insert(int(rng.integers(0, len(counts) + 1)), 1 << 28)
        if trial % 5 == 0:
            counts[0] = 0
        s = compress_counts(counts)
        assert decompress_counts(s) == counts
        values = [c - counts[i - 2] if i > 2 else c for i, c in enumerate(counts)]
        assert len(s) == sum(_value_length(x) for x in values)
        seen |= {(_value_length(x), x < 0) for x in values}
    assert seen == {(k, neg) for k in range(1, 7) for neg in (False, True)}      # 1..6 characters, differences of both signs


def test_decompress_counts_refuses():
    from xmem2_amd.rle import decompress_counts
    for bad, what in (('5/3', 'outside'), ('5p3', 'outside'), ('5é3', 'outside'), (b'5\xff', 'outside'),
                      ('PPPPPPP0', 'more than 6'), ('5P', 'ends inside'), ('PPPPP', 'ends inside'), ('', 'empty'), (b'', 'empty')):
        with pytest.raises(ValueError, match=what):
            decompress_counts(bad)
    assert decompress_counts('PPPPP0') == [0]                         # six characters are a value; zeros in high groups are legal


# ---- 2. the consumers -----------------------------------------------------------------------------------------------------------
def test_decode_and_events_take_a_string_like_a_list():
    from xmem2_amd import rle
    rng = np.random.default_rng(3)
    for shape in ((1, 1), (5, 3), (17, 33)):
        for _ in range(4):
            plane = rng.random(shape) < 0.4
            counts = rle.encode_host(plane.astype(np.uint8), 1).counts
            s = rle.compress_counts(counts)
            for form in (s, s.encode('ascii')):
                np.testing.assert_array_equal(rle.decode(form, *shape), rle.decode(counts, *shape))
                np.testing.assert_array_equal(rle.decode(form, *shape), plane)
                np.testing.assert_array_equal(rle.events_from_counts(form, *shape), rle.events_from_counts(counts, *shape))
    for bad in (rle.compress_counts([5]), rle.compress_counts([2, 0, 4]), rle.compress_counts([3, -1, 4]), '5P', ''):
        with pytest.raises(ValueError):
            rle.decode(bad, 2, 3)
        with pytest.raises(ValueError):
            rle.events_from_counts(bad, 2, 3)


def test_a_single_count_is_an_empty_plane():
    from xmem2_amd import rle
    s = rle.compress_counts([6 * 7])
    assert not rle.decode(s, 6, 7).any() and rle.decode(s, 6, 7).shape == (6, 7)
    assert len(rle.events_from_counts(s, 6, 7)) == 0


def _masks():
    """Three 4 x 15 frames of labels 5 and 9; frame 0 holds a first run of 44 zeros for label 5: its string starts with a backslash."""
    a = np.zeros((4, 15), np.uint8)
    a[0, 11] = 1                                                     # j = 11 * 4 + 0 = 44
    a[2:4, 13] = 1
    a[1:3, 2:5] = 2
    b = np.zeros((4, 15), np.uint8)
    b[:, :3] = 2
    b[3, 14] = 1
    return [a, None, b]


def test_writer_with_strings_through_json_through_the_reader(tmp_path):
    from xmem2_amd import rle
    masks = _masks()
    writer, plain = rle.TrackWriter(4, 15), rle.TrackWriter(4, 15)
    for t, m in enumerate(masks):
        name = f'{t:05d}.jpg'
        if m is None:
            writer.add_frame(name)
            plain.add_frame(name)
            continue
        meta, events = rle.record_host(m, 2)
        strings = [rle.compress_counts(rle.counts_from_events(ev, 4, 15)) for ev in rle.label_events(meta, events)]
        writer.add_frame(name, meta, None, labels=[5, 9], strings=strings)          # the events are not needed
        plain.add_frame(name, meta, events, labels=[5, 9])
    doc = writer.to_dict()
    seg = doc['annotations'][0]['segmentations'][0]
    assert seg == {'size': [4, 15], 'counts': rle.compress_counts(rle.encode_host(masks[0], 1).counts)} and seg['counts'][0] == '\\'
    assert doc['annotations'][0]['bboxes'] == plain.to_dict()['annotations'][0]['bboxes']
    assert doc['annotations'][1]['areas'] == plain.to_dict()['annotations'][1]['areas'] == [6, None, 12]
    path = writer.write(str(tmp_path / 'c'))
    text = open(path).read()
    assert '\\\\' in text                                             # json.dumps escaped the backslash
    back = json.loads(text)
    assert back == doc
    lut = np.zeros(3, np.uint8)
    lut[1], lut[2] = 5, 9
    reader = rle.TrackReader(path)
    video, decoded = rle.read_tracks(path)
    for t, m in enumerate(masks):
        if m is None:
            assert reader.mask_host(t) is None and decoded[t] is None and not reader.has_mask(t)
            continue
        np.testing.assert_array_equal(reader.mask_host(t), lut[m])
        np.testing.assert_array_equal(decoded[t], lut[m])
        meta, events = reader.record(t)                               # the record of a string frame equals that of a list frame
        want_meta, want_events = rle.TrackReader(plain.to_dict()).record(t)
        np.testing.assert_array_equal(meta, want_meta)
        np.testing.assert_array_equal(events, want_events)
    # add_mask builds the same file on the host
    host = rle.TrackWriter(4, 15)
    for t, m in enumerate(masks):
        host.add_mask(f'{t:05d}.jpg', m, k=2, labels=[5, 9], counts='compressed')
    assert host.to_dict() == doc
    with pytest.raises(ValueError):
        host.add_mask('x.jpg', masks[0], counts='zip')
    with pytest.raises(ValueError):
        writer.add_frame('x.jpg', *rle.record_host(masks[0], 2), strings=['0'])


def test_recode_there_and_back_gives_the_identical_file(tmp_path, capsys):
    from xmem2_amd import rle
    plain = rle.TrackWriter(4, 15)
    for t, m in enumerate(_masks()):
        plain.add_mask(f'{t:05d}.jpg', m, k=2, labels=[5, 9])
    src = plain.write(str(tmp_path / 'list'))
    comp, back = str(tmp_path / 'out' / 'c.json'), str(tmp_path / 'out' / 'l.json')
    assert rle.main(['--tracks', src, '--recode', 'compressed', '--out', comp]) == 0
    assert rle.main(['--tracks', comp, '--recode', 'list', '--out', back]) == 0
    assert open(back, 'rb').read() == open(src, 'rb').read()
    assert len(open(comp, 'rb').read()) < len(open(src, 'rb').read())
    doc = json.load(open(comp))
    assert all(isinstance(s['counts'], str) for a in doc['annotations'] for s in a['segmentations'] if s is not None)
    host = rle.TrackWriter(4, 15)
    for t, m in enumerate(_masks()):
        host.add_mask(f'{t:05d}.jpg', m, k=2, labels=[5, 9], counts='compressed')
    assert doc == host.to_dict()                                      # the file the 'compressed' option writes
    assert rle.main(['--tracks', comp, '--recode', 'compressed', '--out', back]) == 0     # already in that form: kept
    assert open(back, 'rb').read() == open(comp, 'rb').read()
    assert rle.main(['--tracks', comp, '--out', str(tmp_path / 'png')]) == 0              # to PNGs from the string form
    from PIL import Image
    np.testing.assert_array_equal(np.array(Image.open(tmp_path / 'png' / '00000.png')), rle.read_tracks(src)[1][0])
    capsys.readouterr()


def test_a_file_mixing_both_forms_reads():
    from xmem2_amd import rle
    plain = rle.TrackWriter(4, 15)
    masks = _masks()
    for t, m in enumerate(masks):
        plain.add_mask(f'{t:05d}.jpg', m, k=2, labels=[5, 9])
    doc = plain.to_dict()
    mixed = json.loads(json.dumps(doc))
    mixed['annotations'][0]['segmentations'][0]['counts'] = rle.compress_counts(doc['annotations'][0]['segmentations'][0]['counts'])
    mixed['annotations'][1]['segmentations'][2]['counts'] = rle.compress_counts(doc['annotations'][1]['segmentations'][2]['counts'])
    a, b = rle.TrackReader(mixed), rle.TrackReader(doc)
    for t in range(3):
        if masks[t] is None:
            assert a.mask_host(t) is None
            continue
        np.testing.assert_array_equal(a.mask_host(t), b.mask_host(t))
        for x, y in zip(a.record(t), b.record(t)):
            np.testing.assert_array_equal(x, y)
    assert a._all_compressed(0) is False and a._all_compressed(1) is False          # frame 0 mixes the forms, frame 1 has no entry
    assert rle.recode_tracks(mixed, 'list') == doc
    mixed['annotations'][0]['segmentations'][0]['counts'] = '5P'
    with pytest.raises(ValueError):
        rle.TrackReader(mixed).mask_host(0)


def test_split_string_record_and_label_strings():
    from xmem2_amd import rle
    lens = np.array([[2, 0, 3], [0, 0, 1]], np.int32)
    chars = np.zeros((2, 8), np.uint8)
    chars[0, :5] = list(b'53071')
    chars[1, :1] = list(b'7')
    buf = np.concatenate((lens.view(np.uint8).reshape(-1), chars.reshape(-1)))
    got_len, got_chars = rle.split_string_record(buf, 2, 3, 8)
    np.testing.assert_array_equal(got_len, lens)
    np.testing.assert_array_equal(got_chars, chars)
    assert rle.label_strings(got_len[0], got_chars[0]) == ['53', '', '071'] and rle.label_strings(got_len[1], got_chars[1]) == ['', '', '7']
    with pytest.raises(ValueError):
        rle.label_strings(np.array([5, 5, 5]), chars[0])              # more characters than were kept
    with pytest.raises(ValueError):
        rle.label_strings(np.array([-1, -1, -1]), chars[0])           # a frame whose events did not fit


# ---- 3. symbols, config, bad arguments ------------------------------------------------------------------------------------------
def test_string_symbols_are_declared_listed_and_exported_and_the_abi_version_stays_5():
    from xmem2_amd import _lib
    for name in ('xmem_rle_compress', 'xmem_rle_compress_workspace_bytes', 'xmem_rle_decompress', 'xmem_rle_decompress_workspace_bytes'):
        assert hasattr(_lib.load(), name)
    assert _lib.load().xmem_version() == 5 == _lib.ABI_VERSION


def test_tracks_counts_defaults_to_the_list_form():
    from xmem2_amd import rle
    from xmem2_amd.configuration import VIDEO_INFERENCE_CONFIG
    from xmem2_amd.run_on_video import _TrackLoop
    assert VIDEO_INFERENCE_CONFIG['tracks_counts'] == 'list' and rle.COUNT_FORMS == ('list', 'compressed')
    assert _TrackLoop().counts == 'list' and _TrackLoop('compressed').counts == 'compressed'
    with pytest.raises(ValueError):
        _TrackLoop('zip')


def test_string_abi_rejects_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib
    lib = _lib.load()
    one = 16                                                          # stands for a non-null pointer: every call returns before using it

    def compress(meta=one, events=one, N=1, H=8, W=8, K=1, cap=64, ccap=64, lens=one, chars=one, ws=one, nbytes=1 << 20):
        return lib.xmem_rle_compress(meta, events, N, H, W, K, cap, ccap, lens, chars, ws, nbytes, None)

    def decompress(chars=one, n=4, ofs=one, N=1, H=8, W=8, K=1, cap=64, meta=one, events=one, status=one, ws=one, nbytes=1 << 20):
        return lib.xmem_rle_decompress(chars, n, ofs, N, H, W, K, cap, meta, events, status, ws, nbytes, None)
    for null in ('meta', 'events', 'lens', 'chars', 'ws'):
        assert compress(**{null: None}) == -1
    for null in ('chars', 'ofs', 'meta', 'events', 'status', 'ws'):
        assert decompress(**{null: None}) == -1
    for fn in (compress, decompress):
        for bad in (dict(K=0), dict(K=255), dict(N=0), dict(H=0), dict(W=0), dict(cap=0)):
            assert fn(**bad) == -1
        assert fn(H=16385) == _lib.UNSUPPORTED and fn(W=16385) == _lib.UNSUPPORTED and fn(N=65536) == _lib.UNSUPPORTED
        assert fn(nbytes=4) == -3                                     # workspace too small
    assert compress(ccap=0) == -1 and decompress(n=-1) == -1
    assert compress(cap=(1 << 28) + 1, nbytes=1 << 40) == _lib.UNSUPPORTED
    assert lib.xmem_rle_compress_workspace_bytes(3, 5, 1000) == 3 * 1005 * 4
    assert lib.xmem_rle_decompress_workspace_bytes(3, 5) == 3 * 5 * 2 * 4
    for k in (0, 255):
        assert lib.xmem_rle_compress_workspace_bytes(1, k, 64) == 0 and lib.xmem_rle_decompress_workspace_bytes(1, k) == 0
    assert lib.xmem_rle_compress_workspace_bytes(1, 1, 0) == 0 and lib.xmem_rle_compress_workspace_bytes(65536, 1, 64) == 0


def test_string_ops_have_no_cpu_path_and_validate():
    import torch
    from xmem2_amd import ops
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.rle_compress(torch.zeros(70, dtype=torch.int32), 8, 8, 1, 64)
    for bad in (dict(H=0), dict(W=16385), dict(K=255), dict(K=True)):
        args = dict(H=8, W=8, K=1)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.rle_compress(torch.zeros(70, dtype=torch.int32), args['H'], args['W'], args['K'], 64)
        with pytest.raises(ValueError):
            ops.rle_decompress([['0']], args['H'], args['W'], args['K'])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            ops.rle_decompress([['`0P1']], 8, 8, 1)
