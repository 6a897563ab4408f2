"""Shared helpers of the PNG tests: a file taken apart chunk by chunk without the module under test, planes that reach the token
rules' boundaries, and what an opened file must show."""
import io
import struct
import zlib

import numpy as np
from PIL import Image

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def chunks(data):
    """[(type, payload)] of a PNG file; asserts the signature, every CRC and that nothing follows IEND"""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        n, kind = struct.unpack('>I4s', data[at:at + 8])
        payload = data[at + 8:at + 8 + n]
        assert len(payload) == n and struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + payload), kind
        out.append((kind, payload))
        at += 12 + n
    assert at == len(data) and out[-1] == (b'IEND', b'')
    return out


def filtered_up(rows):
    """the Up-filtered scanlines of uint8 rows [H, L] as bytes, the row above row 0 being zeros (int16 arithmetic, not the module's)"""
    rows = rows.astype(np.int16)
    above = np.concatenate([np.zeros_like(rows[:1]), rows[:-1]])
    body = ((rows - above) & 255).astype(np.uint8)
    return np.concatenate([np.full((rows.shape[0], 1), 2, np.uint8), body], axis=1).tobytes()


def expected_pixels(plane, mode, table=None):
    """what the opened file must hold: [H, W] or, for 'rgb', [H, W, 3]"""
    if table is None:
        return plane
    return np.asarray(table)[plane]


def check_file(data, plane, mode, table=None, palette=None):
    """everything the issue asks of one file; -> the deflate block's length"""
    Image.open(io.BytesIO(data)).verify()
    im = Image.open(io.BytesIO(data))
    want = expected_pixels(plane, mode, table)
    assert im.mode == {'grey': 'L', 'rgb': 'RGB', 'palette': 'P'}[mode] and im.size == (plane.shape[1], plane.shape[0])
    np.testing.assert_array_equal(np.array(im), want)
    parts = chunks(data)
    kinds = [k for k, _ in parts]
    assert kinds == ([b'IHDR', b'PLTE', b'IDAT', b'IEND'] if mode == 'palette' else [b'IHDR', b'IDAT', b'IEND'])
    assert parts[0][1] == struct.pack('>IIBBBBB', plane.shape[1], plane.shape[0], 8, {'grey': 0, 'rgb': 2, 'palette': 3}[mode], 0, 0, 0)
    if mode == 'palette':
        assert parts[1][1] == np.asarray(palette, np.uint8).tobytes()
        np.testing.assert_array_equal(np.array(im.getpalette(), np.uint8).reshape(-1, 3), np.asarray(palette, np.uint8))
    idat = dict(parts)[b'IDAT']
    assert idat[:2] == b'\x78\x01' and idat[2] & 7 == 3                   # one final block of fixed Huffman codes
    rows = want.reshape(plane.shape[0], -1)
    assert zlib.decompress(idat) == filtered_up(rows)                     # checks the Adler-32 too
    return len(idat) - 6


def boundary_rows():
    """grey rows (name, uint8 [1, L]) whose data length sits at every run and match boundary: constant, and with one odd byte at
    either end"""
    out = []
    for L in (2, 3, 4, 258, 259, 260, 261, 262, 517, 518, 519, 520):
        const = np.full((1, L), 9, np.uint8)
        head, tail = const.copy(), const.copy()
        head[0, 0], tail[0, -1] = 200, 201
        out += [(f'const{L}', const), (f'head{L}', head), (f'tail{L}', tail)]
    return out


def every_run_length():
    """uint8 [4, W]: rows built from runs of every length 1..300, values changing from run to run (above and below 144), the
    lengths spread over the rows so that a row stays short"""
    runs = [[], [], [], []]
    for n in range(1, 301):
        runs[n % 4].append(np.full(n, (n * 37) % 256, np.uint8))
    rows = [np.concatenate(r) for r in runs]
    W = max(len(r) for r in rows)
    return np.stack([np.concatenate([r, np.arange(W - len(r), dtype=np.uint8) * 3 + 1]) for r in rows])


def noise(shape, seed, low=0):
    return np.random.default_rng(seed).integers(low, 256, shape, dtype=np.uint8)


def tables(seed=5):
    """(byte map [256], colour table [256, 3], palette [256, 3]), none of them trivial"""
    rng = np.random.default_rng(seed)
    return rng.permutation(256).astype(np.uint8), rng.integers(0, 256, (256, 3), dtype=np.uint8), rng.integers(0, 256, (256, 3), dtype=np.uint8)
