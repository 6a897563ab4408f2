"""PNG files of uint8 planes, built on the device (config['png_on_device']; csrc/png.hip, include/xmem_hip_png.h).

`encode_host` is the definition: one deterministic function of the plane that the kernels match byte for byte.

    file      signature, IHDR (8 bit, no interlace), PLTE (256 entries; 'palette' only), exactly one IDAT, IEND
    modes     'grey'     colour type 0: the plane's bytes, through a uint8 [256] byte map if `table` is given
              'palette'  colour type 3: the bytes through the byte map `table`, `palette` uint8 [256, 3] as the PLTE chunk
              'rgb'      colour type 2: every byte replaced by its row of `table`, uint8 [256, 3]
    IDAT      a zlib stream: 78 01, ONE deflate block (BFINAL = 1, BTYPE = 01: the fixed Huffman codes of RFC 1951 3.2.6), the
              big-endian Adler-32 of the filtered scanlines
    filter    every scanline is filter type 2 (Up); the row above row 0 is zeros
    tokens    per row, never across rows: the filter byte is a literal; the row's bytes are cut into maximal runs of equal bytes; a
              run of n bytes is its first byte as a literal, then for the other m = n - 1 bytes m // 258 matches of length 258 at
              distance 1 and, for t = m % 258, one match of length t at distance 1 if t >= 3, else t literals

So the deflate size D is a function of the plane, D <= ceil((3 + 9 H (1 + W C) + 7) / 8), and a file is 63 + D bytes, 843 + D with a
PLTE.  The files are 1.2 to 2.3 times the size of Pillow's at compress_level=1 (profiles/r07_png.txt).
"""
import struct
import zlib

import numpy as np

MODES = {'grey': (0, 1), 'rgb': (2, 3), 'palette': (3, 1)}     # mode -> (PNG colour type, bytes per pixel)
SIGNATURE = b'\x89PNG\r\n\x1a\n'
META = 4                                                         # int32 words per frame in a device record: file length, deflate length, 2 spare
MAX_SIDE = 16384
PLTE_BYTES = 12 + 768


def _rev(code, n):
    return int(format(code, f'0{n}b')[::-1], 2)


def _token_tables():
    """(literal bits [256], literal lengths [256], match bits [259], match lengths [259]): a token's bits in the order they enter
    the stream, first bit in bit 0.  A match is its length code, the code's extra bits and the five zero bits of distance code 0."""
    lit_bits, lit_len = np.zeros(256, np.uint32), np.zeros(256, np.uint8)
    for v in range(256):
        lit_bits[v], lit_len[v] = (_rev(0x30 + v, 8), 8) if v < 144 else (_rev(0x190 + v - 144, 9), 9)
    m_bits, m_len = np.zeros(259, np.uint32), np.zeros(259, np.uint8)
    for n in range(3, 259):
        x = n - 3
        extra = 0 if x < 8 or n == 258 else x.bit_length() - 3
        code = 285 if n == 258 else 257 + x if x < 8 else 261 + 4 * extra + ((x >> extra) & 3)
        bits, width = (_rev(code - 256, 7), 7) if code < 280 else (_rev(0xc0 + code - 280, 8), 8)
        m_bits[n], m_len[n] = bits | (x & ((1 << extra) - 1)) << width, width + extra + 5
    return lit_bits, lit_len, m_bits, m_len


_LIT_BITS, _LIT_LEN, _MATCH_BITS, _MATCH_LEN = _token_tables()


def _check_mode(mode):
    if mode not in MODES:
        raise ValueError(f'png: mode = {mode!r}: expected one of {sorted(MODES)}')
    return MODES[mode]


def _tables(mode, table, palette):
    """the byte map / colour table and the palette of a mode as contiguous uint8 arrays (or None), checked"""
    _, C = _check_mode(mode)
    if table is None:
        if mode != 'grey':
            raise ValueError(f"png: mode {mode!r} needs a table")
    else:
        table = np.ascontiguousarray(table)
        if table.dtype != np.uint8 or table.shape != ((256,) if C == 1 else (256, 3)):
            raise ValueError(f'png: the table of mode {mode!r} must be uint8 {[256] if C == 1 else [256, 3]}')
    if (palette is not None) != (mode == 'palette'):
        raise ValueError("png: mode 'palette', and no other, takes a palette")
    if palette is not None:
        palette = np.ascontiguousarray(palette)
        if palette.dtype != np.uint8 or palette.shape != (256, 3):
            raise ValueError('png: the palette must be uint8 [256, 3]')
    return table, palette


def pixel_bytes(plane, mode, table=None):
    """uint8 [H, W C]: the bytes of the image's rows, before the filter"""
    _, C = _check_mode(mode)
    plane = np.asarray(plane)
    if plane.dtype != np.uint8 or plane.ndim != 2 or plane.size == 0:
        raise ValueError('png: a plane must be a uint8 array [H, W] with H, W >= 1')
    if max(plane.shape) > MAX_SIDE:
        raise ValueError(f'png: a plane of {plane.shape}: at most {MAX_SIDE} on a side')
    if table is None:
        return plane
    return np.asarray(table)[plane].reshape(plane.shape[0], plane.shape[1] * C)


def filtered_scanlines(rows):
    """uint8 [H, 1 + L] of uint8 rows [H, L]: the byte 2 and the row minus the row above, mod 256"""
    H, L = rows.shape
    out = np.empty((H, L + 1), np.uint8)
    out[:, 0] = 2
    out[0, 1:] = rows[0]
    out[1:, 1:] = rows[1:] - rows[:-1]
    return out


def _tokens(filtered):
    """(bits uint32, lengths uint8) per byte of the filtered scanlines in stream order; a byte inside a match has length 0"""
    H, L1 = filtered.shape
    flat = filtered.reshape(-1)
    idx = np.arange(flat.size, dtype=np.int64)
    col = idx % L1
    start = np.ones(flat.size, bool)
    start[1:] = flat[1:] != flat[:-1]
    start |= col <= 1                                                    # the filter byte is a token of its own; a run never crosses a row
    s = np.maximum.accumulate(np.where(start, idx, 0))
    nxt = np.where(start, idx, flat.size)
    e = np.empty_like(idx)                                               # the run's end: the first start behind the byte
    e[:-1] = np.minimum.accumulate(nxt[::-1])[::-1][1:]
    e[-1] = flat.size
    o = idx - s
    rem = e - idx                                                        # bytes of the run from this one on
    t = (e - s - 1) % 258
    literal = (o == 0) | ((rem <= t) & (t < 3))
    match = ~literal & ((o - 1) % 258 == 0)
    length = np.where(match, np.minimum(rem, 258), 0)
    bits = np.where(literal, _LIT_BITS[flat], _MATCH_BITS[length])
    nbits = np.where(literal, _LIT_LEN[flat], _MATCH_LEN[length]).astype(np.uint8)
    return bits.astype(np.uint32), nbits


def deflate_fixed(filtered):
    """the deflate block of the filtered scanlines as bytes: header bits 1, 1, 0, the tokens, the 7-bit end-of-block code"""
    bits, nbits = _tokens(filtered)
    keep = nbits > 0
    bits, nbits = bits[keep], nbits[keep].astype(np.int64)
    first = 3 + np.cumsum(nbits) - nbits
    total = 3 + int(nbits.sum()) + 7
    stream = np.zeros(total, np.uint8)
    stream[:2] = 1
    k = np.arange(int(nbits.sum()), dtype=np.int64) - np.repeat(first - 3, nbits)
    stream[3:total - 7] = (np.repeat(bits, nbits) >> k.astype(np.uint32)) & 1
    return np.packbits(stream, bitorder='little').tobytes()


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def encode_host(plane, mode, table=None, palette=None):
    """The PNG file of `plane`, uint8 [H, W], as bytes (the module's docstring has the rules)."""
    colour_type, _ = _check_mode(mode)
    table, palette = _tables(mode, table, palette)
    H, W = np.asarray(plane).shape
    filtered = filtered_scanlines(pixel_bytes(plane, mode, table))
    idat = b'\x78\x01' + deflate_fixed(filtered) + struct.pack('>I', zlib.adler32(filtered.tobytes()))
    return SIGNATURE + _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, colour_type, 0, 0, 0)) \
        + (_chunk(b'PLTE', palette.tobytes()) if palette is not None else b'') + _chunk(b'IDAT', idat) + _chunk(b'IEND', b'')


def file_bytes(deflate_bytes, mode):
    """the length of a file whose deflate block has `deflate_bytes` bytes"""
    return 57 + 6 + deflate_bytes + (PLTE_BYTES if mode == 'palette' else 0)


def worst_case_bytes(H, W, mode):
    """no plane of H x W gives a longer file: every byte a 9-bit literal"""
    _, C = _check_mode(mode)
    return file_bytes((3 + 9 * H * (1 + W * C) + 7 + 7) // 8, mode)


def default_capacity(H, W, mode):
    """bytes per frame a frame loop starts with: a sixteenth of the raw rows (a mask's runs are long: three ragged ellipses at
    480 x 854 need a hundredth), never more than the worst case; a frame that needs more is encoded again at its true length"""
    _, C = _check_mode(mode)
    return min(worst_case_bytes(H, W, mode), file_bytes(4096 + H * (1 + W * C) // 16, mode))


def record_bytes(N, capacity):
    """the length of the uint8 device record of N frames: the meta words, then `capacity` bytes per frame, padded to whole words"""
    return 4 * META * N + -(-N * capacity // 4) * 4


def split_record(buf, N, capacity):
    """(meta int32 [N, META], bytes uint8 [N, capacity]) of a record of `ops.png_encode(..., wait=False)`, as views.
    meta[n, 0] is the true length of frame n's file, also when it exceeds `capacity`; meta[n, 1] that of its deflate block."""
    buf = np.asarray(buf).reshape(-1)
    if buf.dtype != np.uint8 or buf.size != record_bytes(N, capacity):
        raise ValueError(f'png.split_record: expected {record_bytes(N, capacity)} bytes for {N} frames of capacity {capacity}')
    meta = buf[:4 * META * N].view(np.int32).reshape(N, META)
    return meta, buf[4 * META * N:4 * META * N + N * capacity].reshape(N, capacity)


def parse_option(value):
    """config['png_on_device'] -> None or {'mode': 'rgb' | 'palette'}"""
    if value is None or value is False:
        return None
    if value is True:
        return {'mode': 'rgb'}
    if isinstance(value, str):
        value = {'mode': value}
    if not isinstance(value, dict) or set(value) - {'mode'}:
        raise ValueError(f"png_on_device = {value!r}: expected None, True or {{'mode': 'rgb' | 'palette'}}")
    mode = value.get('mode', 'rgb')
    if mode not in ('rgb', 'palette'):
        raise ValueError(f"png_on_device: mode = {mode!r}: expected 'rgb' or 'palette'")
    return {'mode': mode}


def label_map(mapper):
    """uint8 [256]: `MaskMapper.remap_index_mask` as of now as a byte map (dense ids -> the annotation's labels)"""
    return np.asarray(mapper.remap_index_mask(np.arange(256, dtype=np.uint8)), dtype=np.uint8)


def reader_palette(reader):
    """uint8 [256, 3]: the palette of the reader's reference mask, padded with zeros as Pillow pads it"""
    pal = np.zeros(768, np.uint8)
    raw = reader.reference_mask.getpalette() or []
    pal[:min(len(raw), 768)] = raw[:768]
    return pal.reshape(256, 3)


def color_table(reader, mapper_labels):
    """uint8 [256, 3], the table of mode 'rgb': `VideoReader.map_the_colors_back` - a look-up per value - of the values 0..255,
    composed with the label map `mapper_labels`, uint8 [256] (`label_map`): table[v] is the colour the written mask gives a pixel
    whose dense id is v."""
    from PIL import Image
    lut = np.asarray(reader.map_the_colors_back(Image.fromarray(np.arange(256, dtype=np.uint8)[None])), dtype=np.uint8)[0]
    return np.ascontiguousarray(lut[np.asarray(mapper_labels, dtype=np.uint8)])


# ---- what the frame loops, VideoSession.save and the command lines share ---------------------------------------------------------------

def mask_tables(reader, mapper, mode):
    """(table, palette) of a mask PNG as the loops write it, host arrays: 'rgb' gives today's colours, 'palette' the index PNG whose
    pixel values are the annotation's labels under the annotation's palette"""
    labels = label_map(mapper)
    if mode == 'rgb':
        return color_table(reader, labels), None
    return labels, reader_palette(reader)


def bytes_job(files):
    """The `_AsyncSaver` job that writes finished files: `files` is a list of (bytes, sub-directory, file name)."""
    def job():
        return files
    return job


def plane_files(names, labels, files, stem):
    """(bytes, sub-directory, name) of `matte.plane_job`'s files, `files` being the T x K encoded planes in that order"""
    import os
    k = len(labels)
    return [(files[t * k + j], os.path.join(sub, str(lab)), stem + '.png') for t, sub in enumerate(names) for j, lab in enumerate(labels)]


def files_of_record(buf, N, capacity, again, grow=None):
    """The N files of a host record that arrived: `again(n, length) -> bytes` encodes frame n once more at its true length when it
    did not fit, `grow(length)` hears of every such length."""
    meta, data = split_record(buf, N, capacity)
    out = []
    for n in range(N):
        length = int(meta[n, 0])
        if length > capacity:
            if grow is not None:
                grow(length)
            out.append(again(n, length))
        else:
            out.append(data[n, :length].tobytes())
    return out
