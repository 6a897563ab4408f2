"""Block motion between two frames: an exhaustive integer block-matching search on 8-bit luma.  This module is the definition, in
numpy; csrc/motion.hip (include/xmem_hip_motion.h, `ops.block_motion`) gives the same bytes on the device.  Its one user is the
motion-compensated temporal vote, `temporal.mode_mc_host`.

  luma     (77 R + 150 G + 29 B + 128) >> 8 of an 8-bit RGB frame.
  blocks   BLOCK x BLOCK pixels; the blocks of the last row and column are cropped to the image.
  search   the candidates of a block are the integer (dy, dx) in [-search, search]^2 for which the displaced (cropped) block lies
           wholly inside `ref`: nothing exists outside the image, there is no padding and no clamping.  (0, 0) always is one.  The
           cost is the sum of absolute differences (SAD) over the block; the winner minimises (SAD, dy^2 + dx^2, dy, dx) in that order.
  bias     if SAD(0, 0) - SAD(winner) <= bias * pixels of the block, the block takes (0, 0) and its SAD: flat and noisy areas stay
           still.

The defaults SEARCH, BIAS and MAX_SAD are choices, not measurements on real footage.
"""
import numpy as np

BLOCK = 16           # a constant of the kernels, not an option
MAX_SEARCH = 32
SEARCH = 16          # default search range, in pixels either way
BIAS = 1             # default zero bias, in grey levels per pixel
MAX_SAD = 24         # default abstention threshold of the compensated vote, in grey levels per pixel


def _int_in(where, name, v, low, top):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not low <= v <= top:
        raise ValueError(f'{where}: {name} = {v!r} must be an integer in {low}..{top}')
    return int(v)


def parse_motion(value, where):
    """True or {'search', 'bias', 'max_sad'} (any subset) -> the full dict; ValueError, naming `where`, for anything else"""
    if value is True:
        value = {}
    if not isinstance(value, dict) or not set(value) <= {'search', 'bias', 'max_sad'}:
        raise ValueError(f"{where} = {value!r}: expected True or a dict with keys out of 'search', 'bias', 'max_sad'")
    return {'search': _int_in(where, 'search', value.get('search', SEARCH), 1, MAX_SEARCH),
            'bias': _int_in(where, 'bias', value.get('bias', BIAS), 0, 255),
            'max_sad': _int_in(where, 'max_sad', value.get('max_sad', MAX_SAD), 0, 255)}


def blocks_of(H, W):
    """(By, Bx) of an H x W image"""
    return (H + BLOCK - 1) // BLOCK, (W + BLOCK - 1) // BLOCK


def block_pixels(H, W):
    """int32 [By,Bx]: the pixels of every (cropped) block"""
    By, Bx = blocks_of(H, W)
    hs = np.minimum(BLOCK, H - BLOCK * np.arange(By))
    ws = np.minimum(BLOCK, W - BLOCK * np.arange(Bx))
    return (hs[:, None] * ws[None, :]).astype(np.int32)


def per_pixel(blocks, H, W):
    """[By,Bx,...] -> [H,W,...]: every pixel gets its block's value"""
    return np.repeat(np.repeat(blocks, BLOCK, 0), BLOCK, 1)[:H, :W]


def luma_host(rgb):
    """uint8 [...,H,W,3] -> uint8 [...,H,W]"""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim < 3 or rgb.shape[-1] != 3:
        raise ValueError(f'luma_host: expected uint8 [H,W,3], got {rgb.dtype} {rgb.shape}')
    c = rgb.astype(np.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def block_motion_host(cur, ref, search=SEARCH, bias=BIAS):
    """The definition above: uint8 [H,W] twice -> (vec int8 [By,Bx,2] as (dy, dx), sad int32 [By,Bx])"""
    cur, ref = np.asarray(cur), np.asarray(ref)
    if cur.dtype != np.uint8 or ref.dtype != np.uint8 or cur.ndim != 2 or cur.size == 0 or ref.shape != cur.shape:
        raise ValueError(f'block_motion_host: cur and ref must be uint8 [H,W] of one shape, got {cur.dtype} {cur.shape} and {ref.dtype} {ref.shape}')
    S = _int_in('block_motion_host', 'search', search, 1, MAX_SEARCH)
    bias = _int_in('block_motion_host', 'bias', bias, 0, 255)
    H, W = cur.shape
    By, Bx = blocks_of(H, W)
    vec = np.zeros((By, Bx, 2), np.int8)
    sad = np.zeros((By, Bx), np.int32)
    c, r = cur.astype(np.int16), ref.astype(np.int16)
    for by in range(By):
        y0, y1 = by * BLOCK, min(H, by * BLOCK + BLOCK)
        for bx in range(Bx):
            x0, x1 = bx * BLOCK, min(W, bx * BLOCK + BLOCK)
            blk = c[y0:y1, x0:x1]
            dys = np.arange(max(-S, -y0), min(S, H - y1) + 1)
            dxs = np.arange(max(-S, -x0), min(S, W - x1) + 1)
            # every in-bounds displaced block at once: [ndy, ndx, h, w] windows of ref
            win = np.lib.stride_tricks.sliding_window_view(r[y0 + dys[0]:y1 + dys[-1], x0 + dxs[0]:x1 + dxs[-1]], blk.shape)
            cost = np.abs(win - blk).sum((2, 3), dtype=np.int32)
            key = (cost.astype(np.int64) << 32) | ((dys[:, None] ** 2 + dxs[None, :] ** 2) << 16) | ((dys[:, None] + 32) << 8) | (dxs[None, :] + 32)
            i, j = np.unravel_index(key.argmin(), key.shape)
            zero = int(cost[-dys[0], -dxs[0]])
            if zero - int(cost[i, j]) <= bias * blk.size:
                sad[by, bx] = zero
            else:
                vec[by, bx] = (dys[i], dxs[j])
                sad[by, bx] = cost[i, j]
    return vec, sad
