"""Oracles for the block-motion search and the motion-compensated vote that share no code with `xmem2_amd.motion` and
`xmem2_amd.temporal`: the search loops over blocks, candidates and pixels in plain Python and compares (SAD, d^2, dy, dx) tuples; the
vote counts one-hot planes per label over the entries that vote and picks by (count, is the centre's label, -label).  Also the
inputs the host and the device tests share."""
import numpy as np

B = 16


def motion_oracle(cur, ref, search, bias):
    H, W = cur.shape
    By, Bx = -(-H // B), -(-W // B)
    vec = np.zeros((By, Bx, 2), np.int8)
    sad = np.zeros((By, Bx), np.int32)
    c, r = cur.tolist(), ref.tolist()
    for by in range(By):
        for bx in range(Bx):
            ys = range(by * B, min(H, by * B + B))
            xs = range(bx * B, min(W, bx * B + B))
            best = zero = None
            for dy in range(-search, search + 1):
                if ys[0] + dy < 0 or ys[-1] + dy >= H:
                    continue
                for dx in range(-search, search + 1):
                    if xs[0] + dx < 0 or xs[-1] + dx >= W:
                        continue
                    s = 0
                    for y in ys:
                        cr, rr = c[y], r[y + dy]
                        for x in xs:
                            s += abs(cr[x] - rr[x + dx])
                    if best is None or (s, dy * dy + dx * dx, dy, dx) < best:
                        best = (s, dy * dy + dx * dx, dy, dx)
                    if dy == 0 and dx == 0:
                        zero = s
            if zero - best[0] <= bias * len(ys) * len(xs):
                best = (zero, 0, 0, 0)
            vec[by, bx] = best[2:]
            sad[by, bx] = best[0]
    return vec, sad


def mode_mc_oracle(masks, luma, radius, search, bias, max_sad, present=None, locked=None, search_fn=motion_oracle):
    T, H, W = masks.shape
    present = np.ones(T, bool) if present is None else np.asarray(present, bool)
    locked = np.zeros(T, bool) if locked is None else np.asarray(locked, bool)
    labels = [int(v) for v in np.unique(masks)]
    out = masks.copy()
    changed = np.zeros(T, np.int64)
    for t in range(T):
        if not present[t] or locked[t]:
            continue
        counts = np.stack([(masks[t] == lab) for lab in labels]).astype(np.int64)            # the centre votes with its own pixel
        for f in range(max(0, t - radius), min(T - 1, t + radius) + 1):
            if f == t or not present[f]:
                continue
            vec, sad = search_fn(luma[t], luma[f], search, bias)
            for y in range(H):
                for x in range(W):
                    by, bx = y // B, x // B
                    n = (min(H, by * B + B) - by * B) * (min(W, bx * B + B) - bx * B)
                    if sad[by, bx] > max_sad * n:
                        continue
                    counts[labels.index(int(masks[f, y + vec[by, bx, 0], x + vec[by, bx, 1]])), y, x] += 1
        for y in range(H):
            for x in range(W):
                centre = int(masks[t, y, x])
                best = max(range(len(labels)), key=lambda i: (int(counts[i, y, x]), labels[i] == centre, -labels[i]))
                out[t, y, x] = labels[best]
        changed[t] = int(np.count_nonzero(out[t] != masks[t]))
    return out, changed


def shifted_pair(rng, H, W, dy, dx):
    """(cur, ref) with ref[y + dy, x + dx] == cur[y, x] wherever both exist: random texture, no two blocks alike"""
    big = rng.integers(0, 256, (H + 128, W + 128), dtype=np.uint8)
    return big[64:64 + H, 64:64 + W].copy(), big[64 - dy:64 - dy + H, 64 - dx:64 - dx + W].copy()


def stripes(H, W, phase=0):
    """vertical stripes of period 4.  Against the same stripes two columns out of phase every dx = 2 (mod 4) and every dy costs
    nothing: d^2 picks |dx| = 2 and dy = 0, and dx = -2 wins over dx = +2 where both are in bounds"""
    return np.broadcast_to(((np.arange(W) + phase) % 4 * 60).astype(np.uint8), (H, W)).copy()


def bias_block(extra):
    """a 48 x 48 pair whose block (1, 1) has SAD(0, 0) = 2 * 256 + extra (extra 0 or 1) and SAD(0, 1) = 0: a ramp of 2 per column,
    the block of `cur` one column ahead; `extra` is taken off the one pixel of `ref` that only the candidate (0, 0) sees"""
    ref = np.broadcast_to((2 * np.arange(48) + 10).astype(np.uint8), (48, 48)).copy()
    cur = ref.copy()
    cur[16:32, 16:32] = ref[16:32, 17:33]
    ref[16, 16] -= extra                                                 # cur[16, 16] - ref[16, 16] becomes 2 + extra
    return cur, ref


def pan_clip(T=5, H=80, W=112, pan=(2, -3), seed=0):
    """(luma [T,H,W], clean masks, noisy masks): a texture and an object of labels 1 and 2 that pan together; a 5 x 5 patch of
    label 1 is zeroed in frame 2 of `noisy`"""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (H + 64, W + 64), dtype=np.uint8)
    obj = np.zeros((H + 64, W + 64), np.uint8)
    obj[60:85, 70:100] = 1
    obj[70:80, 80:95] = 2
    cut = lambda a, t: a[32 - pan[0] * t:32 - pan[0] * t + H, 32 - pan[1] * t:32 - pan[1] * t + W]
    luma = np.stack([cut(big, t) for t in range(T)])
    masks = np.stack([cut(obj, t) for t in range(T)])
    noisy = masks.copy()
    ys, xs = np.argwhere(masks[2] == 1)[40]
    noisy[2, ys:ys + 5, xs:xs + 5] = 0
    return luma, masks, noisy


SIZES = [(1, 1), (15, 17), (16, 16), (33, 50)]
SEARCHES = [1, 7, 32]


def shift_for(search):
    return min(search, 2), -min(search, 3)


def search_cases():
    """(name, cur, ref, search, bias) of every pair the search is held to, on the host and on the device"""
    for H, W in SIZES:
        for S in SEARCHES:
            rng = np.random.default_rng(H * 1000 + W * 10 + S)
            yield (f'shift {H}x{W} s{S}',) + shifted_pair(rng, H, W, *shift_for(S)) + (S, 1)
            yield f'constant {H}x{W} s{S}', np.full((H, W), 77, np.uint8), np.full((H, W), 200, np.uint8), S, 1
            yield f'stripes {H}x{W} s{S}', stripes(H, W), stripes(H, W, 2), S, 0
            yield f'rows {H}x{W} s{S}', stripes(W, H).T.copy(), stripes(W, H, 2).T.copy(), S, 0      # the same for dy
    for extra in (0, 1):
        yield (f'bias +{extra}',) + bias_block(extra) + (7, 2)


# ---- a clip whose masks flicker under the synthetic network: two objects with labels 2 and 5 on a texture that moves a pixel a frame

FLICKER_T, FLICKER_HW = 10, (96, 128)
FLICKER_LABELS = (2, 5)                                       # dense ids 1 and 2
FLICKER_COLOURS = {2: (200, 0, 0), 5: (0, 200, 0)}
FLICKER_GIVEN = [0, 4]
FLICKER_LUT = np.array((0,) + FLICKER_LABELS, np.uint8)


def make_flicker_clip(root, T=FLICKER_T):
    """(frames dir, annotations dir, names, lumas uint8 [T,H,W] of the written frames)"""
    from PIL import Image
    from xmem2_amd.motion import luma_host
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    imgs, msks = root / 'JPEGImages', root / 'Annotations'
    imgs.mkdir(); msks.mkdir()
    frames, masks = synthetic_frames(T, *FLICKER_HW, seed=1234), synthetic_masks(T, 2, *FLICKER_HW)
    pal = [0] * 768
    for lab, rgb in FLICKER_COLOURS.items():
        pal[3 * lab:3 * lab + 3] = rgb
    names, lumas = [f'frame_{i:06d}.png' for i in range(T)], []
    for i, name in enumerate(names):
        rgb = np.clip((frames[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(imgs / name)
        lumas.append(luma_host(rgb))
        idx = np.zeros(FLICKER_HW, np.uint8)
        for o, lab in enumerate(FLICKER_LABELS):
            idx[masks[i, o] > 0] = lab
        im = Image.fromarray(idx, mode='P'); im.putpalette(pal); im.save(msks / name)
    return str(imgs), str(msks), names, np.stack(lumas)


def flicker_written_ids(out_dir, names):
    """the written mask PNGs of a run on that clip mapped to dense ids, uint8 [T,H,W]"""
    import os
    from PIL import Image
    ids = []
    for n in names:
        rgb = np.array(Image.open(os.path.join(str(out_dir), 'masks', n)).convert('RGB'))
        m = np.zeros(rgb.shape[:2], np.uint8)
        for dense, lab in enumerate(FLICKER_LABELS, start=1):
            m[(rgb == np.array(FLICKER_COLOURS[lab], np.uint8)).all(-1)] = dense
        assert ((m > 0) == rgb.any(-1)).all(), n
        ids.append(m)
    return np.stack(ids)


def flicker_locked(T=FLICKER_T):
    return [t in FLICKER_GIVEN for t in range(T)]
