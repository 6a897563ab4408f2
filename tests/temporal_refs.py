"""An oracle for the temporal majority vote that shares no code with `xmem2_amd.temporal.mode_host`: one one-hot plane per label,
summed over the clipped window of present frames by differences of a running sum, and the winner picked by the key
(count, is the centre's label, -label) in plain Python order."""
import numpy as np


def mode_oracle(masks, radius, present=None, locked=None):
    masks = np.asarray(masks, np.uint8)
    T = masks.shape[0]
    present = np.ones(T, bool) if present is None else np.asarray(present, bool)
    locked = np.zeros(T, bool) if locked is None else np.asarray(locked, bool)
    labels = [int(v) for v in np.unique(masks)]
    onehot = np.stack([(masks == lab) & present[:, None, None] for lab in labels]).astype(np.int64)     # [L,T,H,W]
    run = np.concatenate([np.zeros_like(onehot[:, :1]), np.cumsum(onehot, axis=1)], axis=1)            # run[:, t] = sum of frames < t
    out = masks.copy()
    changed = np.zeros(T, np.int64)
    for t in range(T):
        if not present[t] or locked[t]:
            continue
        a, b = max(0, t - radius), min(T - 1, t + radius)
        counts = run[:, b + 1] - run[:, a]                                                              # [L,H,W]
        for y in range(masks.shape[1]):
            for x in range(masks.shape[2]):
                centre = int(masks[t, y, x])
                best = max(range(len(labels)), key=lambda i: (int(counts[i, y, x]), labels[i] == centre, -labels[i]))
                out[t, y, x] = labels[best]
        changed[t] = int(np.count_nonzero(out[t] != masks[t]))
    return out, changed


def flicker_stack(rng, T, H, W, labels=(0, 1, 127, 128, 255), flips=0.15, run=6):
    """uint8 [T,H,W] with long constant runs in time and single-frame flips: a vote changes pixels of it"""
    labels = np.asarray(labels, np.uint8)
    out = np.empty((T, H, W), np.uint8)
    cur = labels[rng.integers(0, len(labels), (H, W))]
    for t in range(T):
        move = rng.random((H, W)) < 1.0 / run
        cur = np.where(move, labels[rng.integers(0, len(labels), (H, W))], cur)
        flip = rng.random((H, W)) < flips
        out[t] = np.where(flip, labels[rng.integers(0, len(labels), (H, W))], cur)
    return out
