"""numpy / scipy restatements of the robot user of click evaluation (the reference's fbrs Clicker and get_iou), shared by
test_click_eval_host.py and test_gpu_click_eval.py.  Two forms of the same choice: `next_click_scipy` as the reference words it (float64
distance_transform_edt of the padded error planes), and `next_click_int` on the integer squared distances `edt_sq_int` the HIP
kernels compute.  gt holds 1 = object, `ignore_label` = ignore, anything else = background."""
import numpy as np

IGNORE = -1


def edt_sq_int(mask):
    """int32 [H,W]: squared Euclidean distance of every non-zero pixel of `mask` to the nearest zero pixel of the plane or of a ring
    of zeros around it (0 where mask is 0), by the separable integer form: column distance g, then min over x' of (x - x')^2 + g^2."""
    m = np.pad(np.asarray(mask) != 0, 1)
    Hp, Wp = m.shape
    rows = np.arange(Hp, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(~m, rows, -1), 0)               # every padded column starts and ends with a zero
    dn = np.minimum.accumulate(np.where(~m, rows, Hp)[::-1], 0)[::-1]
    g2 = np.minimum(rows - up, dn - rows) ** 2
    xs = np.arange(Wp, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2
    out = np.empty((Hp, Wp), np.int64)
    for y in range(Hp):
        out[y] = (dx2 + g2[y][None, :]).min(1)
    return out[1:-1, 1:-1].astype(np.int32)


def error_planes(gt, pred, ignore_label=IGNORE):
    gt, pred = np.asarray(gt), np.asarray(pred).astype(bool)
    obj, valid = gt == 1, gt != ignore_label
    return obj & ~pred & valid, ~obj & pred & valid


def get_iou(gt, pred, ignore_label=IGNORE):
    gt, pred = np.asarray(gt), np.asarray(pred).astype(bool)
    obj, valid = gt == 1, gt != ignore_label
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.float64((pred & obj & valid).sum()) / np.float64(((pred | obj) & valid).sum())


def iou_counts(gt, pred, ignore_label=IGNORE):
    gt, pred = np.asarray(gt), np.asarray(pred).astype(bool)
    obj, valid = gt == 1, gt != ignore_label
    return int((pred & obj & valid).sum()), int(((pred | obj) & valid).sum())


def _pick(fn_d, fp_d):
    fn_max, fp_max = fn_d.max(), fp_d.max()
    positive = bool(fn_max > fp_max)
    ys, xs = np.where(fn_d == fn_max) if positive else np.where(fp_d == fp_max)
    return positive, (int(ys[0]), int(xs[0]))


def next_click_scipy(gt, pred, not_clicked, ignore_label=IGNORE):
    from scipy.ndimage import distance_transform_edt
    fn, fp = error_planes(gt, pred, ignore_label)
    d = [distance_transform_edt(np.pad(p, ((1, 1), (1, 1)), 'constant'))[1:-1, 1:-1] * not_clicked for p in (fn, fp)]
    return _pick(*d)


def next_click_int(gt, pred, not_clicked, ignore_label=IGNORE):
    fn, fp = error_planes(gt, pred, ignore_label)
    return _pick(edt_sq_int(fn) * not_clicked, edt_sq_int(fp) * not_clicked)


def successive_clicks(gt, pred, n, chooser=next_click_int, ignore_label=IGNORE, clicks=()):
    """The next n clicks on the same prediction after `clicks` ((is_positive, (row, col)) each) as an int array [n,3]."""
    not_clicked = np.ones(np.asarray(gt).shape, bool)
    for _p, (r, c) in clicks:
        not_clicked[r, c] = False
    out = []
    for _ in range(n):
        positive, (r, c) = chooser(gt, pred, not_clicked, ignore_label)
        not_clicked[r, c] = False
        out.append((int(positive), r, c))
    return np.array(out, np.int32).reshape(n, 3)
