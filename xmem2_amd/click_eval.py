"""Robot-click evaluation (NoC) on MI355X: the reference's fbrs Clicker, evaluate_sample / evaluate_dataset and NoC helpers
(inference/interact/fbrs/inference/clicker.py, evaluation.py, utils.py) with the robot on the device.

    python -m xmem2_amd.click_eval --images DIR --masks DIR (--model fbrs.pth | --synthetic-seed N) [--brs-mode NoBRS|f-BRS-B|f-BRS-C]
                                   [--max-clicks 20] [--iou-thrs 0.8 0.85 0.9] [--clicks-out FILE.json] [--out DIR]

``Clicker`` is the robot user: given the ground truth it clicks the point of the largest error region of a prediction that lies
deepest inside it.  The reference takes two float64 scipy distance transforms of the padded error planes on the host; here the
planes, their exact integer squared distance transform, the arg-max and the IoU counts are HIP kernels (csrc/edt.hip through
ops.click_errors, ops.edt_sq, ops.next_click) and one 32-byte record comes back per click - the probability map stays on the device.
Squared integer distances order exactly as their float64 roots, ties resolve to the smallest row-major index as np.where does, and
`fn_max > fp_max` is strict (a tie, 0 == 0 when the prediction is right included, is a negative click): the clicks are the
reference's, bit for bit.

The command line makes one sample of every labelled frame and object k (ground truth: index == k, 255 = ignore), runs the predictor
FBRSController / FeatureBRSController configure, and prints the NoC table.  --clicks-out writes the JSON `python -m xmem2_amd.click`
reads (the same clicks give the same masks); --out writes the palette masks, committed object by object as click.py does.
"""
import argparse
import json
import os
import sys
import time
from datetime import timedelta

import numpy as np
import torch

from . import ops
from .click import Click

IGNORE_U8 = 255                 # the ignore value of the uint8 ground truth on the device (csrc/edt.hip)


def _device_of(t=None):
    if isinstance(t, torch.Tensor) and t.is_cuda:
        return t.device
    return torch.device('cuda', torch.cuda.current_device())


def _gt_u8(gt_mask, ignore_label, device):
    """uint8 [H,W] on the device: 1 where gt_mask == 1, 255 where gt_mask == ignore_label, else 0 (uploaded / converted once)."""
    if isinstance(gt_mask, torch.Tensor):
        g = gt_mask.to(device)
        out = (g == 1).to(torch.uint8)
        representable = g.dtype not in (torch.uint8, torch.bool) or 0 <= ignore_label <= 255       # -1 never occurs in a uint8 map
        if ignore_label != 1 and representable:
            out = out + (g == ignore_label).to(torch.uint8) * IGNORE_U8
    else:
        g = np.asarray(gt_mask)
        host = (g == 1).astype(np.uint8)
        host[(g == ignore_label) & (g != 1)] = IGNORE_U8
        out = torch.from_numpy(host).to(device)
    if out.dim() != 2:
        raise ValueError(f'the ground truth must be [H,W], got {tuple(out.shape)}')
    return out.contiguous()


def _pred_arg(pred, pred_thr, shape, device):
    """(tensor, threshold or None) as ops.click_errors takes a prediction: a float32 probability map with its threshold, or a uint8 mask."""
    if not isinstance(pred, torch.Tensor):
        pred = torch.from_numpy(np.ascontiguousarray(pred))
    if pred.numel() != shape[0] * shape[1]:
        raise ValueError(f'prediction {tuple(pred.shape)} and ground truth {tuple(shape)} differ in size')
    pred = pred.reshape(shape)
    if pred.dtype in (torch.float32, torch.float64, torch.float16) and pred_thr is not None:
        return pred.to(device, torch.float32), float(pred_thr)
    if pred.dtype.is_floating_point:
        raise ValueError('a probability map needs pred_thr (a boolean or uint8 mask does not)')
    return (pred != 0).to(device, torch.uint8) if pred.dtype != torch.uint8 else pred.to(device), None


def _iou_of(inter, union):
    return np.float64(inter) / np.float64(union) if union else np.float64('nan')


class Clicker:
    """fbrs/inference/clicker.py with the ground truth, `not_clicked` and every distance on the device.  gt_mask: numpy or a tensor,
    1 = object, ignore_label = ignore, anything else background.  Clicks are click.Click(is_positive, (row, col)) with Python ints."""

    def __init__(self, gt_mask=None, init_clicks=None, ignore_label=-1):
        self.gt_mask = None
        self.last_iou = None        # IoU of the prediction the last make_next_click saw
        self.last_record = None     # its record: (is_positive, row, col, fn_max_d2, fp_max_d2, inter, union, 0)
        if gt_mask is not None:
            self.device = _device_of(gt_mask)
            with torch.cuda.device(self.device):
                self.gt_mask = _gt_u8(gt_mask, ignore_label, self.device)
                H, W = self.gt_mask.shape
                self.not_clicked_map = torch.empty((H, W), dtype=torch.uint8, device=self.device)
                self._planes = torch.empty((2, H, W), dtype=torch.uint8, device=self.device)
                self._d2 = torch.empty((2, H, W), dtype=torch.int32, device=self.device)
                self._counts = torch.empty(2, dtype=torch.int32, device=self.device)
                self._record = torch.empty(ops.CLICK_RECORD, dtype=torch.int32, device=self.device)
        self.reset_clicks()
        for click in init_clicks or ():
            self.add_click(click)

    def make_next_click(self, pred, pred_thr=None):
        """pred: a probability map on the device with pred_thr (pred > pred_thr), or a boolean / uint8 mask.  Five launches and one
        copy of the record; not_clicked is updated by the kernel."""
        if self.gt_mask is None:
            raise RuntimeError('Clicker: make_next_click needs a ground truth')
        with torch.cuda.device(self.device):
            pred, thr = _pred_arg(pred, pred_thr, self.gt_mask.shape, self.device)
            ops.click_errors(pred, self.gt_mask, thr, planes=self._planes, counts=self._counts)
            ops.edt_sq(self._planes, out=self._d2)
            ops.next_click(self._d2, self.not_clicked_map, self._counts, record=self._record)
            rec = [int(v) for v in self._record.cpu().numpy()]
        self.last_record = rec
        self.last_iou = _iou_of(rec[5], rec[6])
        self._append(Click(bool(rec[0]), (rec[1], rec[2])))

    def get_clicks(self, clicks_limit=None):
        return self.clicks_list[:clicks_limit]

    def _append(self, click):
        if click.is_positive:
            self.num_pos_clicks += 1
        else:
            self.num_neg_clicks += 1
        self.clicks_list.append(click)

    def _mark(self, click, value):
        if self.gt_mask is not None:
            self.not_clicked_map[int(click.coords[0]), int(click.coords[1])] = value

    def add_click(self, click):
        self._append(click)
        self._mark(click, 0)

    def _remove_last_click(self):
        click = self.clicks_list.pop()
        if click.is_positive:
            self.num_pos_clicks -= 1
        else:
            self.num_neg_clicks -= 1
        self._mark(click, 1)

    def reset_clicks(self):
        if self.gt_mask is not None:
            self.not_clicked_map.fill_(1)
        self.num_pos_clicks = 0
        self.num_neg_clicks = 0
        self.clicks_list = []

    def get_state(self):
        return list(self.clicks_list)

    def set_state(self, state):
        self.reset_clicks()
        for click in state:
            self.add_click(click)

    def __len__(self):
        return len(self.clicks_list)


def get_iou(gt_mask, pred_mask, ignore_label=-1, pred_thr=None):
    """utils.get_iou: |pred & gt| / |pred | gt| outside the ignore label, float64 (NaN for an empty union).  numpy arrays are scored
    on the host; with a device tensor on either side the counts come from ops.click_errors (8 bytes to the host) and the division
    is the same.  `pred_thr` lets pred_mask be a probability map (pred > pred_thr)."""
    if not isinstance(gt_mask, torch.Tensor) and not isinstance(pred_mask, torch.Tensor):
        gt, pred = np.asarray(gt_mask), np.asarray(pred_mask)
        pred = pred > pred_thr if pred_thr is not None else pred.astype(bool)
        obj, valid = gt == 1, gt != ignore_label
        return _iou_of(int((pred & obj & valid).sum()), int(((pred | obj) & valid).sum()))
    device = _device_of(gt_mask if isinstance(gt_mask, torch.Tensor) and gt_mask.is_cuda else pred_mask)
    with torch.cuda.device(device):
        return _device_iou(_gt_u8(gt_mask, ignore_label, device), pred_mask, pred_thr)


def _device_iou(gt_u8, pred, pred_thr):
    pred, thr = _pred_arg(pred, pred_thr, gt_u8.shape, gt_u8.device)
    inter, union = (int(v) for v in ops.click_errors(pred, gt_u8, thr)[1].cpu().numpy())
    return _iou_of(inter, union)


def evaluate_sample(image, gt_mask, predictor, max_iou_thr, pred_thr=0.49, max_clicks=20):
    """evaluation.evaluate_sample with a click.NoBRSPredictor or click_brs.FeatureBRSPredictor: starting from an empty prediction, the
    robot clicks, the predictor answers, the IoU of the answer is taken and the loop stops at iou >= max_iou_thr or after max_clicks.
    image [3,H,W] (normalised) on the device.  -> (clicks_list, ious float32 [n], pred_probs [H,W] on the device).

    The record of a robot step carries the IoU counts of the prediction it clicked on, so the IoU of answer n arrives with click
    n + 1: the click is made ahead and taken back when the loop stops there (one 32-byte copy per step either way)."""
    clicker = Clicker(gt_mask=gt_mask)
    ious = []
    pred_probs = None
    with torch.no_grad(), torch.cuda.device(clicker.device):
        predictor.set_input_image(image)
        clicker.make_next_click(torch.zeros(clicker.gt_mask.shape, dtype=torch.uint8, device=clicker.device))
        for n in range(max_clicks):
            pred_probs = predictor.get_prediction(clicker.get_clicks())
            if n + 1 == max_clicks:
                ious.append(_device_iou(clicker.gt_mask, pred_probs, pred_thr))
                break
            clicker.make_next_click(pred_probs, pred_thr)
            ious.append(clicker.last_iou)
            if clicker.last_iou >= max_iou_thr:
                clicker._remove_last_click()
                break
    return clicker.clicks_list, np.array(ious, dtype=np.float32), pred_probs


def evaluate_dataset(samples, predictor, oracle_eval=False, **kwargs):
    """samples: an iterable of (image, gt_mask) -> (all_ious, elapsed seconds)."""
    if oracle_eval:
        raise NotImplementedError('evaluate_dataset: oracle_eval needs the ground-truth mask loss of the reference, which is not built')
    all_ious = []
    start = time.time()
    for image, gt_mask in samples:
        all_ious.append(evaluate_sample(image, gt_mask, predictor, **kwargs)[1])
    torch.cuda.synchronize()
    return all_ious, time.time() - start


# ---- metric helpers (fbrs/inference/utils.py) ------------------------------------------------------------------------------

def compute_noc_metric(all_ious, iou_thrs, max_clicks=20):
    """Per threshold: (mean number of clicks to reach it, a run that never does counting max_clicks; the number of runs at max_clicks)."""
    noc_list, over_max_list = [], []
    for thr in iou_thrs:
        scores = []
        for ious in all_ious:
            reached = np.asarray(ious) >= thr
            scores.append(int(np.argmax(reached)) + 1 if reached.any() else max_clicks)
        scores = np.array(scores, dtype=np.int64)
        noc_list.append(scores.mean())
        over_max_list.append((scores == max_clicks).sum())
    return noc_list, over_max_list


def get_time_metrics(all_ious, elapsed_time):
    """(seconds per click, seconds per image)"""
    return elapsed_time / sum(len(v) for v in all_ious), elapsed_time / len(all_ious)


def get_results_table(noc_list, over_max_list, brs_type, dataset_name, mean_spc, elapsed_time, n_clicks=20, model_name=None):
    """(header, row) of the reference's results table: NoC@80/85/90, the runs that reached n_clicks at 85 / 90, seconds per click."""
    cols = [f'{"BRS Type":^13}', f'{"Dataset":^11}', f'{"NoC@80%":^9}', f'{"NoC@85%":^9}', f'{"NoC@90%":^9}',
            f'{">=" + str(n_clicks) + "@85%":^9}', f'{">=" + str(n_clicks) + "@90%":^9}', f'{"SPC,s":^7}', f'{"Time":^9}']
    head = '|' + '|'.join(cols) + '|'
    rule = '-' * len(head)
    header = (f'Eval results for model: {model_name}\n' if model_name is not None else '') + rule + '\n' + head + '\n' + rule
    n = len(noc_list)
    cells = [f'{brs_type:^13}', f'{dataset_name:^11}', f'{noc_list[0]:^9.2f}',
             f'{noc_list[1]:^9.2f}' if n > 1 else f'{"?":^9}', f'{noc_list[2]:^9.2f}' if n > 2 else f'{"?":^9}',
             f'{over_max_list[1]:^9}' if n > 1 else f'{"?":^9}', f'{over_max_list[2]:^9}' if n > 2 else f'{"?":^9}',
             f'{mean_spc:^7.3f}', f'{str(timedelta(seconds=int(elapsed_time))):^9}']
    return header, '|' + '|'.join(cells) + '|'


# ---- command line ------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m xmem2_amd.click_eval', description='Robot-click evaluation: NoC of the click tool '
                                 'against ground-truth masks.')
    ap.add_argument('--images', required=True, help='directory of frames')
    ap.add_argument('--masks', required=True, help='directory of indexed ground-truth masks (k = object, 0 = background, 255 = ignore)')
    src = ap.add_mutually_exclusive_group()
    src.add_argument('--model', default=None, help='click-network checkpoint (saves/fbrs.pth)')
    src.add_argument('--synthetic-seed', type=int, default=None, help='conditioned synthetic weights instead of a checkpoint')
    ap.add_argument('--brs-mode', choices=('NoBRS', 'f-BRS-B', 'f-BRS-C'), default='NoBRS')
    ap.add_argument('--max-clicks', type=int, default=20)
    ap.add_argument('--iou-thrs', type=float, nargs='+', default=[0.8, 0.85, 0.9], help='one to three IoU thresholds, ascending')
    ap.add_argument('--clicks-out', default=None, help='write the clicks as the JSON python -m xmem2_amd.click reads')
    ap.add_argument('--out', default=None, help='output directory for the palette masks of the last predictions')
    args = ap.parse_args(argv)
    if args.model is None and args.synthetic_seed is None:
        ap.error('one of --model or --synthetic-seed is required')
    if args.model is not None and not os.path.isfile(args.model):
        ap.error(f'--model: no such file: {args.model}')
    for name in ('images', 'masks'):
        if not os.path.isdir(getattr(args, name)):
            ap.error(f'--{name}: not a directory: {getattr(args, name)}')
    if args.max_clicks < 1:
        ap.error('--max-clicks must be at least 1')
    if not 1 <= len(args.iou_thrs) <= 3 or any(not 0.0 < t <= 1.0 for t in args.iou_thrs) or sorted(args.iou_thrs) != args.iou_thrs:
        ap.error('--iou-thrs: one to three ascending values in (0, 1]')
    return args


def clicks_json(per_frame):
    """{frame number: [(object, Click), ...]} -> the document click.load_clicks accepts."""
    return {str(n): [{'object': int(k), 'x': int(c.coords[1]), 'y': int(c.coords[0]), 'positive': bool(c.is_positive)} for k, c in rows]
            for n, rows in sorted(per_frame.items()) if rows}


def main(argv=None):
    args = parse_args(argv)
    from .click import ClickNet
    torch.set_grad_enabled(False)
    net = ClickNet(device=torch.device('cuda', torch.cuda.current_device()))
    if args.model:
        net.load_weights(args.model)
    else:
        from .synth import synthetic_click_state_dict
        net.load_state_dict(synthetic_click_state_dict(args.synthetic_seed))
    return run(args, net)


def run(args, net):
    """The command line after its arguments are parsed and its click network `net` is loaded."""
    from PIL import Image
    from .click import FBRSController, click_commit
    from .scribble import IM_MEAN, IM_STD, _load_index, _palette, index_dir
    imgs, masks = index_dir(args.images), index_dir(args.masks, ('.png',))
    missing = sorted(set(masks) - set(imgs))
    if missing:
        raise FileNotFoundError(f'masks without a frame: numbers {missing[:10]}')
    if not masks:
        print('no ground-truth masks found', file=sys.stderr)
        return 1
    device = net.device
    if args.brs_mode == 'NoBRS':
        ctl = FBRSController(net, device=device)
    else:
        from .click_brs import FeatureBRSController
        ctl = FeatureBRSController(net, device=device, brs_mode=args.brs_mode)
    ctl._reset_predictor()                      # the predictor as the controller configures it (zoom-in, flip, clicks limit)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    pal = _palette()
    all_ious, per_frame = [], {}
    start = time.time()
    for n in sorted(masks):
        img = np.array(Image.open(os.path.join(args.images, imgs[n])).convert('RGB'), dtype=np.uint8)
        index = _load_index(os.path.join(args.masks, masks[n]))
        if index.shape != img.shape[:2]:
            raise ValueError(f'frame {n}: image {img.shape[:2]} and mask {index.shape} differ in size')
        labels = [int(v) for v in np.unique(index) if 0 < v < 255]
        if not labels:
            continue
        image = torch.from_numpy(((img.astype(np.float32) / 255.0 - IM_MEAN) / IM_STD).transpose(2, 0, 1).copy()).to(device)
        K = max(labels)
        prob = torch.zeros((K + 1,) + index.shape, dtype=torch.float32, device=device)
        prob[0] = 1
        mask = None
        rows = per_frame.setdefault(n, [])
        for k in labels:
            gt = np.where(index == 255, -1, index == k).astype(np.int32)
            clicks, ious, pred = evaluate_sample(image, gt, ctl.predictor, max(args.iou_thrs), max_clicks=args.max_clicks)
            all_ious.append(ious)
            rows.extend((k, c) for c in clicks)
            if args.out:
                prob, mask = click_commit(prob, ops.prob_threshold(pred, 0.5), k)
        if args.out and mask is not None:
            out = Image.fromarray(mask.cpu().numpy(), mode='P')
            out.putpalette(pal)
            out.save(os.path.join(args.out, os.path.splitext(imgs[n])[0] + '.png'))
    torch.cuda.synchronize()
    elapsed = time.time() - start
    if not all_ious:
        print('no labelled object found', file=sys.stderr)
        return 1
    if args.clicks_out:
        with open(args.clicks_out, 'w') as f:
            json.dump(clicks_json(per_frame), f, indent=1)
            f.write('\n')
    noc, over = compute_noc_metric(all_ious, args.iou_thrs, max_clicks=args.max_clicks)
    spc, _spi = get_time_metrics(all_ious, elapsed)
    header, row = get_results_table(noc, over, args.brs_mode, os.path.basename(os.path.normpath(args.masks))[:11], spc, elapsed,
                                    n_clicks=args.max_clicks, model_name=args.model or f'synthetic seed {args.synthetic_seed}')
    print(header)
    print(row)
    return 0


if __name__ == '__main__':
    sys.exit(main())
