"""f-BRS click refinement on MI355X: the reference's FeatureBRSPredictor with its ScaleBiasOptimizer and BRSMaskLoss
(inference/interact/fbrs/inference/predictors/brs.py:54-140, brs_functors.py:8-109, brs_losses.py:6-26, __init__.py:42-71).

From the second click on the reference does not just run the network: it optimises a per-channel scale and bias on one feature
map (x [2C], L-BFGS-B, at most 20 evaluations) until the mask honours every click, 3 x 3 pixels around each.  'f-BRS-B'
(`after_aspp`) acts on head_input (C = ch + 32), 'f-BRS-C' (`after_deeplab`) on the input of the SepConvHead (C = ch).  Only data
gradients are needed, no weight gradients:

    forward    y = input_data (1 + s) + b -> [_DeepLabHead ->] SepConvHead -> logits [B,h4,w4] -> upsample -> sigmoid -> loss
    backward   loss kernel (dL/dlogits through the adjoint of the upsample) -> per layer: ReLU gate, the pointwise layer transposed on
               the MFMA convolution, the depthwise layer with reversed taps -> per-channel reduction to grad [2C]

One evaluation is ONE replay of a captured HIP graph and one small device-to-host copy (the record: f, the two maxima, the
integer intersection / union counts of the new mask with the last one, grad); the host applies the reference's stop rules to the
record and swaps the best logits and the last mask with device copies.  The backward runs unconditionally - on a stop the
reference skips it, but it discards the gradient then.  Every kernel is bit-reproducible (csrc/brs.hip): the same x gives the same
f and grad, which L-BFGS and the strict `<` that keeps the best prediction depend on.

``BRSOptimizer`` is the device-free host loop (it talks to an objective with evaluate / keep_best / keep_mask), ``BRSEngine`` the
captured graphs of one network and insertion mode, ``FeatureBRSPredictor`` the predictor, ``FeatureBRSController`` FBRSController
with the reference controller's defaults.  'f-BRS-A', 'RGB-BRS' and 'DistMap-BRS' need the adjoint of the ASPP or of the whole
backbone and are not built.
"""
import numpy as np
import torch

from . import ops, stages
from .click import (BRS_MODES, CLICK_CAPACITY, MAX_GEOMETRIES, NORM_RADIUS, Click, FBRSController, NoBRSPredictor, ZoomIn, get_points_nd,
                    grown_capacity, run_click_stage)

INSERTION_MODES = {'f-BRS-B': 'after_aspp', 'f-BRS-C': 'after_deeplab'}       # predictors/__init__.py:49-53
LBFGS_DEFAULTS = {'m': 20, 'factr': 0, 'pgtol': 1e-8, 'maxfun': 20}           # predictors/__init__.py:15-20


def _fmin_l_bfgs_b():
    try:
        from scipy.optimize import fmin_l_bfgs_b
    except ImportError as e:
        raise ImportError('xmem2_amd.click_brs: the f-BRS refinement optimises with scipy.optimize.fmin_l_bfgs_b, and scipy is not '
                          "installed (brs_mode='NoBRS' needs no optimiser)") from e
    return fmin_l_bfgs_b


def lbfgs_params(overrides=None):
    """get_predictor's merge (predictors/__init__.py:15-33): the defaults, the caller's values over them, maxiter = 2 maxfun."""
    p = dict(LBFGS_DEFAULTS)
    p.update(overrides or {})
    p['maxiter'] = 2 * p['maxfun']
    return p


def flipped_clicks(clicks_list, width):
    """AddHorizontalFlip.transform's clicks of the mirrored sample (transforms/flip.py:15-17)."""
    return [Click(c.is_positive, (c.coords[0], width - c.coords[1] - 1)) for c in clicks_list]


def click_squares(clicks_lists, shape, radius=1):
    """BRSBasePredictor._get_clicks_maps_nd (brs.py:24-44) as rectangles: int32 [len(clicks_lists), n, 5] of (r0, r1, c0, c1, positive)
    per click, rows [r0, r1) x columns [c0, c1) being what the numpy slice [y - radius:y + radius + 1, x - radius:x + radius + 1]
    around (int(round(row)), int(round(col))) selects in a map of `shape`: clipped at the far edges, and EMPTY when the rounded row
    or column is below `radius`, because the slice then starts at a negative index, which numpy counts from the end."""
    H, W = int(shape[0]), int(shape[1])
    out = np.zeros((len(clicks_lists), max(1, max(len(cl) for cl in clicks_lists)), 5), np.int32)
    for i, cl in enumerate(clicks_lists):
        for k, click in enumerate(cl):
            y, x = int(round(click.coords[0])), int(round(click.coords[1]))
            r0, r1, _ = slice(y - radius, y + radius + 1).indices(H)
            c0, c1, _ = slice(x - radius, x + radius + 1).indices(W)
            out[i, k] = (r0, max(r0, r1), c0, max(c0, c1), int(bool(click.is_positive)))
    return out


# ---- the host loop ---------------------------------------------------------------------------------------------------

class BRSOptimizer:
    """ScaleBiasOptimizer.__call__ (brs_functors.py:41-77) and the L-BFGS call around it, free of any device: `objective` has
    evaluate(x float32 [2C]) -> dict(f, f_max_pos, f_max_neg, inter [B], union [B], grad [2C]) for the mask of THIS evaluation
    against the kept one, keep_best() (this evaluation's logits become the best prediction) and keep_mask() (its mask becomes the
    last mask)."""

    def __init__(self, prob_thresh=0.49, min_iou_diff=0.01, optimizer_params=None):
        self.prob_thresh, self.min_iou_diff = prob_thresh, min_iou_diff
        self.optimizer_params = lbfgs_params() if optimizer_params is None else dict(optimizer_params)
        self._minimise = _fmin_l_bfgs_b()
        self.init_click(None)

    def init_click(self, objective):
        self.objective = objective
        self.has_best = False
        self._best_loss = None
        self._has_last_mask = False
        self.evaluations = []           # per evaluation of this click: dict(x, f, stop, best); stop 0 none, 1 maxima, 2 mask IoU

    def __call__(self, x):
        x32 = np.asarray(x, np.float64).astype(np.float32)
        rec = self.objective.evaluate(x32)
        f_val = rec['f']
        best = not self.has_best or f_val < self._best_loss
        if best:
            self.objective.keep_best()
            self.has_best, self._best_loss = True, f_val
        stop = 0
        if rec['f_max_pos'] < (1 - self.prob_thresh) and rec['f_max_neg'] < self.prob_thresh:
            stop = 1
        elif self._has_last_mask and self.min_iou_diff > 0:
            iou = [i / u for i, u in zip(rec['inter'], rec['union']) if u > 0]
            if len(iou) > 0 and float(np.mean(iou)) > 1 - self.min_iou_diff:
                stop = 2
        self.evaluations.append(dict(x=x32, f=float(f_val), stop=stop, best=best))
        if stop:
            return [float(f_val), np.zeros_like(np.asarray(x, np.float64))]
        self.objective.keep_mask()
        self._has_last_mask = True
        return [float(f_val), np.asarray(rec['grad'], np.float64)]

    def minimise(self, x0):
        return self._minimise(func=self, x0=x0, **self.optimizer_params)[0]


# ---- the device side ---------------------------------------------------------------------------------------------------

class _Objective:
    """One captured objective graph with its static buffers (BRSEngine.objective)."""

    def __init__(self, feat_shape, H, W, device, cap):
        B, h4, w4, C = feat_shape
        f32 = dict(dtype=torch.float32, device=device)
        self.B, self.C, self.H, self.W, self.cap = B, C, H, W, cap
        self.x = torch.zeros(2 * C, **f32)
        self.feat = torch.zeros(feat_shape, **f32)
        self.rects = torch.zeros((B, cap, 5), dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self.last = torch.zeros((B, H, W), dtype=torch.uint8, device=device)
        self.mask = torch.zeros((B, H, W), dtype=torch.uint8, device=device)
        self.record = torch.zeros(ops.BRS_RECORD + 2 * C, **f32)
        self.logits = torch.zeros((B, h4, w4), **f32)
        self.best_logits = torch.zeros((B, h4, w4), **f32)
        self.graph = None

    def begin(self, input_data, rects):
        """A new click: the features the scale and bias act on, and the click squares [B,n,5] (click_squares)."""
        n = rects.shape[1]
        host = np.zeros((self.B, self.cap, 5), np.int32)
        host[:, :n] = rects
        self.feat.copy_(input_data)
        self.rects.copy_(torch.from_numpy(host))
        self.count.copy_(torch.from_numpy(np.array([n], np.int32)))

    def evaluate(self, x32):
        self.x.copy_(torch.from_numpy(np.ascontiguousarray(x32, np.float32)))
        self.graph.replay()
        rec = self.record.cpu().numpy()                 # the one device-to-host copy of an evaluation (it also waits for the replay)
        counts = rec[4:8].view(np.int32)
        return dict(f=rec[3], f_max_pos=rec[1], f_max_neg=rec[2], inter=[int(counts[2 * b]) for b in range(self.B)],
                    union=[int(counts[2 * b + 1]) for b in range(self.B)], grad=rec[ops.BRS_RECORD:].copy())

    def keep_best(self):
        self.best_logits.copy_(self.logits)

    def keep_mask(self):
        self.last.copy_(self.mask)


class BRSEngine:
    """The captured graphs of one ClickNet and insertion mode, least recently used dropped as ClickNet._graphs does: per working
    geometry a *features* graph (click_input -> features [-> _DeepLabHead], leaving input_data in a static buffer) and an *objective*
    graph (forward from x, loss, backward, record)."""

    def __init__(self, net, insertion_mode):
        if insertion_mode not in INSERTION_MODES.values():
            raise NotImplementedError(f'BRSEngine: insertion mode {insertion_mode!r} is not built (after_aspp, after_deeplab)')
        self.net, self.insertion_mode = net, insertion_mode
        self.num_channels = net.deeplab_ch + (32 if insertion_mode == 'after_aspp' else 0)
        self._features = stages.StageCache(lambda: MAX_GEOMETRIES)      # (h, w, with_flip) -> Stage whose output is input_data
        self._objectives = stages.StageCache(lambda: MAX_GEOMETRIES)    # (input_data shape, h, w, regulariser) -> _Objective
        self._cap = CLICK_CAPACITY

    @property
    def captures(self):
        """graphs captured so far"""
        return self._features.captures + self._objectives.captures

    def _grow(self, n):
        """Room for n clicks per sample: the captured graphs hold the old buffers and go when they grow."""
        if n > self._cap:
            self._cap = grown_capacity(self._cap, n)
            self._features.clear()
            self._objectives.clear()

    def _scope(self):
        return f'@brs#{self.net._scope}#{self.insertion_mode}#'

    # features ------------------------------------------------------------------------------------------------------------
    def _features_forward(self, image, clicks, counts, with_flip):
        net = self.net
        x = ops.click_input(image, clicks, counts, net._w['rgb_conv'], NORM_RADIUS, with_flip)
        f = net.features(x)['head_input']
        return f if self.insertion_mode == 'after_aspp' else net.deeplab_head(f)

    def features(self, image, points, with_flip=True):
        """FeatureBRSPredictor._get_head_input (brs.py:121-140): image [3,h,w] at the working size and points [2n,2] as ClickNet.run takes
        them -> input_data [B,h4,w4,C], the graph's static buffer (valid until the next call at this geometry)."""
        self.net._need_weights()
        self._grow(np.asarray(points).size // 4)
        with ops.ws_scope(self._scope()):
            return run_click_stage(self._features, self._features_forward, image, points, self._cap, with_flip)

    # objective -----------------------------------------------------------------------------------------------------------
    def _objective_forward(self, st, reg_weight, reg_bias_weight):
        net, W = self.net, self.net._w
        B, h4, w4 = st.logits.shape
        kept = []
        y = ops.brs_affine(st.feat, st.x)
        if self.insertion_mode == 'after_aspp':
            y = net.deeplab_head(y, kept)
        net.sep_conv_head(y, kept, out=st.logits.view(B, h4, w4, 1))
        dlogit = ops.brs_loss(st.logits, st.H, st.W, st.rects, st.count, st.last, st.mask, st.record)
        # backward: per layer the ReLU gate on the kept output, the pointwise layer transposed, the depthwise layer with reversed taps
        g = ops.relu_gate_outer(kept[-1], dlogit, W['head.2T'])
        g = ops.depthwise3x3(ops.conv2d(g, W['head.1.pwT']), W['head.1.dwT'])
        g = ops.relu_gate(kept[-2], g, out=g)
        g = ops.depthwise3x3(ops.conv2d(g, W['head.0.pwT']), W['head.0.dwT'])
        if self.insertion_mode == 'after_aspp':
            g = ops.conv2d(g, W['dl.2T'])
            g = ops.relu_gate(kept[1], g, out=g)
            g = ops.depthwise3x3(ops.conv2d(g, W['dl.1.pwT']), W['dl.1.dwT'])
            g = ops.relu_gate(kept[0], g, out=g)
            g = ops.depthwise3x3(ops.conv2d(g, W['dl.0.pwT']), W['dl.0.dwT'])
        ops.brs_param_grad(g, st.feat, st.x, st.record, st.record[ops.BRS_RECORD:], reg_weight, reg_bias_weight)

    def objective(self, feat_shape, H, W, num_clicks, reg_weight=1e-3, reg_bias_weight=10.0):
        """The objective of input_data shaped feat_shape [B,h4,w4,C] and a working image H x W, able to hold num_clicks squares per
        sample: get_prediction_logits + ScaleBiasOptimizer.unpack_opt_params + BRSMaskLoss and their gradient as one graph."""
        net = self.net
        net._need_weights()
        if feat_shape[3] != self.num_channels:
            raise RuntimeError(f'BRSEngine: input_data has {feat_shape[3]} channels, {self.insertion_mode} optimises {self.num_channels}')
        self._grow(num_clicks)
        key = (tuple(feat_shape), int(H), int(W), float(reg_weight), float(reg_bias_weight))
        st = self._objectives.lookup(key)
        if st is None:
            st = _Objective(tuple(feat_shape), int(H), int(W), net.device, self._cap)
            with ops.ws_scope(self._scope()):
                st.graph = stages.capture(lambda: self._objective_forward(st, reg_weight, reg_bias_weight), ()).graph
            self._objectives.put(key, st)
        return st


def engine_for(net, insertion_mode):
    """The network's engine for an insertion mode (one per network, so that controllers and anchors share its captured graphs;
    dropped with the weights by ClickNet.load_state_dict / to)."""
    eng = net._brs.get(insertion_mode)
    if eng is None:
        eng = net._brs[insertion_mode] = BRSEngine(net, insertion_mode)
    return eng


# ---- predictor and controller --------------------------------------------------------------------------------------------

class FeatureBRSPredictor(NoBRSPredictor):
    """FeatureBRSPredictor + ScaleBiasOptimizer + BRSMaskLoss for one image and one clicks list.  insertion_mode 'after_aspp' is
    f-BRS-B (C = ch + 32, on head_input), 'after_deeplab' f-BRS-C (C = ch, on the input of the SepConvHead).

    State as in the reference: opt_data [2C] starts at zero, is the warm start of the next click, is reset by set_input_image, is
    part of get_states / set_states (so undo restores it) and is NOT reset when the zoom-in changes the ROI; input_data is
    recomputed iff num_clicks <= net_clicks_limit, the working image changed, or there is none, and is not part of the states."""

    def __init__(self, net, insertion_mode='after_deeplab', net_clicks_limit=8, with_flip=True, zoom_in=None, max_size=None,
                 optimize_after_n_clicks=1, prob_thresh=0.49, min_iou_diff=0.01, reg_weight=1e-3, reg_bias_weight=10.0, scale_act=None,
                 lbfgs=None, engine=None):
        super().__init__(net, net_clicks_limit, with_flip, zoom_in, max_size)
        if scale_act is not None:
            raise NotImplementedError(f'FeatureBRSPredictor: scale_act={scale_act!r} is not built (the reference controller uses None)')
        if prob_thresh != 0.5:
            raise NotImplementedError('FeatureBRSPredictor: the mask of an evaluation is logit > 0, i.e. prob_thresh = 0.5 (the '
                                      f'reference controller\'s value), got {prob_thresh!r}')
        if not isinstance(net_clicks_limit, int):
            raise ValueError('FeatureBRSPredictor: net_clicks_limit must be an integer (the reference compares the number of clicks with it)')
        self.insertion_mode, self.optimize_after_n_clicks = insertion_mode, optimize_after_n_clicks
        self.reg_weight, self.reg_bias_weight = reg_weight, reg_bias_weight
        self.opt_functor = BRSOptimizer(prob_thresh, min_iou_diff, lbfgs_params(lbfgs))
        self.engine = engine if engine is not None else engine_for(net, insertion_mode)
        self.num_channels = self.engine.num_channels
        self.opt_data = None
        self.input_data = None

    def set_input_image(self, image):
        super().set_input_image(image)
        self.opt_data = None
        self.input_data = None

    def _predict(self, image, clicks, image_changed):
        H, W = int(image.shape[-2]), int(image.shape[-1])
        lists = [clicks] + ([flipped_clicks(clicks, W)] if self.with_flip else [])
        num_clicks = len(clicks)
        if self.opt_data is None:
            self.opt_data = np.zeros(2 * self.num_channels, np.float32)
        if num_clicks <= self.net_clicks_limit or image_changed or self.input_data is None:
            points = get_points_nd([clicks], self.net_clicks_limit)[0]
            self.input_data = self.engine.features(image, points, self.with_flip).clone()
        obj = self.engine.objective(tuple(self.input_data.shape), H, W, num_clicks, self.reg_weight, self.reg_bias_weight)
        obj.begin(self.input_data, click_squares(lists, (H, W)))
        functor = self.opt_functor
        functor.init_click(obj)
        if num_clicks > self.optimize_after_n_clicks:
            self.opt_data = functor.minimise(self.opt_data)
        if functor.has_best:
            logits = obj.best_logits
        else:
            obj.evaluate(np.asarray(self.opt_data, np.float64).astype(np.float32))
            logits = obj.logits
        return ops.click_prob(logits, H, W)

    def get_states(self):
        return {'transform_states': [t.get_state() for t in self.transforms], 'opt_data': self.opt_data}

    def set_states(self, states):
        super().set_states(states)
        self.opt_data = states['opt_data']


class FeatureBRSController(FBRSController):
    """FBRSController with the back-propagating refinement and the reference controller's own defaults
    (inference/interact/fbrs_controller.py:17-27): brs_mode='f-BRS-B', net_clicks_limit=8, brs_opt_func_params={'min_iou_diff': 1e-3},
    lbfgs_params={'maxfun': 20} merged over m=20, factr=0, pgtol=1e-8 with maxiter = 2 maxfun; optimize_after_n_clicks=1,
    reg_weight=1e-3, reg_bias_weight=10, scale_act=None.  brs_mode 'f-BRS-B', 'f-BRS-C' or 'NoBRS'."""

    def __init__(self, checkpoint_path_or_net, device='cuda:0', max_size=800, brs_mode='f-BRS-B', zoom_in_params=None, with_flip=True,
                 net_clicks_limit=8, prob_thresh=0.5, brs_opt_func_params=None, lbfgs_params=None, optimize_after_n_clicks=1):
        if brs_mode in BRS_MODES and brs_mode not in INSERTION_MODES:
            raise NotImplementedError(f'FeatureBRSController: brs_mode={brs_mode!r} back-propagates through the ASPP or the whole backbone, '
                                      "whose adjoints are not built ('f-BRS-B', 'f-BRS-C' and 'NoBRS' are)")
        if brs_mode != 'NoBRS' and brs_mode not in INSERTION_MODES:
            raise ValueError(f'FeatureBRSController: unknown brs_mode {brs_mode!r}')
        self.brs_mode = brs_mode
        self.brs_opt_func_params = {'min_iou_diff': 1e-3}
        self.brs_opt_func_params.update(brs_opt_func_params or {})
        unknown = set(self.brs_opt_func_params) - {'min_iou_diff', 'reg_weight', 'reg_bias_weight', 'scale_act'}
        if unknown:
            raise ValueError(f'FeatureBRSController: unknown brs_opt_func_params {sorted(unknown)}')
        self.lbfgs_params = {'maxfun': 20}
        self.lbfgs_params.update(lbfgs_params or {})
        self.optimize_after_n_clicks = optimize_after_n_clicks
        if brs_mode != 'NoBRS':
            _fmin_l_bfgs_b()                # fail at construction, not at the second click
        self._setup(checkpoint_path_or_net, device, max_size, zoom_in_params, with_flip, net_clicks_limit, prob_thresh)

    def _reset_predictor(self):
        if self.brs_mode == 'NoBRS':
            return super()._reset_predictor()
        self.predictor = FeatureBRSPredictor(self.net, INSERTION_MODES[self.brs_mode], self.net_clicks_limit, self.with_flip,
                                             ZoomIn(prob_thresh=self.prob_thresh, **self.zoom_in_params), self.max_size,
                                             optimize_after_n_clicks=self.optimize_after_n_clicks, prob_thresh=self.prob_thresh,
                                             lbfgs=self.lbfgs_params, **self.brs_opt_func_params)
        if self.image is not None:
            self.predictor.set_input_image(self.image)
