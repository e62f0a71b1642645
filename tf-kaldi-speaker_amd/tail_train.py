"""Train the two segment-level layers together with the classifier head: the first part of stage two of every fine-tune
(egs/voxceleb/v1/nnet/lib/finetune.py:6-7: "... and then update the entire network"), as the reference's `noupdate_var_list`
does it when the frame-level layers are named as fixed (model/trainer.py:309-320, 501-527).

Everything up to the `pooling` node stays as the checkpoint has it, so no frame-level backward pass is needed (frame_train.py
goes on from here: the 1-tap frame layers in front of the pooling node, through the gradient of statistics pooling).  A step is: the
frozen forward to `pooling` (Trainer.predict, by the caller), xv_seg_forward through tdnn6 and tdnn7 (tdnn12 / tdnn13 for the
extended TDNN) with their CURRENT weights, one xv_loss_classifier_grad for the loss and grad_x, xv_seg_backward through both
layers (csrc/seg_grad.hip), one xv_opt_step per tensor.  Trained: the two dense kernels and biases, gamma and beta of their
batch norms, the head.  NOT trained: the moving statistics.  Batch norm runs in INFERENCE mode (the reference feeds
is_training=True and normalises with batch statistics): the layers are trained on exactly the function extraction and
validation evaluate, as head_train.py does: **parity unpinned**.  That is the default, batch_norm="moving".  With
batch_norm="batch" the trained layers take the reference's mode (Layer's batch_stats: the statistics of the batch, the gradient
through them, moving-average updates by xv_bn_batch_forward / xv_bn_batch_backward, csrc/bn_batch.hip; batch_stats_options says
which layer takes which momentum and variance), pinned to torch instead of TensorFlow.

`weight_l2_regularizer` goes on the two dense kernels only (tf.layers.dense(kernel_regularizer=...), model/tdnn.py:137-160),
the head keeps the rule of head_train.optimizer_config, the clip is per tensor (model/trainer.py:529-533), Adam's step count
is shared.  segment_variables, check_supported and l2_assignment are pure host code; the rest needs a HIP device.

What the trainers stacked in front of this one (frame_train.py, conv_train.py) share lives here, once: Layer, the device state
of one trained layer (SegLayer and conv_train.TConvLayer add their operator); layer_weights, layer_tensors and layer_variables
between the checkpoint's names and the layers; and TailTrainer._step, the step behind the forward (the head's loss and
gradient, the backward, Adam's shared count, one update per tensor, the StepResult), with its optional `mark` callback."""
import collections

import numpy as np

from . import _lib
from ._lib import ptr
from . import head_train
from . import losses
from . import metric_losses
from . import model_io

StepResult = head_train.StepResult
SegSpec = collections.namedtuple("SegSpec", "kernel bias bn act")       # variable names (bn: the scope or None), XV_SEG_ACT_*

_SCOPES = {"tdnn": ("tdnn", 6, 7), "extended_tdnn": ("etdnn", 12, 13), "resnet_18": ("resnet_18", 6, 7)}
_BN = ("gamma", "beta", "moving_mean", "moving_variance")


def _dict(params):
    return params if isinstance(params, dict) else params.dict


METRIC_LOSSES = ("semihard_triplet_loss", "angular_triplet_loss")       # valid.METRIC_LOSSES: what the second door takes


def check_supported(params, metric=False):
    """NotImplementedError for what the segment-level backward pass does not cover, then for everything HeadTrainer refuses.
    metric=True is the second door, as valid.metric_valid is for validation: it takes `semihard_triplet_loss` and
    `angular_triplet_loss` (metric_losses.MetricHead, no classifier layer) and refuses every other loss."""
    d = _dict(params)
    if d.get("network_relu_type") == "prelu":
        raise NotImplementedError("network_relu_type prelu: the trainable alpha of the segment layers is not implemented")
    if d.get("feature_norm"):
        raise NotImplementedError("feature_norm: the gradient of the l2 scaling behind the last layer is not implemented")
    if d.get("network_type", "tdnn") not in _SCOPES:
        raise NotImplementedError("Not implement %s network" % d.get("network_type"))
    if metric:
        if d.get("loss_func") not in METRIC_LOSSES:
            raise NotImplementedError("loss_func %r: the metric door trains %s" % (d.get("loss_func"), " and ".join(METRIC_LOSSES)))
        if d.get("aux_loss_func"):
            raise NotImplementedError("aux_loss_func %r: auxiliary losses are not implemented" % (d["aux_loss_func"],))
        metric_losses.from_params(params, validation=False)       # loss_type, triplet_type, asoftmax m
    else:
        losses.head_config(params, 0, False)
    if d.get("sample_with_prob"):
        raise NotImplementedError("sample_with_prob is not implemented")
    head_train.optimizer_config(params)


def segment_variables(params):
    """-> (SegSpec of the first layer, SegSpec of the second) under the scope names csrc/api_graph.hip uses."""
    d = _dict(params)
    scope, a, b = _SCOPES[d.get("network_type", "tdnn")]
    act = _lib.XV_SEG_ACT_LRELU if d.get("network_relu_type") == "lrelu" else _lib.XV_SEG_ACT_RELU
    name = lambda i, what: "%s/tdnn%d_%s" % (scope, i, what)                # noqa: E731
    first = SegSpec(name(a, "dense/kernel"), name(a, "dense/bias"), name(a, "bn"), act)
    second = SegSpec(name(b, "dense/kernel"), name(b, "dense/bias"), None if d.get("last_layer_no_bn") else name(b, "bn"),
                     _lib.XV_SEG_ACT_NONE if d.get("last_layer_linear") else act)
    return first, second


def trained_names(params):
    """The TensorFlow names of every variable TailTrainer updates, the head's last."""
    return _trained_names(params, False)


def metric_trained_names(params):
    """trained_names behind the metric door: there is no head layer."""
    return _trained_names(params, True)


def _trained_names(params, metric):
    out = []
    for spec in segment_variables(params):
        out += [spec.kernel, spec.bias]
        if spec.bn:
            out += [spec.bn + "/gamma", spec.bn + "/beta"]
    if metric:
        return out
    out.append(model_io.SOFTMAX_KERNEL)
    if _dict(params).get("loss_func") == "softmax":
        out.append(model_io.SOFTMAX_BIAS)
    return out


def l2_assignment(params):
    """name -> the l2 factor of its update: weight_l2_regularizer on the two dense kernels, optimizer_config's rule on the
    head's kernel, 0 on every bias, gamma and beta."""
    return _l2_assignment(params, False)


def metric_l2_assignment(params):
    """l2_assignment behind the metric door: the names of metric_trained_names."""
    return _l2_assignment(params, True)


def _l2_assignment(params, metric):
    d = _dict(params)
    reg = float(d.get("weight_l2_regularizer", 0.0))
    out = dict.fromkeys(_trained_names(params, metric), 0.0)
    for spec in segment_variables(params):
        out[spec.kernel] = reg
    if not metric:
        out[model_io.SOFTMAX_KERNEL] = head_train.optimizer_config(params)[3]
    return out


BATCH_NORM_MODES = ("moving", "batch")


def batch_stats_options(params, batch_norm, kernel=None):
    """The keywords a trained Layer takes for the trainers' batch_norm mode.  "moving" (the default of every trainer): none,
    today's inference-mode batch norm with constant moving statistics.  "batch": batch_stats, momentum =
    params.batchnorm_momentum (0.99 when absent, as every nnet_conf of the reference sets it) and bessel, by the rank of the
    tensor the layer's batch norm sees in model/tdnn.py: tf.layers.batch_normalization takes the fused kernel for a rank-4
    input only, and the fused kernel moves moving_variance towards the Bessel-corrected batch variance.
      * rank-4 convolution kernels ([1, W, C, N]: tf.layers.conv2d of `tdnn`, model/tdnn.py:38-91): the input is [b, 1, l, N],
        bessel is true;
      * that network's 1-tap dense frame layers tdnn4 and tdnn5: model/tdnn.py:94 squeezes the tensor to [b, l, 512] BEFORE
        tdnn4_dense, so their batch norms see rank 3 and bessel is false (the rank of the layer's OWN kernel decides, not the
        network's);
      * rank-3 kernels (tf.layers.conv1d of the extended TDNN, model/tdnn.py:371-539, whose expand_dims is commented out) and all
        its dense layers: rank 3, false;
      * the segment layers behind the pooling: rank 2, false.
    `kernel` is the layer's TensorFlow kernel (None for a segment layer)."""
    if batch_norm not in BATCH_NORM_MODES:
        raise ValueError("batch_norm must be one of %s, got %r" % (", ".join(BATCH_NORM_MODES), batch_norm))
    if batch_norm == "moving":
        return {}
    momentum = _dict(params).get("batchnorm_momentum")
    return dict(batch_stats=True, momentum=0.99 if momentum is None else float(momentum),
                bessel=kernel is not None and np.ndim(kernel) == 4)


class Layer(object):
    """What every trained layer keeps on the device: the rows [N, ldw] of the weights (ldw = the width K rounded up to 4, the
    padding stays zero), the bias, the four batch-norm vectors or None, their gradients, the optimizer slots and a workspace
    that only grows.  SegLayer (dense, xv_seg_*) and conv_train.TConvLayer (packed utterances, xv_tconv_*) add the operator.

    batch_stats (with a batch norm; without one it changes nothing): forward() normalises with the statistics of the batch and
    moves moving_mean and moving_variance (bn[2], bn[3]) in place, backward() goes through the statistics
    (xv_bn_batch_forward / xv_bn_batch_backward, csrc/bn_batch.hip).  The layer's operator then runs without batch norm and
    with XV_SEG_ACT_NONE: forward for z (its y goes to a scratch buffer the layer keeps), backward on gz for gbias, gw and gx.
    momentum and bessel are those of include/xvec_hip.h.  forward(.., training=False) is today's inference path with the
    current moving statistics."""

    def __init__(self, rows, bias, bn, act, device=0, num_slots=0, batch_stats=False, momentum=0.99, bessel=False):
        torch = losses._need_device()
        self.out_dim, self.in_dim = int(rows.shape[0]), int(rows.shape[1])
        self.ldw = (self.in_dim + 3) // 4 * 4
        self.act, self.device = int(act), int(device)
        self.batch_stats, self.momentum, self.bessel = bool(batch_stats) and bn is not None, float(momentum), bool(bessel)
        if self.batch_stats and not 0.0 <= self.momentum <= 1.0:
            raise ValueError("momentum must lie in [0, 1], got %r" % (momentum,))
        self._torch, self._lib = torch, _lib.load()
        dev = "cuda:%d" % self.device
        with torch.cuda.device(self.device):
            self.w = torch.zeros((self.out_dim, self.ldw), dtype=torch.float32, device=dev)
            self.w[:, :self.in_dim] = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(dev)
            self.b = None if bias is None else losses._f32(bias, self.device, torch)     # None: a layer without a bias
            self.bn = None
            if bn is not None:
                if any(tuple(np.shape(v)) != (self.out_dim,) for v in bn):
                    raise ValueError("batch norm: four vectors of %d elements expected" % self.out_dim)
                self.bn = [losses._f32(v, self.device, torch) for v in bn]         # gamma, beta, moving_mean, moving_variance
            self.gw = torch.zeros_like(self.w)                                     # the padding columns stay zero
            self.gb = None if self.b is None else torch.zeros_like(self.b)
            self.ggamma = None if self.bn is None else torch.zeros((self.out_dim,), dtype=torch.float32, device=dev)
            self.gbeta = None if self.bn is None else torch.zeros((self.out_dim,), dtype=torch.float32, device=dev)
            self.slots = {name: [torch.zeros_like(t) for _ in range(num_slots)] for name, t, _ in self.trained()}
        self._x = self._z = self._ws = None
        self._scratch = self._bn_ws = self._mean = self._var = None
        self._batch = False                                                    # the last forward used the batch statistics

    def trained(self):
        """[(name, parameter, gradient)] in the order the optimizer takes them."""
        out = [("kernel", self.w, self.gw)] + ([] if self.b is None else [("bias", self.b, self.gb)])
        if self.bn is not None:
            out += [("gamma", self.bn[0], self.ggamma), ("beta", self.bn[1], self.gbeta)]
        return out

    def _empty_batch(self, rows, width, want_gx):
        """The gradient of an empty sum: zeros in every parameter gradient -> gx [rows, width] of zeros, or None."""
        for _, _, g in self.trained():
            g.zero_()
        return self._torch.zeros((rows, width), dtype=self._torch.float32, device=self._x.device) if want_gx else None

    def _workspace(self, need, device):
        if self._ws is None or self._ws.numel() < need:
            self._ws = self._torch.empty(max(need, 16), dtype=self._torch.uint8, device=device)
        return self._ws

    def _use_batch(self, training, rows):
        """Whether this forward takes the batch statistics; they need a row."""
        self._batch = bool(training) and self.batch_stats
        if self._batch and rows < 1:
            raise ValueError("batch statistics need at least one row")
        return self._batch

    def _scratch_y(self, rows, device):
        """The y the operator writes when it is called for z alone: a buffer that only grows, never read."""
        if self._scratch is None or self._scratch.shape[0] < rows:
            self._scratch = self._torch.empty((rows, self.out_dim), dtype=self._torch.float32, device=device)
        return self._scratch

    def _bn_workspace(self, rows, device):
        need = int(self._lib.xv_bn_batch_workspace(rows, self.out_dim))
        if self._bn_ws is None or self._bn_ws.numel() < need:
            self._bn_ws = self._torch.empty(max(need, 16), dtype=self._torch.uint8, device=device)
        return self._bn_ws

    def _bn_forward(self, z, rows, stream):
        """z [rows, N] (the layer's product, no batch norm, no activation) -> y [rows, N] by the batch statistics, which are kept
        for _bn_backward; moving_mean and moving_variance move in place."""
        torch = self._torch
        y = torch.empty((rows, self.out_dim), dtype=torch.float32, device=z.device)
        self._mean = torch.empty((self.out_dim,), dtype=torch.float32, device=z.device)
        self._var = torch.empty((self.out_dim,), dtype=torch.float32, device=z.device)
        ws = self._bn_workspace(rows, z.device)
        _lib.check(self._lib.xv_bn_batch_forward(self.device, ptr(z), self.out_dim, rows, self.out_dim, ptr(self.bn[0]), ptr(self.bn[1]),
                                                 self.act, self.momentum, int(self.bessel), ptr(self.bn[2]), ptr(self.bn[3]), ptr(y),
                                                 self.out_dim, ptr(self._mean), ptr(self._var), ptr(ws), ws.numel(), stream))
        return y

    def _bn_backward(self, gy, z, rows, stream):
        """gy [rows, N] -> gz [rows, N], the gradient at the layer's product; ggamma and gbeta are written."""
        torch = self._torch
        gz = torch.empty((rows, self.out_dim), dtype=torch.float32, device=z.device)
        ws = self._bn_workspace(rows, z.device)
        _lib.check(self._lib.xv_bn_batch_backward(self.device, ptr(gy), self.out_dim, ptr(z), self.out_dim, rows, self.out_dim,
                                                  ptr(self._mean), ptr(self._var), ptr(self.bn[0]), ptr(self.bn[1]), self.act, ptr(gz),
                                                  self.out_dim, ptr(self.ggamma), ptr(self.gbeta), ptr(ws), ws.numel(),
                                                  stream))
        return gz


class SegLayer(Layer):
    """A dense layer: w holds the transpose of the TensorFlow kernel [K, N]."""

    def __init__(self, kernel, bias, bn, act, device=0, num_slots=0, batch_stats=False, momentum=0.99, bessel=False):
        kernel = np.asarray(kernel, dtype=np.float32)
        if kernel.ndim != 2 or tuple(np.shape(bias)) != (kernel.shape[1],):
            raise ValueError("kernel [K, N] and bias [N] expected, got %s and %s" % (kernel.shape, np.shape(bias)))
        Layer.__init__(self, kernel.T, bias, bn, act, device, num_slots, batch_stats, momentum, bessel)

    def forward(self, x, training=True):
        """x [n, K] on the device, float32 contiguous -> y [n, N]; x and z are kept for backward().  With batch_stats, training
        chooses between the statistics of the batch and the moving ones; without, it changes nothing."""
        torch = self._torch
        n = int(x.shape[0])
        if tuple(x.shape) != (n, self.in_dim):
            raise ValueError("x: expected [n, %d], got shape %s" % (self.in_dim, tuple(x.shape)))
        batch = self._use_batch(training, n)
        with torch.cuda.device(self.device):
            z = torch.empty((max(n, 1), self.out_dim), dtype=torch.float32, device=x.device)
            y = self._scratch_y(n, x.device) if batch else torch.empty((max(n, 1), self.out_dim), dtype=torch.float32, device=x.device)
            bn = [None] * 4 if batch else self.bn or [None] * 4
            stream = _lib.stream(self.device)
            _lib.check(self._lib.xv_seg_forward(self.device, ptr(x), self.in_dim, n, self.in_dim, ptr(self.w), self.ldw, self.out_dim,
                                                ptr(self.b), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]),
                                                _lib.XV_SEG_ACT_NONE if batch else self.act, ptr(z), self.out_dim,
                                                ptr(y), self.out_dim, stream))
            if batch:
                y = self._bn_forward(z, n, stream)
        self._x, self._z = x, z
        return y[:n]

    def backward(self, gy, want_gx):
        """gy [n, N] on the device -> gx [n, K] or None; the gradients of the parameters go to gw, gb, ggamma, gbeta."""
        torch = self._torch
        x, z = self._x, self._z
        n = int(x.shape[0])
        if tuple(gy.shape) != (n, self.out_dim) or not gy.is_contiguous():
            raise ValueError("gy: expected a contiguous [%d, %d], got shape %s" % (n, self.out_dim, tuple(gy.shape)))
        with torch.cuda.device(self.device):
            if n == 0:
                return self._empty_batch(0, self.in_dim, want_gx)
            gx = torch.empty((n, self.in_dim), dtype=torch.float32, device=x.device) if want_gx else None
            ws = self._workspace(int(self._lib.xv_seg_workspace(n, self.in_dim, self.out_dim)), x.device)
            bn = self.bn or [None] * 4
            stream = _lib.stream(self.device)
            if self._batch:                  # through the statistics first; the operator then passes gz through its mask
                gz = self._bn_backward(gy, z, n, stream)
                _lib.check(self._lib.xv_seg_backward(self.device, ptr(gz), self.out_dim, ptr(x), self.in_dim, ptr(z), self.out_dim, n,
                                                     self.in_dim, ptr(self.w), self.ldw, self.out_dim, None, None, None, None,
                                                     _lib.XV_SEG_ACT_NONE, ptr(gx), self.in_dim, ptr(self.gw), ptr(self.gb), None, None,
                                                     ptr(ws), ws.numel(), stream))
                return gx
            _lib.check(self._lib.xv_seg_backward(self.device, ptr(gy), self.out_dim, ptr(x), self.in_dim, ptr(z), self.out_dim, n,
                                                 self.in_dim, ptr(self.w), self.ldw, self.out_dim, ptr(bn[0]), ptr(bn[1]), ptr(bn[2]),
                                                 ptr(bn[3]), self.act, ptr(gx), self.in_dim, ptr(self.gw), ptr(self.gb), ptr(self.ggamma),
                                                 ptr(self.gbeta), ptr(ws), ws.numel(), stream))
        return gx

    def kernel(self):
        """The TensorFlow kernel [K, N], float32 numpy."""
        return np.ascontiguousarray(self.w[:, :self.in_dim].t().cpu().numpy())


def layer_forward(layer, training, *args):
    """layer.forward(*args), the call the trainers have always made; only a layer with batch_stats is ever told training=False
    (the inference path of the trainers' forward())."""
    return layer.forward(*args) if training or not layer.batch_stats else layer.forward(*args, training=False)


def layer_weights(spec, weights):
    """-> (kernel, bias, the four batch-norm vectors or None) of `spec` from the checkpoint; KeyError names what it lacks.
    A spec without a bias (spec.bias None: the ResNet's grid convolutions) gives None in its place."""
    wanted = (spec.kernel,) + ((spec.bias,) if spec.bias else ()) + (tuple(spec.bn + "/" + s for s in _BN) if spec.bn else ())
    missing = [k for k in wanted if k not in weights]
    if missing:
        raise KeyError("the checkpoint lacks %s" % ", ".join(missing))
    return (weights[spec.kernel], weights[spec.bias] if spec.bias else None,
            [weights[spec.bn + "/" + s] for s in _BN] if spec.bn else None)


def layer_tensors(specs, layers):
    """[(TensorFlow name, parameter, gradient, slots)] of the layers, in the order of trained_names()."""
    out = []
    for spec, layer in zip(specs, layers):
        names = {"kernel": spec.kernel, "bias": spec.bias, "gamma": (spec.bn or "") + "/gamma", "beta": (spec.bn or "") + "/beta"}
        out += [(names[k], w, g, layer.slots[k]) for k, w, g in layer.trained()]
    return out


def layer_variables(specs, layers):
    """name -> float32 numpy of the layers' trained variables under their TensorFlow names (layer.kernel() gives the kernel);
    of a layer with batch_stats also the moving statistics its forward passes have moved."""
    out = collections.OrderedDict()
    for spec, layer in zip(specs, layers):
        out[spec.kernel] = layer.kernel()
        if spec.bias:
            out[spec.bias] = layer.b.cpu().numpy().copy()
        if spec.bn:
            for k, name in enumerate(_BN if layer.batch_stats else _BN[:2]):
                out[spec.bn + "/" + name] = layer.bn[k].cpu().numpy().copy()
    return out


def optimizer_state(trainer):
    """What the reference's Saver keeps beside the variables: {"num_steps": Adam's shared count (int64 scalar), "<TensorFlow
    name>/slot<k>": slot k of every tensor of trainer.tensors()} as numpy arrays, the slots in the layout the device holds them
    in (a kernel's rows [N, ldw]).  sgd has no slots, momentum one per tensor, adam two."""
    out = collections.OrderedDict(num_steps=np.array(trainer.num_steps, dtype=np.int64))
    for name, _, _, slots in trainer.tensors():
        for k, slot in enumerate(slots):
            out["%s/slot%d" % (name, k)] = slot.cpu().numpy().copy()
    return out


def load_optimizer_state(trainer, state):
    """Put optimizer_state()'s dict back: every slot of every tensor and the step count.  KeyError names what `state` lacks,
    ValueError a slot of another shape or a name the trainer does not have; nothing is changed then."""
    torch = losses._need_device()
    wanted = {"%s/slot%d" % (name, k): slot for name, _, _, slots in trainer.tensors() for k, slot in enumerate(slots)}
    missing = [k for k in list(wanted) + ["num_steps"] if k not in state]
    if missing:
        raise KeyError("the optimizer state lacks %s" % ", ".join(missing))
    extra = [k for k in state if k not in wanted and k != "num_steps"]
    if extra:
        raise ValueError("the optimizer state holds %s, which this trainer does not train" % ", ".join(extra))
    for k, slot in wanted.items():
        if tuple(np.shape(state[k])) != tuple(slot.shape):
            raise ValueError("%s: expected shape %s, got %s" % (k, tuple(slot.shape), tuple(np.shape(state[k]))))
    for k, slot in wanted.items():
        slot.copy_(torch.from_numpy(np.ascontiguousarray(state[k], dtype=np.float32)))
    steps = int(state["num_steps"])
    for t in (trainer, getattr(trainer, "tail", None), trainer.head):
        if t is not None:
            t.num_steps = steps


def _no_mark(stage):
    pass


class MetricTail(object):
    """What stands in HeadTrainer's place behind the metric door: the optimizer's settings and Adam's count, and
    metric_losses.MetricHead for the loss and its gradient.  It owns no parameter."""

    def __init__(self, params, device=0):
        self.kind, self.momentum, self.nesterov, self.l2, self.clip_norm = head_train.optimizer_config(params)
        self.params, self.loss_func = params, _dict(params).get("loss_func")
        self.head = metric_losses.MetricHead(params, device)
        self.num_steps = 0


class TailTrainer(object):
    """The two segment-level layers, built from the checkpoint's variables, and a head_train.HeadTrainer behind them.

    batch_norm="moving" (the default) is inference-mode batch norm with constant moving statistics; "batch" is the reference's
    training mode (batch_stats_options): step() normalises with the statistics of the batch, differentiates through them and
    moves the moving statistics, which variables() then returns as well; forward() (the `output` endpoint) stays the inference
    path, with the CURRENT moving statistics.  trained_names(), l2_assignment() and tensors() do not change: the moving
    statistics are no optimizer tensors.  **Parity unpinned** against TensorFlow, pinned to torch (include/xvec_hip.h)."""

    def __init__(self, params, weights, num_classes, device=0, seed=0, kernel=None, bias=None, batch_norm="moving", metric=False):
        check_supported(params, metric)
        self.params = params
        self.metric = bool(metric)
        self.batch_norm = batch_norm
        stats = batch_stats_options(params, batch_norm)
        self.specs = segment_variables(params)
        kind = head_train.optimizer_config(params)[0]
        num_slots = {_lib.XV_OPT_SGD: 0, _lib.XV_OPT_MOMENTUM: 1, _lib.XV_OPT_ADAM: 2}[kind]
        self.layers = [SegLayer(*layer_weights(spec, weights), spec.act, device, num_slots, **stats) for spec in self.specs]
        if self.layers[1].in_dim != self.layers[0].out_dim:
            raise ValueError("%s has %d rows, %s %d columns" % (self.specs[1].kernel, self.layers[1].in_dim, self.specs[0].kernel,
                                                                  self.layers[0].out_dim))
        self.pool_dim, self.embed_dim = self.layers[0].in_dim, self.layers[1].out_dim
        # metric=True: no classifier layer is built; num_classes, seed, kernel and bias are not used
        self.head = MetricTail(params, device) if metric else head_train.HeadTrainer(params, self.embed_dim, num_classes, device, seed,
                                                                                     kernel, bias)
        self.l2 = _l2_assignment(params, metric)
        torch = losses._need_device()
        self._torch, self._lib, self.device = torch, _lib.load(), int(device)
        self._ws = None
        self._fit_workspace(self.layers)
        self.num_steps = 0                                                   # adam's t, shared by every tensor

    def _fit_workspace(self, layers):
        """Grow the optimizer's workspace to the largest tensor among `layers` and the head."""
        largest = max([layer.w.numel() for layer in layers] + ([] if self.metric else [self.head.head.raw_rows.numel()]))
        need = max(int(self._lib.xv_opt_workspace(largest)), 8)
        if self._ws is None or self._ws.numel() < need:
            with self._torch.cuda.device(self.device):
                self._ws = self._torch.empty(need, dtype=self._torch.uint8, device=layers[0].w.device)

    def tensors(self):
        """[(TensorFlow name, parameter, gradient, slots)] of everything trained, in the order of trained_names()."""
        out = layer_tensors(self.specs, self.layers)
        if self.metric:
            return out
        h = self.head
        out.append((model_io.SOFTMAX_KERNEL, h.head.raw_rows, h._grad_rows, h._row_slots))
        if h.head.bias is not None:
            out.append((model_io.SOFTMAX_BIAS, h.head.bias, h._grad_bias, h._bias_slots))
        return out

    def forward(self, pooled):
        """pooled [n, pool_dim] -> the `output` endpoint [n, embed_dim] on the device, with the current weights and, in every
        batch_norm mode, the current moving statistics (inference)."""
        torch = self._torch
        with torch.cuda.device(self.device):
            return self._forward(losses._f32(pooled, self.device, torch), False)

    def _forward(self, x, training=True):
        return layer_forward(self.layers[1], training, layer_forward(self.layers[0], training, x))

    def _backward(self, gy, want_gx):
        return self.layers[0].backward(self.layers[1].backward(gy, True), want_gx)

    def _apply(self, w, g, slots, lr, l2):
        h = self.head
        stream = _lib.stream(self.device)
        _lib.check(self._lib.xv_opt_step(self.device, h.kind, int(h.nesterov), ptr(w), ptr(g), ptr(slots[0]) if slots else None,
                                         ptr(slots[1]) if len(slots) > 1 else None, w.numel(), float(lr), l2, h.clip_norm, h.momentum,
                                         self.num_steps, ptr(self._ws), self._ws.numel(), stream))

    def _step(self, owner, forward, backward, labels, learning_rate, global_step, mark):
        """THE training step, of this trainer (owner is self) and of every trainer stacked in front of it (frame_train.Stacked):
        y = forward(mark), the head's mean loss at `global_step` and its gradients, backward(grad_y, mark), then Adam's shared
        step count and per tensor of owner.tensors() l2, the clip and the update -> StepResult(mean loss, top-1 accuracy), both
        of the parameters BEFORE the update.  mark(stage) is called behind the head ("head") and the updates ("optimizer"), and
        by forward and backward behind their own stages; the loss is read back after the last mark."""
        torch = self._torch
        h = self.head
        mark = mark or _no_mark
        with torch.cuda.device(self.device):
            y = forward(mark)
            if self.metric:        # one group = the batch, grad_scale 1; the group loss, no accuracy
                res = h.head.loss_and_grad(y, labels, as_tensor=True, sync=False)
                gx = res.grad_x
            else:
                out, top1, gx, _, _ = h.head._grad_device(y, labels, global_step, None, True, h._grad_rows, h._grad_bias)
                n = int(out.shape[1])
            mark("head")
            backward(gx, mark)
            owner.num_steps += 1
            self.num_steps = h.num_steps = owner.num_steps
            for name, w, g, slots in owner.tensors():
                self._apply(w, g, slots, learning_rate, owner.l2[name])
            mark("optimizer")
            if self.metric:
                return StepResult(float(res.group_loss[0]), float("nan"))
            lab = losses._labels_dev(labels, n, out.device, torch)
            return StepResult(float(out[0].double().mean()) if n else float("nan"),
                              float((top1 == lab).double().mean()) if n else float("nan"))

    def step(self, pooled, labels, learning_rate, global_step=0, mark=None):
        """One training step on a batch of pooled rows [n, pool_dim]: forward through both layers, then _step.  mark(stage), if
        given, is called in front of the first layer ("start", the rows are on the device by then), then behind
        "segment_forward", "head", "segment_backward" and "optimizer", in this order."""
        def forward(mark):
            x = losses._f32(pooled, self.device, self._torch)
            mark("start")
            y = self._forward(x)
            mark("segment_forward")
            return y

        def backward(gx, mark):
            self._backward(gx, False)
            mark("segment_backward")
        return self._step(self, forward, backward, labels, learning_rate, global_step, mark)

    def optimizer_state(self):
        """tail_train.optimizer_state of this trainer."""
        return optimizer_state(self)

    def load_optimizer_state(self, state):
        load_optimizer_state(self, state)

    def variables(self):
        """name -> float32 numpy of every trained variable under its TensorFlow name (kernels as [in, out])."""
        out = layer_variables(self.specs, self.layers)
        if self.metric:
            return out
        out[model_io.SOFTMAX_KERNEL] = self.head.kernel()
        if self.head.bias() is not None:
            out[model_io.SOFTMAX_BIAS] = self.head.bias()
        return out
