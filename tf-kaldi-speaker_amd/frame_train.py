"""Train the 1-tap frame layers behind the last multi-tap convolution together with the segment-level layers and the head: the
next part of stage two of every fine-tune (egs/voxceleb/v1/nnet/lib/finetune.py:6-7: "... and then update the entire network"),
as the reference's `noupdate_var_list` does it when only the multi-tap layers are named as fixed (model/trainer.py:309-320,
501-527).

The frozen forward stops at `tdnn3_relu` (`tdnn7_relu` for the extended TDNN), a public frame-level node that
Trainer.predict_packed returns as packed rows [total_out_frames, C] on the device.  Behind it tdnn4 and tdnn5 (tdnn8, tdnn9,
tdnn10) have kernel width 1: on packed frames they are dense + batch norm + activation with one row per frame, which is what
xv_seg_forward / xv_seg_backward compute (tail_train.SegLayer).  The one new mathematical piece is statistics pooling on the
CURRENT activations and its gradient (csrc/pool_grad.hip; model/pooling.py:27-52):
    m = mean_t x_t,  v = mean_t (x_t - m)^2,  std = sqrt(max(v, 1e-12)),  pooled = [m | std];
    gx_t = gm / n + [v > 1e-12] gs (x_t - m) / (n std)
(the floor mask is a constant to TensorFlow; the term of d v / d m multiplies sum_t (x_t - m) = 0).

A step is: SegLayer.forward per frame layer on the packed rows, StatPool.forward, the two segment layers, one
xv_loss_classifier_grad, the segment layers backward (now with gx for the first), StatPool.backward, the frame layers backward
(no gx for the first), one xv_opt_step per tensor.  Trained: every dense kernel and bias, gamma and beta of every batch norm
behind the frozen node, the head.  NOT trained: the moving statistics.  Batch norm runs in INFERENCE mode and the pooling floor
mask is a constant: **parity unpinned**, as for tail_train.py.  batch_norm="batch" switches the layers trained here to the
statistics of the batch and moving-average updates, as tail_train.py describes; the frozen forward stays as it is.

`weight_l2_regularizer` goes on every dense kernel, the frame layers' included (model/tdnn.py: every layer takes
kernel_regularizer); the head keeps the rule of head_train.optimizer_config, the clip is per tensor, Adam's step count is shared.
frame_variables, frozen_node, trained_names, l2_assignment and check_supported are pure host code; the rest needs a HIP device.

StackedTrainer is "frame layers -> StatPool -> TailTrainer" for any kind of frame layer: it builds and checks the chain, and its
step is tail_train.TailTrainer._step.  FrameTrainer here and conv_train.ConvTrainer say only what their frame layers are;
stacked_names and stacked_l2 give both modules their trained_names and l2_assignment."""

import numpy as np

from . import _lib
from ._lib import ptr
from . import head_train
from . import losses
from . import tail_train

StepResult = head_train.StepResult
SegSpec = tail_train.SegSpec

# network_type -> (variable scope, the trailing 1-tap frame layers, the frame layer whose activation is the frozen node)
_FRAME = {"tdnn": ("tdnn", (4, 5), 3), "extended_tdnn": ("etdnn", (8, 9, 10), 7)}


def _dict(params):
    return params if isinstance(params, dict) else params.dict


def check_supported(params, metric=False):
    """NotImplementedError for what the frame-level stage does not cover: ResNet-18 (its dense1 / dense2 follow 2-D
    convolutions), any pooling other than statistics pooling, then everything tail_train.check_supported refuses (metric: its
    second door)."""
    d = _dict(params)
    if d.get("network_type", "tdnn") == "resnet_18":
        raise NotImplementedError("resnet_18: no 1-tap frame layers lie between its convolutions and the pooling node")
    if d.get("pooling_type", "statistics_pooling") != "statistics_pooling":
        raise NotImplementedError("pooling_type %s: only the gradient of statistics_pooling is implemented" % d.get("pooling_type"))
    tail_train.check_supported(params, metric)
    if d.get("network_type", "tdnn") not in _FRAME:
        raise NotImplementedError("Not implement %s network" % d.get("network_type"))


def frame_variables(params):
    """-> the SegSpecs of the trailing 1-tap frame layers, in forward order, under the scope names csrc/api_graph.hip uses:
    tdnn4, tdnn5 for the TDNN and tdnn8, tdnn9, tdnn10 for the extended TDNN.  Each has a batch norm and the activation."""
    d = _dict(params)
    scope, layers, _ = _FRAME[d.get("network_type", "tdnn")]
    act = _lib.XV_SEG_ACT_LRELU if d.get("network_relu_type") == "lrelu" else _lib.XV_SEG_ACT_RELU
    return tuple(SegSpec("%s/tdnn%d_dense/kernel" % (scope, i), "%s/tdnn%d_dense/bias" % (scope, i), "%s/tdnn%d_bn" % (scope, i), act)
                 for i in layers)


def frozen_node(params):
    """The frame-level endpoint the frozen forward stops at: the input of the first trained frame layer."""
    return "tdnn%d_relu" % _FRAME[_dict(params).get("network_type", "tdnn")][2]


def stacked_names(frame_specs, params, metric=False):
    """The TensorFlow names of every variable a StackedTrainer with these frame layers updates: the frame layers first, then
    tail_train.trained_names."""
    out = []
    for spec in frame_specs:
        out += [spec.kernel] + ([spec.bias] if spec.bias else []) + [spec.bn + "/gamma", spec.bn + "/beta"]
    return out + tail_train._trained_names(params, metric)


def stacked_l2(frame_specs, params, metric=False):
    """name -> the l2 factor of its update: weight_l2_regularizer on every kernel, the frame layers' included, optimizer_config's
    rule on the head's kernel, 0 on every bias, gamma and beta."""
    reg = float(_dict(params).get("weight_l2_regularizer", 0.0))
    out = dict.fromkeys(stacked_names(frame_specs, params, metric), 0.0)
    out.update(tail_train._l2_assignment(params, metric))
    for spec in frame_specs:
        out[spec.kernel] = reg
    return out


def trained_names(params):
    """The TensorFlow names of every variable FrameTrainer updates (stacked_names of frame_variables)."""
    return stacked_names(frame_variables(params), params)


def l2_assignment(params):
    """name -> the l2 factor of its update (stacked_l2 of frame_variables)."""
    return stacked_l2(frame_variables(params), params)


def metric_trained_names(params):
    """trained_names behind the metric door (tail_train.metric_trained_names): no head layer."""
    return stacked_names(frame_variables(params), params, True)


def metric_l2_assignment(params):
    return stacked_l2(frame_variables(params), params, True)


class StatPool(object):
    """Statistics pooling of packed rows with its gradient (xv_stat_pool_forward / xv_stat_pool_backward): forward() keeps x,
    pooled and the variance before the floor for backward()."""

    def __init__(self, channels, device=0):
        self.channels, self.device = int(channels), int(device)
        self._torch, self._lib = losses._need_device(), _lib.load()
        self._x = self._offsets = self._pooled = self._var = None
        self._batch = self._rows = 0
        self._covers = False

    def forward(self, x_dev, offsets):
        """x_dev [rows, C] on the device, float32 contiguous; offsets [B + 1] (host integers or an int32 device tensor) ->
        pooled [B, 2 C] = [mean | std] on the device."""
        torch = self._torch
        c = self.channels
        if x_dev.dim() != 2 or int(x_dev.shape[1]) != c or x_dev.dtype != torch.float32 or not x_dev.is_contiguous():
            raise ValueError("x: expected a contiguous float32 [rows, %d], got %s" % (c, tuple(x_dev.shape)))
        rows = int(x_dev.shape[0])
        with torch.cuda.device(self.device):
            if torch.is_tensor(offsets):
                off = offsets.to(device=x_dev.device, dtype=torch.int32).contiguous()
                covers = False                                   # not known without a copy to the host
            else:
                host = np.ascontiguousarray(offsets, dtype=np.int64)
                if host.ndim != 1 or host.size < 1 or host[0] < 0 or np.any(np.diff(host) < 0) or host[-1] > rows:
                    raise ValueError("offsets must ascend from >= 0 to at most the %d rows of x" % rows)
                off = torch.from_numpy(host.astype(np.int32)).to(x_dev.device)
                covers = host.size > 1 and int(host[0]) == 0 and int(host[-1]) == rows
            batch = int(off.numel()) - 1
            pooled = torch.empty((max(batch, 1), 2 * c), dtype=torch.float32, device=x_dev.device)
            var = torch.empty((max(batch, 1), c), dtype=torch.float32, device=x_dev.device)
            stream = _lib.stream(self.device)
            _lib.check(self._lib.xv_stat_pool_forward(self.device, ptr(x_dev), c, c, ptr(off), batch, rows, ptr(pooled), 2 * c, ptr(var), c,
                                                      stream))
        self._x, self._offsets, self._pooled, self._var, self._batch, self._rows = x_dev, off, pooled, var, batch, rows
        self._covers = covers
        return pooled[:batch]

    def backward(self, g_pooled):
        """g_pooled [B, 2 C] on the device -> gx [rows, C]; rows no utterance owns come back as zeros."""
        torch = self._torch
        c = self.channels
        if self._x is None:
            raise RuntimeError("StatPool.backward needs a forward first")
        if tuple(g_pooled.shape) != (self._batch, 2 * c) or not g_pooled.is_contiguous():
            raise ValueError("g_pooled: expected a contiguous [%d, %d], got %s" % (self._batch, 2 * c, tuple(g_pooled.shape)))
        with torch.cuda.device(self.device):
            make = torch.empty if self._covers else torch.zeros           # every row has an owner: every element is written
            gx = make((self._rows, c), dtype=torch.float32, device=self._x.device)
            stream = _lib.stream(self.device)
            _lib.check(self._lib.xv_stat_pool_backward(self.device, ptr(g_pooled), 2 * c, ptr(self._x), c, c, ptr(self._offsets), self._batch,
                                                       self._rows, ptr(self._pooled), 2 * c, ptr(self._var), c, ptr(gx), c,
                                                       stream))
        return gx


class StackedTrainer(object):
    """Frame layers -> StatPool -> a tail_train.TailTrainer (the two segment-level layers and the head), all built from the
    checkpoint's variables, and THE step through them (TailTrainer._step).  A subclass says what its frame layers are: its
    module's three functions, _layer, _width, _walk, and its own words in _CHAIN and _INPUT.

    batch_norm="moving" (the default) or "batch", as tail_train.TailTrainer takes it and for every layer this trainer trains
    (what lies in front of a FrameTrainer, the frozen forward, is not touched): tail_train.batch_stats_options gives each frame
    layer its momentum and, by the rank of its own kernel, bessel.  forward() is the inference path in both modes."""

    _check = _specs = _l2 = None        # the module's check_supported, frame_variables and l2_assignment, as staticmethods
    _metric_l2 = None                   # its metric_l2_assignment
    _CHAIN = None       # "%s ... %d ..., %s ... %d": a layer's kernel and input width, the layer before and its output width
    _INPUT = None       # (the argument's name in the messages, what follows "must be a device tensor")

    def __init__(self, params, weights, num_classes, device=0, seed=0, kernel=None, bias=None, batch_norm="moving", metric=False):
        self._check(params, metric)
        self.params = params
        self.batch_norm = batch_norm
        self.metric = bool(metric)                       # tail_train.check_supported: the door of the two triplet losses
        self.frame_specs = self._specs(params)
        self.tail = tail_train.TailTrainer(params, weights, num_classes, device, seed, kernel, bias, batch_norm, metric)
        num_slots = len(self.tail.layers[0].slots["kernel"])
        self.frame_layers = [self._layer(spec, *tail_train.layer_weights(spec, weights), device, num_slots) for spec in self.frame_specs]
        self._check_chain()
        self.in_dim, self.channels = self._width(self.frame_layers[0]), self.frame_layers[-1].out_dim
        self.device = int(device)
        self.pool = self._make_pool(weights, num_slots)
        self.specs = self.frame_specs + tuple(self.tail.specs)
        self.layers = self.frame_layers + list(self.tail.layers)
        self.head = self.tail.head
        self.embed_dim = self.tail.embed_dim
        self.l2 = self._metric_l2(params) if metric else self._l2(params)
        self._torch = losses._need_device()
        self.tail._fit_workspace(self.layers)
        self.num_steps = 0                                                   # adam's t, shared by every tensor

    def _check_chain(self):
        """Every frame layer takes the columns the layer in front of it gives (a trainer whose layers are no chain says how)."""
        for a, b, sa, sb in zip(self.frame_layers[:-1], self.frame_layers[1:], self.frame_specs[:-1], self.frame_specs[1:]):
            if self._width(b) != a.out_dim:
                raise ValueError(self._CHAIN % (sb.kernel, self._width(b), sa.kernel, a.out_dim))

    def _make_pool(self, weights, num_slots):
        """The pooling stage between the frame layers and the tail, checked against the tail's input width: statistics pooling
        here; att_train's trainers put the key and value networks and the attentive pooling in its place."""
        if self.tail.pool_dim != 2 * self.channels:
            raise ValueError("%s has %d rows, statistics pooling of %d channels gives %d" % (self.tail.specs[0].kernel, self.tail.pool_dim,
                                                                                             self.channels, 2 * self.channels))
        return StatPool(self.channels, self.device)

    def _layer(self, spec, kernel, bias, bn, device, num_slots):
        """The frame layer of `spec` from the checkpoint's kernel, bias and batch-norm vectors (with self._stats(kernel))."""
        raise NotImplementedError

    def _stats(self, kernel):
        """The batch-statistics keywords of the layer with this TensorFlow kernel."""
        return tail_train.batch_stats_options(self.params, self.batch_norm, kernel)

    def _width(self, layer):
        """The columns a row of the layer's input has."""
        raise NotImplementedError

    def _offsets(self, offsets):
        """The offsets as _walk takes them, checked as far as the subclass checks them."""
        return offsets

    def _walk(self, x, offsets, mark, training=True, keep=None):
        """x through every frame layer, mark("frame_forward/<i>") behind layer i -> (the last layer's rows, their offsets).
        keep, a dict if given, receives (rows, offsets) of layer i's output under i: the endpoints an attention reads."""
        raise NotImplementedError

    def tensors(self):
        """[(TensorFlow name, parameter, gradient, slots)] of everything trained, in the order of trained_names()."""
        return tail_train.layer_tensors(self.frame_specs, self.frame_layers) + self.tail.tensors()

    def _packed(self, x_dev):
        torch = self._torch
        name, why = self._INPUT
        if not torch.is_tensor(x_dev) or not x_dev.is_cuda:
            raise ValueError("%s must be a device tensor%s" % (name, why))
        if x_dev.dim() != 2 or int(x_dev.shape[1]) != self.in_dim or x_dev.dtype != torch.float32:
            raise ValueError("%s: expected float32 [rows, %d], got %s" % (name, self.in_dim, tuple(x_dev.shape)))
        return x_dev.contiguous()

    def _forward(self, x_dev, offsets, mark=tail_train._no_mark, training=True):
        x, offsets = self._packed(x_dev), self._offsets(offsets)
        mark("start")
        x, offsets = self._walk(x, offsets, mark, training)
        mark("frame_forward")
        pooled = self.pool.forward(x.contiguous(), offsets)
        mark("pool_forward")
        y = self.tail._forward(pooled.contiguous(), training)
        mark("segment_forward")
        return y

    def _backward(self, gy, mark):
        g = self.tail._backward(gy, True)
        mark("segment_backward")
        g = self.pool.backward(g)
        mark("pool_backward")
        for i in range(len(self.frame_layers) - 1, -1, -1):
            g = self.frame_layers[i].backward(g, i > 0)
            mark("frame_backward/%d" % i)
        mark("frame_backward")

    def forward(self, x_dev, offsets):
        """x_dev [rows, in_dim] on the device (packed rows), offsets [B + 1] of its rows -> the `output` endpoint [B, embed_dim]
        on the device, with the current weights and, in every batch_norm mode, the current moving statistics (inference)."""
        with self._torch.cuda.device(self.device):
            return self._forward(x_dev, offsets, training=False)

    def step(self, x_dev, offsets, labels, learning_rate, global_step=0, mark=None):
        """One training step on a batch of packed rows: forward through the frame layers, the pooling and the segment layers,
        the head's mean loss at `global_step` and its gradients, backward through all of them, then per tensor l2 (kernels only),
        the clip and the update -> StepResult(mean loss, top-1 accuracy), both of the parameters BEFORE the update.

        mark(stage), if given, is called once in front of the first frame layer ("start", the arguments are checked by then) and
        once behind every stage as soon as its calls are queued, in this order (n frame layers): start, frame_forward/0 ..
        frame_forward/n-1, frame_forward, pool_forward, segment_forward, head, segment_backward, pool_backward,
        frame_backward/n-1 .. frame_backward/0, frame_backward, optimizer.  The loss is read back after the last mark."""
        return self.tail._step(self, lambda mark: self._forward(x_dev, offsets, mark), self._backward, labels, learning_rate,
                               global_step, mark)

    def optimizer_state(self):
        """tail_train.optimizer_state of everything this trainer trains: the slots of every tensor and Adam's shared count."""
        return tail_train.optimizer_state(self)

    def load_optimizer_state(self, state):
        tail_train.load_optimizer_state(self, state)

    def variables(self):
        """name -> float32 numpy of every trained variable under its TensorFlow name (layer.kernel() gives the kernels)."""
        out = tail_train.layer_variables(self.frame_specs, self.frame_layers)
        out.update(self.tail.variables())
        return out


class FrameTrainer(StackedTrainer):
    """The trailing 1-tap frame layers on the frozen node's packed rows: dense layers (tail_train.SegLayer), the offsets pass
    through.  forward(frames_dev, offsets), step(frames_dev, offsets, labels, learning_rate, global_step=0, mark=None)."""

    _check, _specs, _l2 = staticmethod(check_supported), staticmethod(frame_variables), staticmethod(l2_assignment)
    _metric_l2 = staticmethod(metric_l2_assignment)
    _CHAIN = "%s has %d rows, %s %d columns"
    _INPUT = ("frames_dev", ": the frames never leave the device")

    def _layer(self, spec, kernel, bias, bn, device, num_slots):
        k = np.asarray(kernel, dtype=np.float32)
        if k.ndim != 2:
            raise ValueError("%s: a dense kernel [cin, cout] expected, got shape %s" % (spec.kernel, k.shape))
        return tail_train.SegLayer(k, bias, bn, spec.act, device, num_slots, **self._stats(k))

    def _width(self, layer):
        return layer.in_dim

    def _walk(self, x, offsets, mark, training=True, keep=None):
        for i, layer in enumerate(self.frame_layers):
            x = tail_train.layer_forward(layer, training, x)
            if keep is not None:
                keep[i] = (x, offsets)
            mark("frame_forward/%d" % i)
        return x, offsets
