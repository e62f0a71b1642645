"""Train EVERY frame-level layer, the multi-tap convolutions included, together with the statistics pooling, the segment-level
layers and the head: the last part of stage two of every fine-tune (egs/voxceleb/v1/nnet/lib/finetune.py:6-7: "... and then
update the entire network") for the TDNN and the extended TDNN.

There is no frozen forward any more: the packed features [total_frames, dim] go straight in, and every frame-level layer runs
through xv_tconv_forward / xv_tconv_backward (csrc/tconv_grad.hip) with its CURRENT weights, in exact fp32 whatever precision
the extraction uses.  A layer is tf.layers.conv2d(.., (1, W)) / tf.layers.conv1d(.., W) (VALID, stride 1: model/tdnn.py), or a
dense layer, which is the same operator with W = 1; then batch norm, then the activation.  An utterance of n frames leaves a
W-tap layer with n - (W - 1) frames; out_offsets() keeps the packed offsets.
    TDNN:           conv 5, conv 5, conv 7, dense 4, 5                                          (context 14)
    extended TDNN:  conv 5, dense, conv 5, dense, conv 7, dense, conv 9, dense 8, 9, 10         (context 22)
Behind them frame_train.StatPool and an unchanged tail_train.TailTrainer.  A step is: the frame layers forward, StatPool.forward,
the two segment layers, one xv_loss_classifier_grad, the segment layers backward, StatPool.backward, the frame layers backward
in reverse (no gx for the first), one xv_opt_step per tensor.  Trained: every kernel (the convolutions' in the shape the
checkpoint had, rank 4 or 3) and bias, gamma and beta of every batch norm, the head.  NOT trained: the moving statistics.
Batch norm runs in INFERENCE mode and the pooling floor mask is a constant: **parity unpinned**, as for tail_train.py.

`weight_l2_regularizer` goes on every kernel, the convolutions' included (model/tdnn.py: every layer takes kernel_regularizer);
the head keeps the rule of head_train.optimizer_config, the clip is per tensor, Adam's step count is shared.
frame_variables, trained_names, l2_assignment, check_supported, out_offsets, kernel_to_rows and rows_to_kernel are pure host
code; the rest needs a HIP device."""
import collections
import ctypes as C

import numpy as np

from . import _lib
from . import frame_train
from . import head_train
from . import losses
from . import tail_train

StepResult = head_train.StepResult
ConvSpec = collections.namedtuple("ConvSpec", "kernel bias bn act taps")      # variable names, XV_SEG_ACT_*, kernel width

# network_type -> (variable scope, the kernel widths of the frame-level layers in forward order)
_NETS = {"tdnn": ("tdnn", (5, 5, 7, 1, 1)), "extended_tdnn": ("etdnn", (5, 1, 5, 1, 7, 1, 9, 1, 1, 1))}
_BN = tail_train._BN
_p = tail_train._p


def _dict(params):
    return params if isinstance(params, dict) else params.dict


def check_supported(params):
    """NotImplementedError for everything frame_train.check_supported refuses: ResNet-18, any pooling other than statistics
    pooling, PReLU, feature_norm, the heads and optimizers HeadTrainer refuses."""
    frame_train.check_supported(params)


def frame_variables(params):
    """-> the ConvSpecs of every frame-level layer, in forward order, under the scope names csrc/api_graph.hip uses: a layer
    of more than one tap is tdnn<i>_conv, a 1-tap layer tdnn<i>_dense.  Each has a batch norm and the activation."""
    d = _dict(params)
    scope, widths = _NETS[d.get("network_type", "tdnn")]
    act = _lib.XV_SEG_ACT_LRELU if d.get("network_relu_type") == "lrelu" else _lib.XV_SEG_ACT_RELU
    return tuple(ConvSpec("%s/tdnn%d_%s/kernel" % (scope, i, "conv" if w > 1 else "dense"),
                          "%s/tdnn%d_%s/bias" % (scope, i, "conv" if w > 1 else "dense"), "%s/tdnn%d_bn" % (scope, i), act, w)
                 for i, w in enumerate(widths, start=1))


def context(params):
    """The frames an utterance loses on its way through the frame-level layers."""
    return sum(spec.taps - 1 for spec in frame_variables(params))


def trained_names(params):
    """The TensorFlow names of every variable ConvTrainer updates: the frame layers first, then tail_train.trained_names."""
    out = []
    for spec in frame_variables(params):
        out += [spec.kernel, spec.bias, spec.bn + "/gamma", spec.bn + "/beta"]
    return out + tail_train.trained_names(params)


def l2_assignment(params):
    """name -> the l2 factor of its update: weight_l2_regularizer on every kernel, the convolutions' included,
    optimizer_config's rule on the head's kernel, 0 on every bias, gamma and beta."""
    reg = float(_dict(params).get("weight_l2_regularizer", 0.0))
    out = dict.fromkeys(trained_names(params), 0.0)
    out.update(tail_train.l2_assignment(params))
    for spec in frame_variables(params):
        out[spec.kernel] = reg
    return out


def out_offsets(offsets, taps):
    """offsets [B + 1] of packed input rows -> the offsets of the packed output rows of a `taps`-tap layer: utterance b keeps
    max(n_in - (taps - 1), 0) rows, packed densely from row 0."""
    n = np.maximum(np.diff(np.asarray(offsets, dtype=np.int64)) - (int(taps) - 1), 0)
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(n, dtype=np.int64)])


def kernel_to_rows(kernel):
    """A TensorFlow kernel [1, W, C, N] (conv2d), [W, C, N] (conv1d) or [C, N] (dense) -> (rows [N, W C] float32 with
    k = tau C + c, W, C)."""
    k = np.asarray(kernel, dtype=np.float32)
    if k.ndim == 4 and k.shape[0] == 1:
        k3 = k[0]
    elif k.ndim == 3:
        k3 = k
    elif k.ndim == 2:
        k3 = k[None]
    else:
        raise ValueError("a kernel [1, W, C, N], [W, C, N] or [C, N] expected, got shape %s" % (k.shape,))
    taps, channels, n = k3.shape
    return np.ascontiguousarray(k3.reshape(taps * channels, n).T), int(taps), int(channels)


def rows_to_kernel(rows, shape):
    """The inverse of kernel_to_rows: rows [N, W C] -> the TensorFlow kernel of `shape`."""
    rows = np.asarray(rows, dtype=np.float32)
    return np.ascontiguousarray(rows.T).reshape(shape).astype(np.float32)


class TConvLayer(object):
    """One frame-level layer's parameters, gradients and optimizer slots on the device.  w holds the rows [N, ldw] of the
    weights (kernel_to_rows; ldw = W C rounded up to 4, the padding stays zero)."""

    def __init__(self, kernel, bias, bn, act, device=0, num_slots=0):
        torch = losses._need_device()
        rows, self.taps, self.channels = kernel_to_rows(kernel)
        self.shape = tuple(np.shape(kernel))
        self.out_dim, self.in_dim = int(rows.shape[0]), int(rows.shape[1])
        if tuple(np.shape(bias)) != (self.out_dim,):
            raise ValueError("bias [%d] expected, got %s" % (self.out_dim, np.shape(bias)))
        self.ldw = (self.in_dim + 3) // 4 * 4
        self.act, self.device = int(act), int(device)
        self._torch, self._lib = torch, _lib.load()
        dev = "cuda:%d" % self.device
        with torch.cuda.device(self.device):
            self.w = torch.zeros((self.out_dim, self.ldw), dtype=torch.float32, device=dev)
            self.w[:, :self.in_dim] = torch.from_numpy(rows).to(dev)
            self.b = losses._f32(bias, self.device, torch)
            self.bn = None
            if bn is not None:
                if any(tuple(np.shape(v)) != (self.out_dim,) for v in bn):
                    raise ValueError("batch norm: four vectors of %d elements expected" % self.out_dim)
                self.bn = [losses._f32(v, self.device, torch) for v in bn]         # gamma, beta, moving_mean, moving_variance
            self.gw = torch.zeros_like(self.w)                                     # the padding columns stay zero
            self.gb = torch.zeros_like(self.b)
            self.ggamma = None if self.bn is None else torch.zeros_like(self.b)
            self.gbeta = None if self.bn is None else torch.zeros_like(self.b)
            self.slots = {name: [torch.zeros_like(t) for _ in range(num_slots)] for name, t, _ in self.trained()}
        self._x = self._z = self._off = self._ws = None
        self._sizes = (0, 0, 0)
        self._covers = False

    def trained(self):
        """[(name, parameter, gradient)] in the order the optimizer takes them."""
        out = [("kernel", self.w, self.gw), ("bias", self.b, self.gb)]
        if self.bn is not None:
            out += [("gamma", self.bn[0], self.ggamma), ("beta", self.bn[1], self.gbeta)]
        return out

    def _workspace(self, need, device):
        if self._ws is None or self._ws.numel() < need:
            self._ws = self._torch.empty(max(need, 16), dtype=self._torch.uint8, device=device)
        return self._ws

    def forward(self, x, offsets):
        """x [rows, C] on the device, float32 contiguous; offsets [B + 1] host integers of its rows -> (y [total_out, N] packed
        from row 0, the output offsets); x, z and the offsets are kept for backward()."""
        torch = self._torch
        if x.dim() != 2 or int(x.shape[1]) != self.channels or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("x: expected a contiguous float32 [rows, %d], got %s" % (self.channels, tuple(x.shape)))
        rows = int(x.shape[0])
        host = np.ascontiguousarray(offsets, dtype=np.int64)
        if host.ndim != 1 or host.size < 1 or host[0] < 0 or np.any(np.diff(host) < 0) or host[-1] > rows:
            raise ValueError("offsets must ascend from >= 0 to at most the %d rows of x" % rows)
        out_off = out_offsets(host, self.taps)
        batch, total_in, total_out = host.size - 1, int(host[-1] - host[0]), int(out_off[-1])
        with torch.cuda.device(self.device):
            off = torch.from_numpy(host.astype(np.int32)).to(x.device)
            z = torch.empty((max(total_out, 1), self.out_dim), dtype=torch.float32, device=x.device)
            y = torch.empty((max(total_out, 1), self.out_dim), dtype=torch.float32, device=x.device)
            if total_out:
                ws = self._workspace(int(self._lib.xv_tconv_forward_workspace(batch, total_out)), x.device)
                bn = self.bn or [None] * 4
                stream = torch.cuda.current_stream(self.device).cuda_stream
                _lib.check(self._lib.xv_tconv_forward(self.device, _p(x), self.channels, self.channels, self.taps, _p(off), batch,
                                                      total_in, total_out, _p(self.w), self.ldw, self.out_dim, _p(self.b), _p(bn[0]),
                                                      _p(bn[1]), _p(bn[2]), _p(bn[3]), self.act, _p(z), self.out_dim, _p(y),
                                                      self.out_dim, _p(ws), ws.numel(), C.c_void_p(stream)))
        self._x, self._z, self._off, self._sizes = x, z, off, (batch, total_in, total_out)
        self._covers = batch > 0 and int(host[0]) == 0 and int(host[-1]) == rows
        return y[:total_out], out_off

    def backward(self, gy, want_gx):
        """gy [total_out, N] on the device -> gx [rows, C] in the row numbering of x (rows no utterance owns: zeros) or None;
        the gradients of the parameters go to gw, gb, ggamma, gbeta."""
        torch = self._torch
        if self._x is None:
            raise RuntimeError("TConvLayer.backward needs a forward first")
        x, z = self._x, self._z
        batch, total_in, total_out = self._sizes
        if tuple(gy.shape) != (total_out, self.out_dim) or not gy.is_contiguous():
            raise ValueError("gy: expected a contiguous [%d, %d], got shape %s" % (total_out, self.out_dim, tuple(gy.shape)))
        with torch.cuda.device(self.device):
            if total_out == 0:                          # the gradient of an empty sum
                for _, _, g in self.trained():
                    g.zero_()
                return torch.zeros((int(x.shape[0]), self.channels), dtype=torch.float32, device=x.device) if want_gx else None
            gx = None
            if want_gx:
                make = torch.empty if self._covers else torch.zeros           # every row has an owner: every element is written
                gx = make((int(x.shape[0]), self.channels), dtype=torch.float32, device=x.device)
            ws = self._workspace(int(self._lib.xv_tconv_workspace(batch, total_in, total_out, self.taps, self.channels, self.out_dim)),
                                 x.device)
            bn = self.bn or [None] * 4
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._lib.xv_tconv_backward(self.device, _p(gy), self.out_dim, _p(x), self.channels, self.channels, self.taps,
                                                   _p(self._off), batch, total_in, total_out, _p(z), self.out_dim, _p(self.w), self.ldw,
                                                   self.out_dim, _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]), self.act, _p(gx),
                                                   self.channels, _p(self.gw), _p(self.gb), _p(self.ggamma), _p(self.gbeta), _p(ws),
                                                   ws.numel(), C.c_void_p(stream)))
        return gx

    def kernel(self):
        """The TensorFlow kernel in the shape the checkpoint had (rank 4, 3 or 2), float32 numpy."""
        return rows_to_kernel(self.w[:, :self.in_dim].cpu().numpy(), self.shape)


class ConvTrainer(object):
    """Every frame-level layer, statistics pooling, and a tail_train.TailTrainer (the two segment-level layers and the head)
    behind them, all built from the checkpoint's variables."""

    def __init__(self, params, weights, num_classes, device=0, seed=0, kernel=None, bias=None):
        check_supported(params)
        self.params = params
        self.frame_specs = frame_variables(params)
        self.tail = tail_train.TailTrainer(params, weights, num_classes, device, seed, kernel, bias)
        num_slots = len(self.tail.layers[0].slots["kernel"])
        self.frame_layers = []
        for spec in self.frame_specs:
            missing = [k for k in (spec.kernel, spec.bias) + tuple(spec.bn + "/" + s for s in _BN) if k not in weights]
            if missing:
                raise KeyError("the checkpoint lacks %s" % ", ".join(missing))
            layer = TConvLayer(weights[spec.kernel], weights[spec.bias], [weights[spec.bn + "/" + s] for s in _BN], spec.act, device,
                               num_slots)
            if layer.taps != spec.taps:
                raise ValueError("%s: a kernel of %d taps expected, got shape %s" % (spec.kernel, spec.taps, layer.shape))
            self.frame_layers.append(layer)
        for a, b, sa, sb in zip(self.frame_layers[:-1], self.frame_layers[1:], self.frame_specs[:-1], self.frame_specs[1:]):
            if b.channels != a.out_dim:
                raise ValueError("%s takes %d channels, %s gives %d" % (sb.kernel, b.channels, sa.kernel, a.out_dim))
        self.in_dim, self.channels = self.frame_layers[0].channels, self.frame_layers[-1].out_dim
        self.context = sum(layer.taps - 1 for layer in self.frame_layers)
        if self.tail.pool_dim != 2 * self.channels:
            raise ValueError("%s has %d rows, statistics pooling of %d channels gives %d" % (self.tail.specs[0].kernel, self.tail.pool_dim,
                                                                                             self.channels, 2 * self.channels))
        self.specs = self.frame_specs + tuple(self.tail.specs)
        self.layers = self.frame_layers + list(self.tail.layers)
        self.head = self.tail.head
        self.embed_dim = self.tail.embed_dim
        self.device = int(device)
        self.pool = frame_train.StatPool(self.channels, device)
        self.l2 = l2_assignment(params)
        torch = losses._need_device()
        self._torch, self._lib = torch, _lib.load()
        largest = max([layer.w.numel() for layer in self.layers] + [self.head.head.raw_rows.numel()])
        if self.tail._ws.numel() < int(self._lib.xv_opt_workspace(largest)):
            with torch.cuda.device(self.device):
                self.tail._ws = torch.empty(int(self._lib.xv_opt_workspace(largest)), dtype=torch.uint8, device=self.tail._ws.device)
        self.num_steps = 0                                                   # adam's t, shared by every tensor

    def tensors(self):
        """[(TensorFlow name, parameter, gradient, slots)] of everything trained, in the order of trained_names()."""
        out = []
        for spec, layer in zip(self.frame_specs, self.frame_layers):
            names = {"kernel": spec.kernel, "bias": spec.bias, "gamma": spec.bn + "/gamma", "beta": spec.bn + "/beta"}
            out += [(names[k], w, g, layer.slots[k]) for k, w, g in layer.trained()]
        return out + self.tail.tensors()

    def _feats(self, feats_dev):
        torch = self._torch
        if not torch.is_tensor(feats_dev) or not feats_dev.is_cuda:
            raise ValueError("feats_dev must be a device tensor")
        if feats_dev.dim() != 2 or int(feats_dev.shape[1]) != self.in_dim or feats_dev.dtype != torch.float32:
            raise ValueError("feats_dev: expected float32 [rows, %d], got %s" % (self.in_dim, tuple(feats_dev.shape)))
        return feats_dev.contiguous()

    def _forward(self, feats_dev, offsets):
        x, off = self._feats(feats_dev), np.ascontiguousarray(offsets, dtype=np.int64)
        if off.size > 1 and np.any(np.diff(off) <= self.context):
            raise ValueError("every utterance needs more than the %d frames of context" % self.context)
        for layer in self.frame_layers:
            x, off = layer.forward(x.contiguous(), off)
        pooled = self.pool.forward(x.contiguous(), off)
        return self.tail.layers[1].forward(self.tail.layers[0].forward(pooled.contiguous()))

    def forward(self, feats_dev, offsets):
        """feats_dev [rows, dim] on the device (packed features), offsets [B + 1] host integers of its rows -> the `output`
        endpoint [B, embed_dim] on the device, with the current weights."""
        with self._torch.cuda.device(self.device):
            return self._forward(feats_dev, offsets)

    def step(self, feats_dev, offsets, labels, learning_rate, global_step=0):
        """One training step on a batch of packed features: forward through the frame layers, the pooling and the segment
        layers, the head's mean loss at `global_step` and its gradients, backward through all of them, then per tensor l2
        (kernels only), the clip and the update -> StepResult(mean loss, top-1 accuracy), both of the parameters BEFORE the
        update."""
        torch = self._torch
        h = self.head
        with torch.cuda.device(self.device):
            y = self._forward(feats_dev, offsets)
            out, top1, gx, _, _ = h.head._grad_device(y, labels, global_step, None, True, h._grad_rows, h._grad_bias)
            n = int(out.shape[1])
            g = self.tail.layers[1].backward(gx, True)
            g = self.tail.layers[0].backward(g, True)
            g = self.pool.backward(g)
            for i in range(len(self.frame_layers) - 1, -1, -1):
                g = self.frame_layers[i].backward(g, i > 0)
            self.num_steps += 1
            self.tail.num_steps = h.num_steps = self.num_steps
            for name, w, gw, slots in self.tensors():
                self.tail._apply(w, gw, slots, learning_rate, self.l2[name])
            lab = losses._labels_dev(labels, n, out.device, torch)
            return StepResult(float(out[0].double().mean()) if n else float("nan"),
                              float((top1 == lab).double().mean()) if n else float("nan"))

    def variables(self):
        """name -> float32 numpy of every trained variable under its TensorFlow name (kernels in the checkpoint's shapes)."""
        out = collections.OrderedDict()
        for spec, layer in zip(self.frame_specs, self.frame_layers):
            out[spec.kernel] = layer.kernel()
            out[spec.bias] = layer.b.cpu().numpy().copy()
            out[spec.bn + "/gamma"] = layer.bn[0].cpu().numpy().copy()
            out[spec.bn + "/beta"] = layer.bn[1].cpu().numpy().copy()
        out.update(self.tail.variables())
        return out
