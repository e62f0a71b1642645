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
Behind them frame_train.StatPool and an unchanged tail_train.TailTrainer: ConvTrainer is a frame_train.StackedTrainer whose frame
layers are TConvLayers (a tail_train.Layer on xv_tconv_*), and takes its step from there.  A step is: the frame layers forward, StatPool.forward,
the two segment layers, one xv_loss_classifier_grad, the segment layers backward, StatPool.backward, the frame layers backward
in reverse (no gx for the first), one xv_opt_step per tensor.  Trained: every kernel (the convolutions' in the shape the
checkpoint had, rank 4 or 3) and bias, gamma and beta of every batch norm, the head.  NOT trained: the moving statistics.
Batch norm runs in INFERENCE mode and the pooling floor mask is a constant: **parity unpinned**, as for tail_train.py.  With
batch_norm="batch" every layer normalises with the statistics of the batch (all output rows of all utterances), the gradient
goes through them and the moving statistics move (tail_train.Layer's batch_stats; bessel for the rank-4 kernels only).

`weight_l2_regularizer` goes on every kernel, the convolutions' included (model/tdnn.py: every layer takes kernel_regularizer);
the head keeps the rule of head_train.optimizer_config, the clip is per tensor, Adam's step count is shared.
frame_variables, trained_names, l2_assignment, check_supported, out_offsets, kernel_to_rows and rows_to_kernel are pure host
code; the rest needs a HIP device."""
import collections

import numpy as np

from . import _lib
from ._lib import ptr
from . import frame_train
from . import head_train
from . import tail_train

StepResult = head_train.StepResult
ConvSpec = collections.namedtuple("ConvSpec", "kernel bias bn act taps")      # variable names, XV_SEG_ACT_*, kernel width

# network_type -> (variable scope, the kernel widths of the frame-level layers in forward order)
_NETS = {"tdnn": ("tdnn", (5, 5, 7, 1, 1)), "extended_tdnn": ("etdnn", (5, 1, 5, 1, 7, 1, 9, 1, 1, 1))}


def _dict(params):
    return params if isinstance(params, dict) else params.dict


def check_supported(params, metric=False):
    """NotImplementedError for everything frame_train.check_supported refuses: ResNet-18, any pooling other than statistics
    pooling, PReLU, feature_norm, the heads and optimizers HeadTrainer refuses (metric: tail_train's second door)."""
    frame_train.check_supported(params, metric)


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
    """The TensorFlow names of every variable ConvTrainer updates (frame_train.stacked_names of frame_variables)."""
    return frame_train.stacked_names(frame_variables(params), params)


def l2_assignment(params):
    """name -> the l2 factor of its update, the convolutions' kernels included (frame_train.stacked_l2 of frame_variables)."""
    return frame_train.stacked_l2(frame_variables(params), params)


def metric_trained_names(params):
    """trained_names behind the metric door (tail_train.metric_trained_names): no head layer."""
    return frame_train.stacked_names(frame_variables(params), params, True)


def metric_l2_assignment(params):
    return frame_train.stacked_l2(frame_variables(params), params, True)


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


class TConvLayer(tail_train.Layer):
    """One frame-level layer on packed utterances: w holds kernel_to_rows of the TensorFlow kernel, whose shape is kept."""

    def __init__(self, kernel, bias, bn, act, device=0, num_slots=0, batch_stats=False, momentum=0.99, bessel=False):
        rows, self.taps, self.channels = kernel_to_rows(kernel)
        self.shape = tuple(np.shape(kernel))
        if tuple(np.shape(bias)) != (int(rows.shape[0]),):
            raise ValueError("bias [%d] expected, got %s" % (int(rows.shape[0]), np.shape(bias)))
        tail_train.Layer.__init__(self, rows, bias, bn, act, device, num_slots, batch_stats, momentum, bessel)
        self._off = None
        self._sizes = (0, 0, 0)
        self._covers = False

    def forward(self, x, offsets, training=True):
        """x [rows, C] on the device, float32 contiguous; offsets [B + 1] host integers of its rows -> (y [total_out, N] packed
        from row 0, the output offsets); x, z and the offsets are kept for backward().  With batch_stats, training chooses
        between the statistics of the batch (all output rows of all utterances) and the moving ones."""
        torch = self._torch
        if x.dim() != 2 or int(x.shape[1]) != self.channels or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("x: expected a contiguous float32 [rows, %d], got %s" % (self.channels, tuple(x.shape)))
        rows = int(x.shape[0])
        host = np.ascontiguousarray(offsets, dtype=np.int64)
        if host.ndim != 1 or host.size < 1 or host[0] < 0 or np.any(np.diff(host) < 0) or host[-1] > rows:
            raise ValueError("offsets must ascend from >= 0 to at most the %d rows of x" % rows)
        out_off = out_offsets(host, self.taps)
        batch, total_in, total_out = host.size - 1, int(host[-1] - host[0]), int(out_off[-1])
        stats = self._use_batch(training, total_out)
        with torch.cuda.device(self.device):
            off = torch.from_numpy(host.astype(np.int32)).to(x.device)
            z = torch.empty((max(total_out, 1), self.out_dim), dtype=torch.float32, device=x.device)
            y = (self._scratch_y(total_out, x.device) if stats
                 else torch.empty((max(total_out, 1), self.out_dim), dtype=torch.float32, device=x.device))
            if total_out:
                ws = self._workspace(int(self._lib.xv_tconv_forward_workspace(batch, total_out)), x.device)
                bn = [None] * 4 if stats else self.bn or [None] * 4
                stream = _lib.stream(self.device)
                _lib.check(self._lib.xv_tconv_forward(self.device, ptr(x), self.channels, self.channels, self.taps, ptr(off), batch,
                                                      total_in, total_out, ptr(self.w), self.ldw, self.out_dim, ptr(self.b), ptr(bn[0]),
                                                      ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), _lib.XV_SEG_ACT_NONE if stats else self.act,
                                                      ptr(z), self.out_dim, ptr(y), self.out_dim, ptr(ws), ws.numel(),
                                                      stream))
                if stats:
                    y = self._bn_forward(z, total_out, stream)
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
            if total_out == 0:
                return self._empty_batch(int(x.shape[0]), self.channels, want_gx)
            gx = None
            if want_gx:
                make = torch.empty if self._covers else torch.zeros           # every row has an owner: every element is written
                gx = make((int(x.shape[0]), self.channels), dtype=torch.float32, device=x.device)
            ws = self._workspace(int(self._lib.xv_tconv_workspace(batch, total_in, total_out, self.taps, self.channels, self.out_dim)),
                                 x.device)
            bn = self.bn or [None] * 4
            stream = _lib.stream(self.device)
            if self._batch:                  # through the statistics first; the operator then passes gz through its mask
                gz = self._bn_backward(gy, z, total_out, stream)
                _lib.check(self._lib.xv_tconv_backward(self.device, ptr(gz), self.out_dim, ptr(x), self.channels, self.channels,
                                                       self.taps, ptr(self._off), batch, total_in, total_out, ptr(z), self.out_dim,
                                                       ptr(self.w), self.ldw, self.out_dim, None, None, None, None,
                                                       _lib.XV_SEG_ACT_NONE, ptr(gx), self.channels, ptr(self.gw), ptr(self.gb), None,
                                                       None, ptr(ws), ws.numel(), stream))
                return gx
            _lib.check(self._lib.xv_tconv_backward(self.device, ptr(gy), self.out_dim, ptr(x), self.channels, self.channels, self.taps,
                                                   ptr(self._off), batch, total_in, total_out, ptr(z), self.out_dim, ptr(self.w), self.ldw,
                                                   self.out_dim, ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), self.act, ptr(gx),
                                                   self.channels, ptr(self.gw), ptr(self.gb), ptr(self.ggamma), ptr(self.gbeta), ptr(ws),
                                                   ws.numel(), stream))
        return gx

    def kernel(self):
        """The TensorFlow kernel in the shape the checkpoint had (rank 4, 3 or 2), float32 numpy."""
        return rows_to_kernel(self.w[:, :self.in_dim].cpu().numpy(), self.shape)


class ConvTrainer(frame_train.StackedTrainer):
    """Every frame-level layer on the packed features: TConvLayers, each handing its output offsets to the next.
    forward(feats_dev, offsets), step(feats_dev, offsets, labels, learning_rate, global_step=0, mark=None); offsets are host
    integers."""

    _check, _specs, _l2 = staticmethod(check_supported), staticmethod(frame_variables), staticmethod(l2_assignment)
    _metric_l2 = staticmethod(metric_l2_assignment)
    _CHAIN = "%s takes %d channels, %s gives %d"
    _INPUT = ("feats_dev", "")

    def __init__(self, params, weights, num_classes, device=0, seed=0, kernel=None, bias=None, batch_norm="moving", metric=False):
        frame_train.StackedTrainer.__init__(self, params, weights, num_classes, device, seed, kernel, bias, batch_norm, metric)
        self.context = sum(layer.taps - 1 for layer in self.frame_layers)

    def _layer(self, spec, kernel, bias, bn, device, num_slots):
        layer = TConvLayer(kernel, bias, bn, spec.act, device, num_slots, **self._stats(kernel))
        if layer.taps != spec.taps:
            raise ValueError("%s: a kernel of %d taps expected, got shape %s" % (spec.kernel, spec.taps, layer.shape))
        return layer

    def _width(self, layer):
        return layer.channels

    def _offsets(self, offsets):
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        if off.size > 1 and np.any(np.diff(off) <= self.context):
            raise ValueError("every utterance needs more than the %d frames of context" % self.context)
        return off

    def _walk(self, x, off, mark, training=True, keep=None):
        for i, layer in enumerate(self.frame_layers):
            x, off = tail_train.layer_forward(layer, training, x.contiguous(), off)
            if keep is not None:
                keep[i] = (x, off)
            mark("frame_forward/%d" % i)
        return x, off
