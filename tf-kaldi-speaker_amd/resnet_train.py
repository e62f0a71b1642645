"""Train EVERY layer of the ResNet-18 (model/resnet.py) together with the statistics pooling, the segment-level layers and the
head: the last part of stage two of every fine-tune (egs/voxceleb/v1/nnet/lib/finetune.py:6-7: "... and then update the entire
network") for the project's third encoder, as conv_train.py does it for the TDNN and the extended TDNN.

There is no frozen forward: the packed features [total_frames, 40] go straight in, viewed as rows (utterance, frame, bin) with one
channel, the layout of Trainer.predict_packed for a grid node.  Every 2-D convolution runs through xv_gconv_forward /
xv_gconv_backward (csrc/gconv_grad.hip) with its CURRENT weights, in exact fp32 whatever precision the extraction uses:
tf.layers.conv2d(.., padding='same', use_bias=False), then batch norm, then (for a block's first convolution and conv0_1) the
activation.  The forward order is
    conv0_1 (3 x 3, 1 -> w)
    stage s = 1 .. 4 of resnet_blocks[s - 1] blocks, w 2^(s-1) channels; the first block of a stage strides by (time_stride, 2)
    (stage 1: (1, 1)) and has the projection shortcut:
        conv0 + bn + act,  conv1 + bn,  shortcut = conv_short (1 x 1, the block's strides) + bn, or the block's input,
        y = act(conv1 + shortcut)                                  (xv_add_act_forward)
    conv5 ([1, 5, C, N], VALID: the five bins that are left become one row per frame), dense1, dense2: one-tap
    conv_train.TConvLayers; conv5 runs on the view [frames, 5 C], whose column f C + c is its kernel's row order
then frame_train.StatPool and an unchanged tail_train.TailTrainer: ResNetTrainer is a frame_train.StackedTrainer.  In backward
a block's input receives the sum of its two gradients (through conv0 and through the shortcut): one float32 addition per element,
torch.add(through conv0, through the shortcut), as att_train.py sums the two gradients of a shared frame node.  An utterance
of L frames keeps L frames, or ceil(ceil(ceil(L / 2) / 2) / 2) with resnet_time_stride; 40 bins become 20, 10, 5.

Trained: every kernel (in the checkpoint's shape, HWIO for the convolutions), the biases of conv5, dense1 and dense2, gamma and
beta of every batch norm, the head.  NOT trained: the moving statistics.  Batch norm runs in INFERENCE mode and the pooling floor
mask is a constant: **parity unpinned** against TensorFlow, pinned to torch (tests/test_gpu_resnet_train.py).  With
batch_norm="batch" every layer normalises with the statistics of the batch (all bins of all frames), the gradient goes through
them and the moving statistics move (tail_train.Layer's batch_stats; bessel by the rank of the checkpoint's kernel: true for the
convolutions and conv5, whose batch norms see rank 4, false for dense1 and dense2).

`weight_l2_regularizer` goes on every kernel (every conv2d and dense of model/resnet.py takes kernel_regularizer), nothing on
gamma, beta or a bias; the head keeps the rule of head_train.optimizer_config, the clip is per tensor, Adam's step count is
shared.  check_supported, grid_variables, frame_variables, block_plan, trained_names, l2_assignment, out_lens, kernel_to_rows and
rows_to_kernel are pure host code; the rest needs a HIP device."""
import collections

import numpy as np

from . import _lib
from ._lib import ptr
from . import conv_train
from . import frame_train
from . import head_train
from . import tail_train

StepResult = head_train.StepResult
ConvSpec = conv_train.ConvSpec
# variable names (bias: always None), XV_SEG_ACT_*, (kh, kw, st, sf)
GridSpec = collections.namedtuple("GridSpec", "kernel bias bn act window")
Block = collections.namedtuple("Block", "name strides shortcut")

SCOPE = "resnet_18"


def _dict(params):
    return params if isinstance(params, dict) else params.dict


def check_supported(params, metric=False):
    """NotImplementedError for what the ResNet stage does not cover: another network, resnet_maxpooling, PReLU, feature_norm,
    any pooling other than statistics pooling, then everything tail_train.check_supported refuses (metric: its second door)."""
    d = _dict(params)
    if d.get("network_type", "tdnn") != "resnet_18":
        raise NotImplementedError("Not implement %s network" % d.get("network_type"))
    if d.get("resnet_maxpooling"):
        raise NotImplementedError("resnet_maxpooling: the gradient of the 3 x 3 max-pooling behind conv0 is not implemented")
    if d.get("network_relu_type") == "prelu":
        raise NotImplementedError("network_relu_type prelu: the trainable alpha of the ResNet's activations is not implemented")
    if d.get("feature_norm"):
        raise NotImplementedError("feature_norm: the gradient of the l2 scaling behind the last layer is not implemented")
    if d.get("pooling_type", "statistics_pooling") != "statistics_pooling":
        raise NotImplementedError("pooling_type %s: only the gradient of statistics_pooling is implemented" % d.get("pooling_type"))
    tail_train.check_supported(params, metric)


def _act(params):
    return _lib.XV_SEG_ACT_LRELU if _dict(params).get("network_relu_type") == "lrelu" else _lib.XV_SEG_ACT_RELU


def block_plan(params):
    """-> the Blocks in forward order: (scope name, (time stride, frequency stride) of its first convolution and shortcut, whether
    it has the projection shortcut).  The first block of each stage has it; stages 2 .. 4 stride by (time_stride, 2)."""
    d = _dict(params)
    blocks = [int(n) for n in d.get("resnet_blocks") or [2, 2, 2, 2]]
    if len(blocks) != 4 or min(blocks) < 1:
        raise ValueError("resnet_blocks: four counts >= 1 expected, got %r" % (d.get("resnet_blocks"),))
    st = 2 if d.get("resnet_time_stride") else 1
    out = []
    for stage in (1, 2, 3, 4):
        out.append(Block("conv%da" % stage, (1, 1) if stage == 1 else (st, 2), True))
        out += [Block("conv%db_%d" % (stage, i), (1, 1), False) for i in range(blocks[stage - 1] - 1)]
    return out


def grid_variables(params):
    """-> the GridSpecs of every 2-D convolution in forward order, under the names of synth.synth_resnet_weights: conv0_1, then
    per block conv0, conv1 and, in the first block of a stage, conv_short.  None has a bias; conv0_1 and a block's conv0 have
    the activation."""
    act = _act(params)
    name = lambda s: "%s/%s" % (SCOPE, s)                                           # noqa: E731
    out = [GridSpec(name("conv0_1/kernel"), None, name("conv0_bn"), act, (3, 3, 1, 1))]
    for b in block_plan(params):
        st, sf = b.strides
        out.append(GridSpec(name(b.name + "_conv0/kernel"), None, name(b.name + "_bn0"), act, (3, 3, st, sf)))
        out.append(GridSpec(name(b.name + "_conv1/kernel"), None, name(b.name + "_bn1"), _lib.XV_SEG_ACT_NONE, (3, 3, 1, 1)))
        if b.shortcut:
            out.append(GridSpec(name(b.name + "_conv_short/kernel"), None, name(b.name + "_bn_short"), _lib.XV_SEG_ACT_NONE,
                                (1, 1, st, sf)))
    return tuple(out)


def frame_variables(params):
    """-> grid_variables, then the ConvSpecs (one tap) of conv5, dense1 and dense2: every layer in front of the pooling."""
    act = _act(params)
    tail = tuple(ConvSpec("%s/%s/kernel" % (SCOPE, n), "%s/%s/bias" % (SCOPE, n), "%s/%s_bn" % (SCOPE, n), act, 1)
                 for n in ("conv5", "dense1", "dense2"))
    return grid_variables(params) + tail


def trained_names(params):
    """The TensorFlow names of every variable ResNetTrainer updates (frame_train.stacked_names of frame_variables)."""
    return frame_train.stacked_names(frame_variables(params), params)


def l2_assignment(params):
    """name -> the l2 factor of its update: weight_l2_regularizer on every kernel (frame_train.stacked_l2 of frame_variables)."""
    return frame_train.stacked_l2(frame_variables(params), params)


def metric_trained_names(params):
    """trained_names behind the metric door (tail_train.metric_trained_names): no head layer."""
    return frame_train.stacked_names(frame_variables(params), params, True)


def metric_l2_assignment(params):
    return frame_train.stacked_l2(frame_variables(params), params, True)


def out_lens(lens, stride=1):
    """Frames per utterance behind a convolution with `stride` along time and 'same' padding: ceil(L / stride)."""
    n = np.asarray(lens, dtype=np.int64)
    return (n + int(stride) - 1) // int(stride)


def kernel_to_rows(kernel):
    """An HWIO kernel [kh, kw, C, N] -> (rows [N, kh kw C] float32 with k = (dl kw + df) C + c, (kh, kw), C)."""
    k = np.asarray(kernel, dtype=np.float32)
    if k.ndim != 4:
        raise ValueError("an HWIO kernel [kh, kw, C, N] expected, got shape %s" % (k.shape,))
    kh, kw, channels, n = k.shape
    return np.ascontiguousarray(k.reshape(kh * kw * channels, n).T), (int(kh), int(kw)), int(channels)


def rows_to_kernel(rows, shape):
    """The inverse of kernel_to_rows: rows [N, kh kw C] -> the HWIO kernel of `shape`."""
    return conv_train.rows_to_kernel(rows, shape)


class GridConvLayer(tail_train.Layer):
    """One 2-D convolution on packed utterances (xv_gconv_*): w holds kernel_to_rows of the HWIO kernel, whose shape is kept;
    there is no bias.  batch_stats goes through xv_bn_batch_* exactly as conv_train.TConvLayer does it, n = all bins of all
    frames."""

    def __init__(self, kernel, bn, act, strides, device=0, num_slots=0, batch_stats=False, momentum=0.99, bessel=False):
        rows, (kh, kw), self.channels = kernel_to_rows(kernel)
        self.window = (kh, kw, int(strides[0]), int(strides[1]))
        self.shape = tuple(np.shape(kernel))
        tail_train.Layer.__init__(self, rows, None, bn, act, device, num_slots, batch_stats, momentum, bessel)
        self._off = None
        self._sizes = (0, 0, 0, 0)
        self._covers = False

    def forward(self, x, offsets, bins, training=True):
        """x [frames bins, C] on the device, float32 contiguous; offsets [B + 1] host integers of its FRAMES -> (y [frames_out
        bins_out, N] packed from row 0, the output frame offsets, bins_out); x, z and the offsets are kept for backward()."""
        torch = self._torch
        kh, kw, st, sf = self.window
        bins = int(bins)
        if x.dim() != 2 or int(x.shape[1]) != self.channels or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("x: expected a contiguous float32 [rows, %d], got %s" % (self.channels, tuple(x.shape)))
        rows = int(x.shape[0])
        host = np.ascontiguousarray(offsets, dtype=np.int64)
        if host.ndim != 1 or host.size < 1 or host[0] < 0 or np.any(np.diff(host) < 0) or host[-1] * bins > rows:
            raise ValueError("offsets must ascend from >= 0 to at most the %d frames of x" % (rows // max(bins, 1)))
        out_off = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(out_lens(np.diff(host), st), dtype=np.int64)])
        bins_out = (bins + sf - 1) // sf
        batch, total_in, total_out = host.size - 1, int(host[-1] - host[0]), int(out_off[-1])
        rows_out = total_out * bins_out
        stats = self._use_batch(training, rows_out)
        with torch.cuda.device(self.device):
            off = torch.from_numpy(host.astype(np.int32)).to(x.device)
            z = torch.empty((max(rows_out, 1), self.out_dim), dtype=torch.float32, device=x.device)
            y = (self._scratch_y(rows_out, x.device) if stats
                 else torch.empty((max(rows_out, 1), self.out_dim), dtype=torch.float32, device=x.device))
            if rows_out:
                ws = self._workspace(int(self._lib.xv_gconv_forward_workspace(batch, total_out, bins, sf)), x.device)
                bn = [None] * 4 if stats else self.bn or [None] * 4
                stream = _lib.stream(self.device)
                _lib.check(self._lib.xv_gconv_forward(self.device, ptr(x), self.channels, self.channels, bins, kh, kw, st, sf, ptr(off),
                                                      batch, total_in, total_out, ptr(self.w), self.ldw, self.out_dim, None, ptr(bn[0]),
                                                      ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), _lib.XV_SEG_ACT_NONE if stats else self.act,
                                                      ptr(z), self.out_dim, ptr(y), self.out_dim, ptr(ws), ws.numel(), stream))
                if stats:
                    y = self._bn_forward(z, rows_out, stream)
        self._x, self._z, self._off, self._sizes = x, z, off, (batch, total_in, total_out, bins)
        self._covers = batch > 0 and int(host[0]) == 0 and int(host[-1]) * bins == rows
        return y[:rows_out], out_off, bins_out

    def backward(self, gy, want_gx):
        """gy [rows_out, N] on the device -> gx [rows, C] in the row numbering of x (rows no utterance owns: zeros) or None; the
        gradients of the parameters go to gw, ggamma, gbeta."""
        torch = self._torch
        if self._x is None:
            raise RuntimeError("GridConvLayer.backward needs a forward first")
        x, z = self._x, self._z
        kh, kw, st, sf = self.window
        batch, total_in, total_out, bins = self._sizes
        rows_out = total_out * ((bins + sf - 1) // sf)
        if tuple(gy.shape) != (rows_out, self.out_dim) or not gy.is_contiguous():
            raise ValueError("gy: expected a contiguous [%d, %d], got shape %s" % (rows_out, self.out_dim, tuple(gy.shape)))
        with torch.cuda.device(self.device):
            if rows_out == 0:
                return self._empty_batch(int(x.shape[0]), self.channels, want_gx)
            gx = None
            if want_gx:
                make = torch.empty if self._covers else torch.zeros           # every row has an owner: every element is written
                gx = make((int(x.shape[0]), self.channels), dtype=torch.float32, device=x.device)
            ws = self._workspace(int(self._lib.xv_gconv_workspace(batch, total_in, total_out, bins, kh, kw, st, sf, self.channels,
                                                                  self.out_dim)), x.device)
            stream = _lib.stream(self.device)
            bn, act, g, gg, gbe = self.bn or [None] * 4, self.act, gy, self.ggamma, self.gbeta
            if self._batch:                  # through the statistics first; the operator then passes gz through its mask
                g = self._bn_backward(gy, z, rows_out, stream)
                bn, act, gg, gbe = [None] * 4, _lib.XV_SEG_ACT_NONE, None, None
            _lib.check(self._lib.xv_gconv_backward(self.device, ptr(g), self.out_dim, ptr(x), self.channels, self.channels, bins, kh, kw,
                                                   st, sf, ptr(self._off), batch, total_in, total_out, ptr(z), self.out_dim, ptr(self.w),
                                                   self.ldw, self.out_dim, ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), act, ptr(gx),
                                                   self.channels, ptr(self.gw), None, ptr(gg), ptr(gbe), ptr(ws), ws.numel(), stream))
        return gx

    def kernel(self):
        """The HWIO kernel in the checkpoint's shape, float32 numpy."""
        return rows_to_kernel(self.w[:, :self.in_dim].cpu().numpy(), self.shape)


class AddAct(object):
    """The residual join of a block, y = act(p + q), with its gradient (xv_add_act_forward / xv_add_act_backward): forward()
    keeps p and q for backward(), whose result is the gradient of both."""

    def __init__(self, act, device=0):
        self.act, self.device = int(act), int(device)
        self._torch, self._lib = tail_train.losses._need_device(), _lib.load()
        self._p = self._q = None

    def _call(self, gy, p, q):
        torch = self._torch
        rows, n = int(p.shape[0]), int(p.shape[1])
        with torch.cuda.device(self.device):
            out = torch.empty((rows, n), dtype=torch.float32, device=p.device)
            stream = _lib.stream(self.device)
            if gy is None:
                _lib.check(self._lib.xv_add_act_forward(self.device, ptr(p), n, ptr(q), n, rows, n, self.act, ptr(out), n, stream))
            else:
                _lib.check(self._lib.xv_add_act_backward(self.device, ptr(gy), n, ptr(p), n, ptr(q), n, rows, n, self.act, ptr(out), n,
                                                         stream))
        return out

    def forward(self, p, q):
        if p.shape != q.shape or p.dim() != 2 or not (p.is_contiguous() and q.is_contiguous()):
            raise ValueError("the two branches of a block: contiguous [rows, N] of one shape expected, got %s and %s"
                             % (tuple(p.shape), tuple(q.shape)))
        self._p, self._q = p, q
        return self._call(None, p, q)

    def backward(self, gy):
        if self._p is None:
            raise RuntimeError("AddAct.backward needs a forward first")
        if gy.shape != self._p.shape or not gy.is_contiguous():
            raise ValueError("gy: expected a contiguous %s, got %s" % (tuple(self._p.shape), tuple(gy.shape)))
        return self._call(gy, self._p, self._q)


class ResNetTrainer(frame_train.StackedTrainer):
    """Every layer of the ResNet-18 on the packed features: GridConvLayers and the residual joins, then conv5, dense1 and dense2
    as one-tap conv_train.TConvLayers.  forward(feats_dev, offsets), step(feats_dev, offsets, labels, learning_rate,
    global_step=0, mark=None); feats_dev [total_frames, 40] on the device, offsets host integers of its frames."""

    _check, _specs, _l2 = staticmethod(check_supported), staticmethod(frame_variables), staticmethod(l2_assignment)
    _metric_l2 = staticmethod(metric_l2_assignment)
    _CHAIN = "%s takes %d channels, %s gives %d"
    _INPUT = ("feats_dev", "")

    def __init__(self, params, weights, num_classes, device=0, seed=0, kernel=None, bias=None, batch_norm="moving", metric=False):
        self.blocks = block_plan(params)
        frame_train.StackedTrainer.__init__(self, params, weights, num_classes, device, seed, kernel, bias, batch_norm, metric)
        self.joins = [AddAct(_act(params), device) for _ in self.blocks]
        self.time_stride = 2 if _dict(params).get("resnet_time_stride") else 1

    def _layer(self, spec, kernel, bias, bn, device, num_slots):
        if isinstance(spec, GridSpec):
            k = np.asarray(kernel)
            if k.ndim != 4 or tuple(k.shape[:2]) != spec.window[:2]:
                raise ValueError("%s: a kernel [%d, %d, C, N] expected, got shape %s" % ((spec.kernel,) + spec.window[:2] + (k.shape,)))
            return GridConvLayer(kernel, bn, spec.act, spec.window[2:], device, num_slots, **self._stats(kernel))
        k = np.asarray(kernel, dtype=np.float32)
        if spec.kernel.endswith("conv5/kernel"):
            # [1, F, C, N], VALID over the F bins that are left: one tap on the view [frames, F C], saved in the checkpoint's shape
            if k.ndim != 4 or k.shape[0] != 1:
                raise ValueError("%s: a kernel [1, F, C, N] expected, got shape %s" % (spec.kernel, k.shape))
            layer = conv_train.TConvLayer(k.reshape(k.shape[1] * k.shape[2], k.shape[3]), bias, bn, spec.act, device, num_slots,
                                          **self._stats(kernel))
            layer.shape, layer.bins = tuple(k.shape), int(k.shape[1])
            return layer
        if k.ndim != 2:
            raise ValueError("%s: a dense kernel [cin, cout] expected, got shape %s" % (spec.kernel, k.shape))
        return conv_train.TConvLayer(k, bias, bn, spec.act, device, num_slots, **self._stats(k))

    def _width(self, layer):
        return layer.channels

    def _check_chain(self):
        """conv0_1 takes one channel; a block's conv0 and shortcut take the block's input, its conv1 what conv0 gives, and the
        two branches of the join agree; conv5 takes the last block's channels in each of its bins; then a chain."""
        specs, layers = self.frame_specs, self.frame_layers

        def need(i, width, j, gives):
            if width != gives:
                raise ValueError(self._CHAIN % (specs[i].kernel, width, specs[j].kernel if j >= 0 else "the feature grid", gives))
        need(0, layers[0].channels, -1, 1)
        i, src = 1, 0                                                     # src: the layer whose output is the block's input
        for b in self.blocks:
            need(i, layers[i].channels, src, layers[src].out_dim)
            need(i + 1, layers[i + 1].channels, i, layers[i].out_dim)
            if b.shortcut:
                need(i + 2, layers[i + 2].channels, src, layers[src].out_dim)
                need(i + 2, layers[i + 2].out_dim, i + 1, layers[i + 1].out_dim)
            else:
                need(i + 1, layers[i + 1].out_dim, src, layers[src].out_dim)
            src = i + 1
            i += 3 if b.shortcut else 2
        conv5 = layers[i]
        need(i, conv5.channels // conv5.bins, src, layers[src].out_dim)
        need(i + 1, layers[i + 1].channels, i, conv5.out_dim)
        need(i + 2, layers[i + 2].channels, i + 1, layers[i + 1].out_dim)

    def _packed(self, x_dev):
        torch = self._torch
        if not torch.is_tensor(x_dev) or not x_dev.is_cuda:
            raise ValueError("feats_dev must be a device tensor")
        if x_dev.dim() != 2 or x_dev.dtype != torch.float32 or int(x_dev.shape[1]) < 1:
            raise ValueError("feats_dev: expected float32 [frames, bins], got %s" % (tuple(x_dev.shape),))
        return x_dev.contiguous()

    def _offsets(self, offsets):
        return np.ascontiguousarray(offsets, dtype=np.int64)

    def _walk(self, x, off, mark, training=True, keep=None):
        layers, fwd = self.frame_layers, tail_train.layer_forward
        bins = int(x.shape[1])
        x, off, bins = fwd(layers[0], training, x.reshape(-1, 1), off, bins)
        mark("frame_forward/0")
        i = 1
        for b, join in zip(self.blocks, self.joins):
            a, aoff, abins = fwd(layers[i], training, x, off, bins)
            mark("frame_forward/%d" % i)
            p, _, _ = fwd(layers[i + 1], training, a, aoff, abins)
            mark("frame_forward/%d" % (i + 1))
            q = x
            if b.shortcut:
                q, _, _ = fwd(layers[i + 2], training, x, off, bins)
                mark("frame_forward/%d" % (i + 2))
            x, off, bins = join.forward(p.contiguous(), q.contiguous()), aoff, abins
            mark("join_forward/%s" % b.name)
            i += 3 if b.shortcut else 2
        if bins != layers[i].bins:
            raise ValueError("%s takes %d bins, the last block gives %d: the features must have %d bins"
                             % (self.frame_specs[i].kernel, layers[i].bins, bins, 8 * layers[i].bins))
        x = x.reshape(int(off[-1]), bins * int(x.shape[1]))               # conv5: the bins of a frame side by side
        for j in range(i, i + 3):
            x, off = fwd(layers[j], training, x.contiguous(), off)
            if keep is not None:
                keep[j] = (x, off)
            mark("frame_forward/%d" % j)
        return x, off

    def _backward(self, gy, mark):
        torch = self._torch
        layers = self.frame_layers
        g = self.tail._backward(gy, True)
        mark("segment_backward")
        g = self.pool.backward(g)
        mark("pool_backward")
        n = len(layers)
        for j in range(n - 1, n - 4, -1):
            g = layers[j].backward(g, True)
            mark("frame_backward/%d" % j)
        i = n - 3
        g = g.reshape(-1, layers[i].channels // layers[i].bins)           # back to rows (utterance, frame, bin)
        for b, join in zip(reversed(self.blocks), reversed(self.joins)):
            i -= 3 if b.shortcut else 2
            gj = join.backward(g.contiguous())
            mark("join_backward/%s" % b.name)
            g1 = layers[i + 1].backward(gj, True)
            mark("frame_backward/%d" % (i + 1))
            g1 = layers[i].backward(g1, True)
            mark("frame_backward/%d" % i)
            g2 = gj
            if b.shortcut:
                g2 = layers[i + 2].backward(gj, True)
                mark("frame_backward/%d" % (i + 2))
            g = torch.add(g1, g2)                                         # the block's input: through conv0 + through the shortcut
        layers[0].backward(g, False)
        mark("frame_backward/0")
        mark("frame_backward")
