"""Train attention models: the frame layers, the key and value networks, the query, the segment-level layers and the head of a
`self_attention` model (model/pooling.py:55-240; egs/voxceleb/v1/nnet_conf/tdnn_softmax_1e-2_tdnn4_att_pretrain.json), the
counterpart of frame_train.py and conv_train.py, which keep refusing every pooling_type but statistics_pooling.

The one new mathematical piece is attentive pooling of the caller's own packed rows with its gradient (csrc/att_pool_grad.hip,
xv_att_pool_forward / xv_att_pool_backward; the rule and its rounding order are stated in include/xvec_hip.h): AttPool.  The key
and value networks are dense (+ bn) (+ relu) layers on packed frames, tail_train.SegLayer: kind 0 is dense, kind 1 dense + relu
or leaky relu, kind 2 dense + bn + activation, and the intermediate layers are always kind 2.  The variable names are the
reference's: <scope>/attention/att_key<i>/att_key<i>_dense/kernel, ..., <scope>/attention/query.

The graph is no longer a chain.  A frame node tdnn<i>_relu that feeds both the next frame layer and a key or value network
receives the sum of both gradients, one float32 addition per element, the chain's gradient first; where the key and the value
read the same node, the key branch and the value branch are added first (key + value), then the chain's in front.

AttFrameTrainer is frame_train.FrameTrainer and AttConvTrainer conv_train.ConvTrainer with this pooling stage in the place of
StatPool; the step, the optimizer and batch_norm="batch" are tail_train's.  Trained additionally: the attention kernels (with
weight_l2_regularizer: model/common.py gives every dense a kernel_regularizer), biases, gamma and beta, and the query (no l2);
in batch mode variables() also returns the moved statistics of the kind-2 attention layers (biased variance: rank-2 kernels).
**Parity unpinned** against TensorFlow, pinned to torch float64 (tests/test_gpu_att_train.py).

Not covered, refused with a message by check_supported: tanh key / value layers (att_*_network_type 3), att_apply_nonlinear,
att_penalty_term > 0, more than XV_MAX_ATT_LAYERS layers, ResNet-18, a last frame layer that reaches the pooled vector through
neither input, key and value nodes of different lengths, for AttFrameTrainer an input in front of the frozen node, and
everything tail_train.check_supported refuses.  check_supported, attention_variables, trained_names and l2_assignment are pure
host code; the rest needs a HIP device."""
import ctypes as C
import re

import numpy as np

from . import _lib
from ._lib import ptr
from . import conv_train
from . import frame_train
from . import head_train
from . import losses
from . import tail_train

StepResult = head_train.StepResult
SegSpec = tail_train.SegSpec


def _dict(params):
    return params if isinstance(params, dict) else params.dict


def _scope(d):
    return conv_train._NETS[d.get("network_type", "tdnn")][0]


def _node(d, which):
    """The 1-based number of the frame layer whose tdnn<i>_relu endpoint feeds the key or the value network."""
    name = str(d.get("att_%s_input" % which))
    m = re.match(r"tdnn(\d+)_relu$", name)
    widths = conv_train._NETS[d.get("network_type", "tdnn")][1]
    if not m or not 1 <= int(m.group(1)) <= len(widths):
        raise NotImplementedError("att_%s_input %s: only the tdnn<i>_relu endpoints of the %d frame layers can feed a trained "
                                  "attention" % (which, name, len(widths)))
    return int(m.group(1))


def check_supported(params, conv_layers=False, metric=False):
    """NotImplementedError, with the reason, for what the attention trainers do not cover (the module's docstring lists it).
    conv_layers: every frame layer is trained (AttConvTrainer); otherwise the layers behind frame_train.frozen_node
    (AttFrameTrainer), and an attention input in front of that node is refused as well."""
    d = _dict(params)
    net = d.get("network_type", "tdnn")
    if net == "resnet_18":
        raise NotImplementedError("resnet_18: no 1-tap frame layers lie between its convolutions and the pooling node")
    if d.get("pooling_type", "statistics_pooling") != "self_attention":
        raise NotImplementedError("pooling_type %s: att_train trains self_attention models (frame_train and conv_train train "
                                  "statistics_pooling)" % d.get("pooling_type", "statistics_pooling"))
    for which in ("key", "value"):
        kind = int(d.get("att_%s_network_type" % which, 0))
        if kind == 3:
            raise NotImplementedError("att_%s_network_type 3 (tanh): xv_seg_forward has no such activation" % which)
        if kind not in (0, 1, 2):
            raise NotImplementedError("att_%s_network_type %d is not one of 0, 1, 2" % (which, kind))
    if d.get("att_apply_nonlinear"):
        raise NotImplementedError("att_apply_nonlinear: the batch norm and activation behind the attention are not implemented")
    if float(d.get("att_penalty_term", 0) or 0) > 0:
        raise NotImplementedError("att_penalty_term > 0: the gradient of the multi-head penalty is not implemented")
    nk, nv = len(d.get("att_key_num_nodes", ())), len(d.get("att_value_num_nodes", ()))
    if not 1 <= nk <= _lib.XV_MAX_ATT_LAYERS or nv > _lib.XV_MAX_ATT_LAYERS:
        raise NotImplementedError("att_key_num_nodes needs 1 .. %d layers and att_value_num_nodes at most %d, got %d and %d"
                                  % (_lib.XV_MAX_ATT_LAYERS, _lib.XV_MAX_ATT_LAYERS, nk, nv))
    tail_train.check_supported(params, metric)
    if net not in conv_train._NETS:
        raise NotImplementedError("Not implement %s network" % net)
    widths = conv_train._NETS[net][1]
    key, value = _node(d, "key"), _node(d, "value")
    if max(key, value) < len(widths):
        raise NotImplementedError("the last frame layer tdnn%d reaches the pooled vector through neither att_key_input nor "
                                  "att_value_input: its variables would get only the l2 term" % len(widths))
    if any(w > 1 for w in widths[min(key, value):max(key, value)]):
        raise NotImplementedError("att_key_input %s and att_value_input %s: a multi-tap layer lies between them, the key and the "
                                  "value must have the same number of frames" % (d.get("att_key_input"), d.get("att_value_input")))
    if not conv_layers:
        frozen = frame_train._FRAME[net][2]
        for which, idx in (("key", key), ("value", value)):
            if idx < frozen:
                raise NotImplementedError("att_%s_input %s lies in front of the frozen node %s: train it with conv_layers"
                                          % (which, d.get("att_%s_input" % which), frame_train.frozen_node(params)))


def attention_variables(params):
    """-> (SegSpecs of the key network, SegSpecs of the value network, the query's name), under the names synth.synth_weights
    and oracle/ref_numpy.py use.  The intermediate layers are dense + bn + activation; the last takes att_*_network_type."""
    d = _dict(params)
    base = _scope(d) + "/attention"
    act = _lib.XV_SEG_ACT_LRELU if d.get("network_relu_type") == "lrelu" else _lib.XV_SEG_ACT_RELU
    out = []
    for which in ("key", "value"):
        nodes = list(d.get("att_%s_num_nodes" % which, ()))
        specs = []
        for i in range(len(nodes)):
            kind = 2 if i < len(nodes) - 1 else int(d.get("att_%s_network_type" % which, 0))
            name = "%s/att_%s%d/att_%s%d" % (base, which, i, which, i)
            specs.append(SegSpec(name + "_dense/kernel", name + "_dense/bias", name + "_bn" if kind == 2 else None,
                                 act if kind in (1, 2) else _lib.XV_SEG_ACT_NONE))
        out.append(tuple(specs))
    return out[0], out[1], base + "/query"


def _frame_specs(params, conv_layers):
    return conv_train.frame_variables(params) if conv_layers else frame_train.frame_variables(params)


def _layer_names(specs):
    out = []
    for spec in specs:
        out += [spec.kernel, spec.bias]
        if spec.bn:
            out += [spec.bn + "/gamma", spec.bn + "/beta"]
    return out


def trained_names(params, conv_layers=False, metric=False):
    """The TensorFlow names of every variable the attention trainer updates: the frame layers, the key network, the value
    network, the query, then tail_train.trained_names."""
    key, value, query = attention_variables(params)
    return _layer_names(_frame_specs(params, conv_layers)) + _layer_names(key + value) + [query] + tail_train._trained_names(params, metric)


def l2_assignment(params, conv_layers=False, metric=False):
    """name -> the l2 factor of its update: weight_l2_regularizer on every kernel, the attention's included, optimizer_config's
    rule on the head's kernel, 0 on the query and on every bias, gamma and beta."""
    reg = float(_dict(params).get("weight_l2_regularizer", 0.0))
    out = dict.fromkeys(trained_names(params, conv_layers, metric), 0.0)
    out.update(tail_train._l2_assignment(params, metric))
    key, value, _ = attention_variables(params)
    for spec in tuple(_frame_specs(params, conv_layers)) + key + value:
        out[spec.kernel] = reg
    return out


class AttPool(object):
    """Self-attentive pooling of packed rows with its gradient (xv_att_pool_forward / xv_att_pool_backward), the counterpart of
    frame_train.StatPool.  It holds the query [H, dq] as a trained tensor: q, its gradient gq and the optimizer slots.
    forward(key_rows, value_rows, offsets) -> pooled [B, 2 P]; backward(g_pooled) -> (gkey, gvalue), gq is written."""

    def __init__(self, query, key_dim, value_dim, split_key, split_value, use_scale, device=0, num_slots=0):
        torch = losses._need_device()
        query = np.asarray(query, dtype=np.float32)
        if query.ndim != 2:
            raise ValueError("query [heads, dq] expected, got shape %s" % (query.shape,))
        self.heads, self.dq = int(query.shape[0]), int(query.shape[1])
        self.key_dim, self.value_dim = int(key_dim), int(value_dim)
        self.split_key, self.split_value, self.device = bool(split_key), bool(split_value), int(device)
        if self.key_dim != (self.heads * self.dq if self.split_key else self.dq):
            raise ValueError("a query of %d heads x %d columns does not fit a key of %d columns (split_key %s)"
                             % (self.heads, self.dq, self.key_dim, self.split_key))
        if self.split_value and self.value_dim % self.heads:
            raise ValueError("the value's %d columns cannot be split into %d heads" % (self.value_dim, self.heads))
        self.dv = self.value_dim // self.heads if self.split_value else self.value_dim
        self.out_dim = 2 * self.heads * self.dv
        self.scale = float(np.float32(1.0 / np.sqrt(float(self.dq)))) if use_scale else 1.0
        self._torch, self._lib = torch, _lib.load()
        with torch.cuda.device(self.device):
            self.q = losses._f32(query, self.device, torch).contiguous()
            self.gq = torch.zeros_like(self.q)
            self.slots = [torch.zeros_like(self.q) for _ in range(num_slots)]
        self._key = self._value = self._offsets = self._weights = self._pooled = self._var = self._ws = None
        self._batch = self._rows = 0
        self._covers = False

    def _call_args(self):
        return (ptr(self._key), self.key_dim, self.key_dim, ptr(self._value), self.value_dim, self.value_dim, ptr(self.q), self.dq,
                self.heads, int(self.split_key), int(self.split_value), C.c_float(self.scale), ptr(self._offsets), self._batch,
                self._rows, ptr(self._weights), self.heads, ptr(self._pooled), self.out_dim, ptr(self._var), self.out_dim // 2)

    def forward(self, key_rows, value_rows, offsets):
        """key_rows [rows, Dk], value_rows [rows, Dv] on the device, float32 contiguous; offsets [B + 1] (host integers or an
        int32 device tensor) of both -> pooled [B, 2 P] = [mean | std] on the device.  weights [rows, H] is kept."""
        torch = self._torch
        rows = int(key_rows.shape[0])
        for name, t, width in (("key_rows", key_rows, self.key_dim), ("value_rows", value_rows, self.value_dim)):
            if t.dim() != 2 or tuple(t.shape) != (rows, width) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("%s: expected a contiguous float32 [%d, %d], got %s" % (name, rows, width, tuple(t.shape)))
        with torch.cuda.device(self.device):
            if torch.is_tensor(offsets):
                off = offsets.to(device=key_rows.device, dtype=torch.int32).contiguous()
                covers = False                                   # not known without a copy to the host
            else:
                host = np.ascontiguousarray(offsets, dtype=np.int64)
                if host.ndim != 1 or host.size < 1 or host[0] < 0 or np.any(np.diff(host) < 0) or host[-1] > rows:
                    raise ValueError("offsets must ascend from >= 0 to at most the %d rows of the key" % rows)
                off = torch.from_numpy(host.astype(np.int32)).to(key_rows.device)
                covers = host.size > 1 and int(host[0]) == 0 and int(host[-1]) == rows
            batch = int(off.numel()) - 1
            self._key, self._value, self._offsets, self._batch, self._rows, self._covers = key_rows, value_rows, off, batch, rows, covers
            self._weights = torch.empty((max(rows, 1), self.heads), dtype=torch.float32, device=key_rows.device)
            self._pooled = torch.empty((max(batch, 1), self.out_dim), dtype=torch.float32, device=key_rows.device)
            self._var = torch.empty((max(batch, 1), self.out_dim // 2), dtype=torch.float32, device=key_rows.device)
            stream = _lib.stream(self.device)
            _lib.check(self._lib.xv_att_pool_forward(self.device, *self._call_args(), stream))
        return self._pooled[:batch]

    def weights(self):
        """The attention weights [rows, H] of the last forward, on the device (rows no utterance owns hold nothing)."""
        return self._weights[:self._rows]

    def backward(self, g_pooled):
        """g_pooled [B, 2 P] on the device -> (gkey [rows, Dk], gvalue [rows, Dv]); rows no utterance owns come back as zeros.
        The gradient of the query goes to gq."""
        torch = self._torch
        if self._key is None:
            raise RuntimeError("AttPool.backward needs a forward first")
        if tuple(g_pooled.shape) != (self._batch, self.out_dim) or not g_pooled.is_contiguous():
            raise ValueError("g_pooled: expected a contiguous [%d, %d], got %s" % (self._batch, self.out_dim, tuple(g_pooled.shape)))
        with torch.cuda.device(self.device):
            make = torch.empty if self._covers else torch.zeros           # every row has an owner: every element is written
            dev = self._key.device
            gkey = make((self._rows, self.key_dim), dtype=torch.float32, device=dev)
            gvalue = make((self._rows, self.value_dim), dtype=torch.float32, device=dev)
            if self._batch == 0:
                self.gq.zero_()
                return gkey, gvalue
            need = int(self._lib.xv_att_pool_workspace(self._batch, self._rows, self.heads, self.key_dim, self.value_dim,
                                                       int(self.split_key), int(self.split_value)))
            if need < 0:
                _lib.check(need)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            stream = _lib.stream(self.device)
            args = self._call_args()
            _lib.check(self._lib.xv_att_pool_backward(self.device, ptr(g_pooled), self.out_dim, *args, ptr(gkey), self.key_dim,
                                                      ptr(gvalue), self.value_dim, ptr(self.gq), self.dq, ptr(self._ws),
                                                      self._ws.numel(), stream))
        return gkey, gvalue

    def query(self):
        """The query [H, dq], float32 numpy."""
        return self.q.cpu().numpy().copy()


class _AttStage(object):
    """What AttFrameTrainer and AttConvTrainer add to their StackedTrainer: the key and value networks and AttPool in the place
    of StatPool, the endpoints kept during the walk, and the sum of the gradients a frame node receives."""

    def _make_pool(self, weights, num_slots):
        d = _dict(self.params)
        self.key_specs, self.value_specs, self.query_name = attention_variables(self.params)
        first = len(conv_train._NETS[d.get("network_type", "tdnn")][1]) - len(self.frame_layers) + 1   # the first trained layer
        self.key_node, self.value_node = _node(d, "key") - first, _node(d, "value") - first           # -1: the trainer's input

        def width(node):
            return self.in_dim if node < 0 else self.frame_layers[node].out_dim

        def chain(specs, cin, what):
            layers = []
            for spec in specs:
                kernel, bias, bn = tail_train.layer_weights(spec, weights)
                layer = tail_train.SegLayer(kernel, bias, bn, spec.act, self.device, num_slots, **self._stats(np.asarray(kernel)))
                if layer.in_dim != cin:
                    raise ValueError("%s has %d rows, its input %s %d columns" % (spec.kernel, layer.in_dim, what, cin))
                layers.append(layer)
                cin, what = layer.out_dim, spec.kernel
            return layers, cin

        self.key_layers, key_dim = chain(self.key_specs, width(self.key_node), d.get("att_key_input"))
        self.value_layers, value_dim = chain(self.value_specs, width(self.value_node), d.get("att_value_input"))
        if self.query_name not in weights:
            raise KeyError("the checkpoint lacks %s" % self.query_name)
        pool = AttPool(weights[self.query_name], key_dim, value_dim, d.get("att_split_key"), d.get("att_split_value"),
                       d.get("att_use_scale"), self.device, num_slots)
        if pool.heads != int(d.get("att_num_heads", 1)):
            raise ValueError("%s has %d rows, att_num_heads is %d" % (self.query_name, pool.heads, int(d.get("att_num_heads", 1))))
        if self.tail.pool_dim != pool.out_dim:
            raise ValueError("%s has %d rows, the attentive pooling gives %d" % (self.tail.specs[0].kernel, self.tail.pool_dim,
                                                                                  pool.out_dim))
        return pool

    def _open(self):
        """Behind StackedTrainer.__init__: the attention's layers join specs and layers, between the frame layers and the tail."""
        self.att_specs = self.key_specs + self.value_specs
        self.att_layers = self.key_layers + self.value_layers
        self.specs = self.frame_specs + self.att_specs + tuple(self.tail.specs)
        self.layers = self.frame_layers + self.att_layers + list(self.tail.layers)
        self.tail._fit_workspace(self.layers)

    def tensors(self):
        """[(TensorFlow name, parameter, gradient, slots)] of everything trained, in the order of trained_names()."""
        return (tail_train.layer_tensors(self.frame_specs, self.frame_layers) + tail_train.layer_tensors(self.att_specs, self.att_layers)
                + [(self.query_name, self.pool.q, self.pool.gq, self.pool.slots)] + self.tail.tensors())

    def variables(self):
        """name -> float32 numpy of every trained variable under its TensorFlow name; in batch mode also the moved statistics."""
        out = tail_train.layer_variables(self.frame_specs, self.frame_layers)
        out.update(tail_train.layer_variables(self.att_specs, self.att_layers))
        out[self.query_name] = self.pool.query()
        out.update(self.tail.variables())
        return out

    def _forward(self, x_dev, offsets, mark=tail_train._no_mark, training=True):
        x, offsets = self._packed(x_dev), self._offsets(offsets)
        mark("start")
        keep = {-1: (x, offsets)}
        self._walk(x, offsets, mark, training, keep)
        mark("frame_forward")
        (key, koff), (value, voff) = keep[self.key_node], keep[self.value_node]
        if self.key_node != self.value_node and not np.array_equal(np.asarray(koff), np.asarray(voff)):
            raise ValueError("the key and the value must have the same number of frames in every utterance")
        for layer in self.key_layers:
            key = tail_train.layer_forward(layer, training, key.contiguous())
        for layer in self.value_layers:
            value = tail_train.layer_forward(layer, training, value.contiguous())
        mark("attention_forward")
        pooled = self.pool.forward(key.contiguous(), value.contiguous(), koff)
        mark("pool_forward")
        y = self.tail._forward(pooled.contiguous(), training)
        mark("segment_forward")
        return y

    def _backward(self, gy, mark):
        torch = self._torch
        g = self.tail._backward(gy, True)
        mark("segment_backward")
        gkey, gvalue = self.pool.backward(g)
        mark("pool_backward")
        for i in range(len(self.key_layers) - 1, -1, -1):
            gkey = self.key_layers[i].backward(gkey.contiguous(), i > 0 or self.key_node >= 0)
        for i in range(len(self.value_layers) - 1, -1, -1):
            gvalue = self.value_layers[i].backward(gvalue.contiguous(), i > 0 or self.value_node >= 0)
        mark("attention_backward")
        att = {}
        if self.key_node >= 0:
            att[self.key_node] = gkey
        if self.value_node >= 0:                                             # both branches on one node: key + value
            att[self.value_node] = torch.add(att[self.value_node], gvalue) if self.value_node in att else gvalue
        g = None
        for i in range(len(self.frame_layers) - 1, -1, -1):
            if i in att:                                                     # the chain's gradient first, then the attention's
                g = att[i] if g is None else torch.add(g, att[i])
            g = self.frame_layers[i].backward(g.contiguous(), i > 0)
            mark("frame_backward/%d" % i)
        mark("frame_backward")


class AttFrameTrainer(_AttStage, frame_train.FrameTrainer):
    """frame_train.FrameTrainer for a self_attention model: the 1-tap frame layers behind the frozen node, the key and value
    networks, the query, the segment-level layers and the head.  forward(frames_dev, offsets), step(frames_dev, offsets, labels,
    learning_rate, global_step=0, mark=None); mark sees "attention_forward" behind "frame_forward" and "attention_backward" behind
    "pool_backward" in addition to StackedTrainer's stages."""

    _check = staticmethod(lambda params, metric=False: check_supported(params, False, metric))
    _l2 = staticmethod(lambda params: l2_assignment(params, False))
    _metric_l2 = staticmethod(lambda params: l2_assignment(params, False, True))

    def __init__(self, params, weights, num_classes, device=0, seed=0, kernel=None, bias=None, batch_norm="moving", metric=False):
        frame_train.FrameTrainer.__init__(self, params, weights, num_classes, device, seed, kernel, bias, batch_norm, metric)
        self._open()


class AttConvTrainer(_AttStage, conv_train.ConvTrainer):
    """conv_train.ConvTrainer for a self_attention model: every frame-level layer on the packed features, the key and value
    networks, the query, the segment-level layers and the head.  forward(feats_dev, offsets), step(feats_dev, offsets, labels,
    learning_rate, global_step=0, mark=None); the marks are AttFrameTrainer's."""

    _check = staticmethod(lambda params, metric=False: check_supported(params, True, metric))
    _l2 = staticmethod(lambda params: l2_assignment(params, True))
    _metric_l2 = staticmethod(lambda params: l2_assignment(params, True, True))

    def __init__(self, params, weights, num_classes, device=0, seed=0, kernel=None, bias=None, batch_norm="moving", metric=False):
        conv_train.ConvTrainer.__init__(self, params, weights, num_classes, device, seed, kernel, bias, batch_norm, metric)
        self._open()
