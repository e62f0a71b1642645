"""The classifier heads of the reference as validation losses on the GPU (csrc/loss.hip through the C ABI:
xv_loss_prepare_classes / xv_loss_workspace / xv_loss_classifier): model/loss.py:9-48 `softmax`, :80-198 `asoftmax`,
:201-286 `additive_margin_softmax`, :289-384 `additive_angular_margin_softmax`, each followed by
tf.losses.sparse_softmax_cross_entropy.  Per row: the loss, the target logit after the margin, the log-sum-exp and the top-1
class (the argmax of the logits before the margin, model/trainer.py:1097); the [n, C] logit matrix is never written.

The annealing weight lambda = max(lambda_min, lambda_base (1 + gamma step)^-power) (loss.py:173-176) is evaluated here in
double and reaches the kernel as fa = 1 / (1 + lambda).  ClassifierHead.loss_and_grad adds the gradients with respect to x, the
kernel and the bias (csrc/loss_grad.hip, xv_loss_classifier_grad); gradients through the encoder, the auxiliary losses
(`aux_loss_func`), the triplet and end-to-end losses are not implemented.  Arrays go in as numpy or as float32 device tensors,
like scoring.py.  No CPU path: without a HIP device classifier_loss and ClassifierHead raise RuntimeError; head_config and
valid_params are pure host code."""
import collections
import copy

import numpy as np

from . import _lib
from ._lib import ptr

SOFTMAX_KERNEL = "softmax/output/kernel"      # [E, num_speakers] (loss.py:30-34, 129)
SOFTMAX_BIAS = "softmax/output/bias"          # [num_speakers], the plain softmax only (tf.layers.dense)

_HEADS = {"softmax": _lib.XV_LOSS_SOFTMAX, "asoftmax": _lib.XV_LOSS_ASOFTMAX,
          "additive_margin_softmax": _lib.XV_LOSS_AMSOFTMAX, "additive_angular_margin_softmax": _lib.XV_LOSS_ARCSOFTMAX}
_PREFIX = {"asoftmax": "asoftmax", "additive_margin_softmax": "amsoftmax", "additive_angular_margin_softmax": "arcsoftmax"}
# model/trainer.py:113-129: the other loss networks, refused by name
_OTHER_LOSSES = ("ge2e", "semihard_triplet_loss", "angular_triplet_loss", "e2e_valid_loss", "generalized_angular_triplet_loss")

LossResult = collections.namedtuple("LossResult", "loss target_logit lse top1 mean")
GradResult = collections.namedtuple("GradResult", "loss target_logit lse top1 mean grad_x grad_kernel grad_bias")


def _dict(params):
    return params if isinstance(params, dict) else params.dict


def valid_params(params):
    """Trainer.save_and_set_valid_loss (model/trainer.py:407-436) on a COPY: asoftmax_m = 1, amsoftmax_m = 0, arcsoftmax_m = 0
    for the head in use and no auxiliary losses.  The caller's params are left as they are (the reference patches them in
    place and restores them afterwards, :438-454)."""
    p = copy.deepcopy(params)
    d = _dict(p)
    func = d.get("loss_func")
    if func == "asoftmax":
        d["asoftmax_m"] = 1
    elif func == "additive_margin_softmax":
        d["amsoftmax_m"] = 0
    elif func == "additive_angular_margin_softmax":
        d["arcsoftmax_m"] = 0
    if "aux_loss_func" in d:
        d["aux_loss_func"] = []
    return p


def annealing_fa(lambda_min, lambda_base, lambda_gamma, lambda_power, global_step):
    lamb = max(float(lambda_min), float(lambda_base) * (1.0 + float(lambda_gamma) * float(global_step)) ** (-float(lambda_power)))
    return 1.0 / (1.0 + lamb)


def head_config(params, global_step=0, validation=False):
    """-> (loss_func, head id, margin, fa) for xv_loss_classifier.  NotImplementedError for a loss outside the softmax family,
    for `aux_loss_func` outside validation and for an asoftmax m other than 1, 2, 4 (loss.py:168)."""
    if validation:
        params = valid_params(params)
    d = _dict(params)
    func = d.get("loss_func")
    if func not in _HEADS:
        if func in _OTHER_LOSSES:
            raise NotImplementedError("loss_func %r: only the softmax family is evaluated here (%s)" % (func, ", ".join(sorted(_HEADS))))
        raise NotImplementedError("Not implement %s loss" % func)                     # trainer.py:129
    if d.get("aux_loss_func"):
        raise NotImplementedError("aux_loss_func %r: auxiliary losses are not implemented" % (d["aux_loss_func"],))
    if func == "softmax":
        return func, _HEADS[func], 0.0, 0.0
    pre = _PREFIX[func]
    margin = d[pre + "_m"]
    if func == "asoftmax":
        if margin not in (1, 2, 4):
            raise NotImplementedError("[ERROR] m=%d is not unsupported." % margin)   # loss.py:168, the reference's wording
        if margin == 1:
            return func, _HEADS[func], 1.0, 0.0                                       # loss.py:139-144: no annealing
    fa = annealing_fa(d[pre + "_lambda_min"], d[pre + "_lambda_base"], d[pre + "_lambda_gamma"], d[pre + "_lambda_power"],
                      global_step)
    return func, _HEADS[func], float(margin), fa


def _need_device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: the loss heads have no CPU fallback")
    return torch


def _f32(x, device, torch):
    if isinstance(x, torch.Tensor):
        return x.to(device="cuda:%d" % device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda:%d" % device)


def _labels_dev(labels, n, dev, torch):
    if isinstance(labels, torch.Tensor):
        ld = labels.to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
    else:
        ld = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)).to(dev)
    if ld.shape[0] != n:
        raise ValueError("labels: %d labels for %d rows" % (ld.shape[0], n))
    return ld


class ClassifierHead(object):
    """`softmax/output/kernel` [E, C] (and bias [C]) prepared once on the device: class rows [C, E], column-normalised for the
    angular heads, raw for softmax.  loss(x, labels) then runs any number of batches against them.  `raw_rows` gives the rows
    without the normalisation: loss_and_grad differentiates with respect to them."""

    def __init__(self, kernel, bias=None, params=None, device=0):
        func = _dict(params).get("loss_func")
        if func not in _HEADS:
            head_config(params)                                 # raises with the right message
        if len(tuple(kernel.shape)) != 2:
            raise ValueError("kernel: expected [E, C], got shape %s" % (tuple(kernel.shape),))
        self.embed_dim, self.num_classes = int(kernel.shape[0]), int(kernel.shape[1])
        if self.num_classes < 1 or self.embed_dim < 1:
            raise ValueError("kernel: empty")
        if bias is not None and func != "softmax":
            bias = None                                         # the angular heads create no bias (loss.py:129)
        if bias is not None and tuple(bias.shape) != (self.num_classes,):
            raise ValueError("bias: shape %s for %d classes" % (tuple(bias.shape), self.num_classes))
        torch = _need_device()
        lib = _lib.load()
        self.params, self.device, self.loss_func = params, int(device), func
        self._ldc = (self.embed_dim + 3) // 4 * 4               # 16-byte rows: the tile loader takes float4
        with torch.cuda.device(self.device):
            kd = _f32(kernel, self.device, torch)
            self.classes = torch.zeros((self.num_classes, self._ldc), dtype=torch.float32, device=kd.device)
            stream = _lib.stream(self.device)
            _lib.check(lib.xv_loss_prepare_classes(self.device, ptr(kd), self.num_classes, self.embed_dim, self.num_classes,
                                                   int(func != "softmax"), ptr(self.classes), self._ldc, stream))
            self.bias = None if bias is None else _f32(bias, self.device, torch)
        self._ws = None
        self._gws = None
        self._raw_rows = None
        self._kernel_src = None if func == "softmax" else kernel        # a reference, no copy: the raw rows are made on first need

    @property
    def raw_rows(self):
        """The class rows [C, ldc] WITHOUT the normalisation: what loss_and_grad differentiates with respect to.  For softmax
        these are `classes` themselves (no second tensor); for the angular heads they are made from the kernel on first use, so
        a head that only validates allocates nothing more than before.  A caller that updates them in place (HeadTrainer) leaves
        `classes` of an angular head, and with it loss(), at the old kernel."""
        if self._raw_rows is None:
            if self.loss_func == "softmax":
                self._raw_rows = self.classes
            else:
                torch = _need_device()
                lib = _lib.load()
                with torch.cuda.device(self.device):
                    kd = _f32(self._kernel_src, self.device, torch)
                    rows = torch.zeros((self.num_classes, self._ldc), dtype=torch.float32, device=kd.device)
                    stream = _lib.stream(self.device)
                    _lib.check(lib.xv_loss_prepare_classes(self.device, ptr(kd), self.num_classes, self.embed_dim, self.num_classes, 0,
                                                           ptr(rows), self._ldc, stream))
                    torch.cuda.current_stream(self.device).synchronize()      # kd may be a temporary
                self._raw_rows, self._kernel_src = rows, None
        return self._raw_rows

    def loss(self, x, labels, global_step=0, validation=False, as_tensor=False):
        """x [n, E], labels [n] -> LossResult(loss [n], target_logit [n], lse [n], top1 [n], mean).  A label outside
        [0, C) raises XvError(XV_ERR_INVALID)."""
        _, head, margin, fa = head_config(self.params, global_step, validation)
        torch = _need_device()
        lib = _lib.load()
        if len(tuple(x.shape)) != 2 or int(x.shape[1]) != self.embed_dim:
            raise ValueError("x: expected [n, %d], got shape %s" % (self.embed_dim, tuple(x.shape)))
        n = int(x.shape[0])
        with torch.cuda.device(self.device):
            xd = _f32(x, self.device, torch)
            if isinstance(labels, torch.Tensor):
                ld = labels.to(device=xd.device, dtype=torch.int32).contiguous().reshape(-1)
            else:
                ld = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)).to(xd.device)
            if ld.shape[0] != n:
                raise ValueError("labels: %d labels for %d rows" % (ld.shape[0], n))
            out = torch.empty((3, max(n, 1)), dtype=torch.float32, device=xd.device)
            top1 = torch.empty((max(n, 1),), dtype=torch.int32, device=xd.device)
            need = int(lib.xv_loss_workspace(n, self.num_classes))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=xd.device)
            stream = _lib.stream(self.device)
            _lib.check(lib.xv_loss_classifier(self.device, ptr(xd), self.embed_dim, n, self.embed_dim, ptr(ld), ptr(self.classes),
                                              self._ldc, self.num_classes, ptr(self.bias), head,
                                              margin, fa, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(top1), ptr(self._ws),
                                              self._ws.numel(), stream))
            loss, target, lse, top1 = out[0, :n], out[1, :n], out[2, :n], top1[:n]
            if as_tensor:
                return LossResult(loss, target, lse, top1, float(loss.double().mean()) if n else float("nan"))
            loss = loss.cpu().numpy()
            return LossResult(loss, target.cpu().numpy(), lse.cpu().numpy(), top1.cpu().numpy(),
                              float(loss.astype(np.float64).mean()) if n else float("nan"))

    def _grad_device(self, x, labels, global_step, grad_scale, need_grad_x, grad_rows=None, grad_bias=None):
        """One xv_loss_classifier_grad against self.raw_rows -> device tensors (out [3, n], top1 [n], grad_x [n, E] or None,
        grad_rows [C, ldc], grad_bias [C] or None).  grad_rows / grad_bias may be given (they are overwritten)."""
        _, head, margin, fa = head_config(self.params, global_step, False)
        torch = _need_device()
        lib = _lib.load()
        if len(tuple(x.shape)) != 2 or int(x.shape[1]) != self.embed_dim:
            raise ValueError("x: expected [n, %d], got shape %s" % (self.embed_dim, tuple(x.shape)))
        n = int(x.shape[0])
        with torch.cuda.device(self.device):
            xd = _f32(x, self.device, torch)
            ld = _labels_dev(labels, n, xd.device, torch)
            out = torch.empty((3, max(n, 1)), dtype=torch.float32, device=xd.device)
            top1 = torch.empty((max(n, 1),), dtype=torch.int32, device=xd.device)
            gx = torch.empty((max(n, 1), self.embed_dim), dtype=torch.float32, device=xd.device) if need_grad_x else None
            if grad_rows is None:
                grad_rows = torch.zeros((self.num_classes, self._ldc), dtype=torch.float32, device=xd.device)     # zeros: the padding
            if grad_bias is None and self.bias is not None:
                grad_bias = torch.empty((self.num_classes,), dtype=torch.float32, device=xd.device)
            if n == 0:                              # nothing to launch: the gradient of an empty sum
                grad_rows.zero_()
                if grad_bias is not None:
                    grad_bias.zero_()
                return out[:, :0], top1[:0], None if gx is None else gx[:0], grad_rows, grad_bias
            need = int(lib.xv_loss_grad_workspace(n, self.num_classes, self.embed_dim))
            if self._gws is None or self._gws.numel() < need:
                self._gws = torch.empty(need, dtype=torch.uint8, device=xd.device)
            stream = _lib.stream(self.device)
            scale = 1.0 / n if grad_scale is None else float(grad_scale)
            _lib.check(lib.xv_loss_classifier_grad(self.device, ptr(xd), self.embed_dim, n, self.embed_dim, ptr(ld), ptr(self.raw_rows),
                                                   self._ldc, self.num_classes, ptr(self.bias), head,
                                                   margin, fa, scale, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(top1),
                                                   ptr(gx), self.embed_dim, ptr(grad_rows),
                                                   ptr(grad_bias), ptr(self._gws), self._gws.numel(),
                                                   stream))
        return out[:, :n], top1[:n], None if gx is None else gx[:n], grad_rows, grad_bias

    def loss_and_grad(self, x, labels, global_step=0, grad_scale=None, need_grad_x=True, as_tensor=False):
        """x [n, E], labels [n] -> GradResult(loss, target_logit, lse, top1 [n], mean, grad_x [n, E] or None, grad_kernel [E, C],
        grad_bias [C] or None): the training loss of the head (training margins, annealed at `global_step`) and the gradients of
        grad_scale * sum_i loss_i (default 1 / n, the mean) with respect to x, `softmax/output/kernel` and the bias, as TensorFlow
        differentiates model/loss.py (the rule: include/xvec_hip.h, xv_loss_classifier_grad).  The per-row values are the bits
        loss() gives with the same margins."""
        out, top1, gx, grows, gbias = self._grad_device(x, labels, global_step, grad_scale, need_grad_x)
        n = int(out.shape[1])
        gk = grows[:, :self.embed_dim].t()
        mean = float(out[0].double().mean()) if n else float("nan")
        if as_tensor:
            return GradResult(out[0], out[1], out[2], top1, mean, gx, gk.contiguous(), gbias)
        host = lambda t: None if t is None else t.cpu().numpy()                         # noqa: E731
        return GradResult(host(out[0]), host(out[1]), host(out[2]), host(top1), mean, host(gx), host(gk.contiguous()), host(gbias))


def classifier_loss(x, labels, kernel, bias=None, params=None, global_step=0, validation=False, device=0, as_tensor=False):
    """One batch through one head: x [n, E] (the network's `output` endpoint, after l2_scaling when `feature_norm` is set),
    labels [n], kernel [E, C], bias [C] (softmax only) -> LossResult.  `params` names the head (`loss_func`) and holds its
    margin and annealing parameters; with validation=True the margins are those of Trainer.save_and_set_valid_loss
    (valid_params) and `params` itself is not touched.  For many batches against one kernel build a ClassifierHead once."""
    if params is None:
        raise ValueError("params: the loss head is named by params.loss_func")
    return ClassifierHead(kernel, bias, params, device).loss(x, labels, global_step, validation, as_tensor)
