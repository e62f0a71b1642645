"""The metric-learning losses of the reference as validation losses on the GPU (csrc/metric_loss.hip through the C ABI:
xv_metric_loss_workspace / xv_metric_loss): model/loss.py:387-527 `semihard_triplet_loss`, :530-663 `angular_triplet_loss`
("all" and "hard") and :666-734 `e2e_valid_loss`, the softmax generalized end-to-end loss with scale 20 that
Trainer.save_and_set_valid_loss (model/trainer.py:424-427) puts in place of the angular triplet loss.  Everything is evaluated in
double from float32 rows; the rules are stated in include/xvec_hip.h and pinned to the reference's numpy twins.

A call takes one batch, or many with `offsets` ([G + 1] row offsets): every batch (group) is evaluated on its own, all of them
in one launch sequence, and `loss` is the mean of the group losses.  Arrays go in as numpy or as float32 device tensors, like
losses.py.  MetricHead.loss_and_grad adds the gradient of the two triplet losses (csrc/metric_loss_grad.hip, xv_metric_loss_grad:
what fine-tuning needs; the rule and its choices are in include/xvec_hip.h).  `generalized_angular_triplet_loss` and the `ge2e`
loss with learnable w, b are not implemented.  No CPU path: without a HIP device the loss functions raise RuntimeError;
from_params and MetricHead's constructor are pure host code."""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr
from .losses import _HEADS, _dict, _f32

MAX_GROUP_ROWS = 4096
MAX_SLOTS = 512           # groups (or panels of groups over 1024 rows) in flight; the result does not depend on it
MAX_GRAD_ROWS = 1024      # the gradient keeps a group's panel and counts in LDS
MAX_GRAD_SLOT_BYTES = 1 << 28

MetricResult = collections.namedtuple("MetricResult", "loss rows counts top1 group_loss group_counts")
MetricGrad = collections.namedtuple("MetricGrad", MetricResult._fields + ("grad_x",))

_KINDS = {"semihard": _lib.XV_METRIC_SEMIHARD, "all": _lib.XV_METRIC_ANGULAR_ALL, "hard": _lib.XV_METRIC_ANGULAR_HARD,
          "softmax": _lib.XV_METRIC_GE2E_SOFTMAX, "contrastive": _lib.XV_METRIC_GE2E_CONTRASTIVE}
_ANGULAR_HEADS = {k: v for k, v in _HEADS.items() if k != "softmax"}


def _need_device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: the metric losses have no CPU fallback")
    return torch


def _check_groups(x, labels, offsets):
    """Host-side argument checks -> (rows, dim, offsets int64 [G + 1])."""
    if len(tuple(x.shape)) != 2 or int(x.shape[1]) < 1:
        raise ValueError("x: expected [n, d], got shape %s" % (tuple(x.shape),))
    n = int(x.shape[0])
    if int(np.prod(tuple(labels.shape))) != n:
        raise ValueError("labels: %d labels for %d rows" % (int(np.prod(tuple(labels.shape))), n))
    off = np.asarray([0, n] if offsets is None else offsets, dtype=np.int64).reshape(-1)
    if len(off) < 2 or off[0] != 0 or off[-1] != n or np.any(np.diff(off) < 1):
        raise ValueError("offsets: expected ascending row offsets from 0 to %d with no empty group, got %s" % (n, off.tolist()))
    if np.diff(off).max() > MAX_GROUP_ROWS:
        raise ValueError("a group of %d rows: at most %d" % (int(np.diff(off).max()), MAX_GROUP_ROWS))
    return n, int(x.shape[1]), off


def _run(x, labels, offsets, kind, pos_head=0, margin=0.0, squared=False, normalize=True, w=0.0, b=0.0, device=0, as_tensor=False):
    n, d, off = _check_groups(x, labels, offsets)
    host_labels = (labels.detach().cpu().numpy() if hasattr(labels, "detach") else np.asarray(labels)).reshape(-1)
    single = np.minimum.reduceat(host_labels, off[:-1]) == np.maximum.reduceat(host_labels, off[:-1])
    if single.any():
        raise ValueError("group %d has fewer than two distinct labels: no triplet and no other class" % int(np.argmax(single)))
    torch = _need_device()
    lib = _lib.load()
    device = int(device)
    with torch.cuda.device(device):
        xd = _f32(x, device, torch)
        if isinstance(labels, torch.Tensor):
            ld = labels.to(device=xd.device, dtype=torch.int32).contiguous().reshape(-1)
        else:
            ld = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)).to(xd.device)
        groups = len(off) - 1
        ge2e = kind in (_lib.XV_METRIC_GE2E_SOFTMAX, _lib.XV_METRIC_GE2E_CONTRASTIVE)
        need = int(lib.xv_metric_loss_workspace(groups, off.ctypes.data_as(C.c_void_p), d, kind))
        if need < 0:
            _lib.check(need)
        # one slot is in `need`; every further one lets one more workgroup run at a time
        slot = int(lib.xv_metric_loss_slot_bytes(int(np.diff(off).max()), d, kind))
        extra = min(groups if ge2e else int(np.sum((np.diff(off) + 15) // 16)), MAX_SLOTS) - 1 if slot else 0
        ws = torch.empty(need + slot * extra, dtype=torch.uint8, device=xd.device)
        rows = torch.empty(n, dtype=torch.float64, device=xd.device)
        counts = torch.empty(n, dtype=torch.int64, device=xd.device)
        top1 = torch.empty(n, dtype=torch.int32, device=xd.device) if ge2e else None
        gloss = torch.empty(groups, dtype=torch.float64, device=xd.device)
        gcount = torch.empty((groups, 2), dtype=torch.int64, device=xd.device)
        stream = _lib.stream(device)
        _lib.check(lib.xv_metric_loss(device, ptr(xd), int(xd.shape[1]), off.ctypes.data_as(C.c_void_p), groups, d, ptr(ld), kind,
                                      int(pos_head), float(margin), int(bool(squared)), int(bool(normalize)), float(w), float(b),
                                      ptr(rows), ptr(counts), ptr(top1), ptr(gloss), ptr(gcount), ptr(ws),
                                      ws.numel(), stream))
        gl = gloss.cpu().numpy()
        loss = float(np.mean(gl))
        if as_tensor:
            return MetricResult(loss, rows, counts, top1, gloss, gcount)
        return MetricResult(loss, rows.cpu().numpy(), counts.cpu().numpy(), None if top1 is None else top1.cpu().numpy(), gl,
                            gcount.cpu().numpy())


def semihard_triplet_loss(x, labels, margin=0.2, squared=False, normalize=True, offsets=None, device=0, as_tensor=False):
    """model/loss.py:387-527 (tf.contrib's triplet_semihard_loss on l2-normalised rows).  x [n, d], labels [n] ->
    MetricResult: rows = every anchor's sum of terms, counts = its positive pairs, group_counts = (pairs, 0)."""
    return _run(x, labels, offsets, _lib.XV_METRIC_SEMIHARD, margin=margin, squared=squared, normalize=normalize, device=device,
                as_tensor=as_tensor)


def _angular_head(loss_type, margin):
    if loss_type not in _ANGULAR_HEADS:
        raise ValueError("loss_type %r: one of %s" % (loss_type, ", ".join(sorted(_ANGULAR_HEADS))))
    if loss_type == "asoftmax" and margin not in (1, 2, 4):
        raise NotImplementedError("[ERROR] m=%d is not unsupported." % margin)        # loss.py:168, the reference's wording
    return _ANGULAR_HEADS[loss_type]


def angular_triplet_loss(x, labels, loss_type="additive_margin_softmax", margin=0.2, triplet_type="all", offsets=None, device=0,
                         as_tensor=False):
    """model/loss.py:530-663.  triplet_type "all": rows = sum of max(t, 0), counts = active triplets, group_counts =
    (active, all triplets); "hard": rows = max(hardest negative - hardest positive, 0), group_counts = (rows, 0)."""
    if triplet_type not in ("all", "hard"):
        raise ValueError("triplet_type %r: all or hard" % (triplet_type,))
    head = _angular_head(loss_type, margin)
    return _run(x, labels, offsets, _KINDS[triplet_type], pos_head=head, margin=margin, device=device, as_tensor=as_tensor)


def ge2e_loss(x, labels, w=20.0, b=0.0, ge2e_type="softmax", offsets=None, device=0, as_tensor=False):
    """model/loss.py:666-734 with fixed w, b.  rows = every row's loss, top1 = the label of its most similar class,
    group_counts = (rows, rows whose top1 is their own label)."""
    if ge2e_type not in ("softmax", "contrastive"):
        raise ValueError("ge2e_type %r: softmax or contrastive" % (ge2e_type,))
    return _run(x, labels, offsets, _KINDS[ge2e_type], w=w, b=b, device=device, as_tensor=as_tensor)


def e2e_valid_loss(x, labels, offsets=None, device=0, as_tensor=False):
    """model/loss.py:666-734 as validation calls it: the softmax form with w = 20, b = 0."""
    return ge2e_loss(x, labels, 20.0, 0.0, "softmax", offsets, device, as_tensor)


def from_params(params, validation=True, device=0):
    """The switch of model/trainer.py:113-129 and :407-436 -> callable(x, labels, offsets=None) -> MetricResult.
    `semihard_triplet_loss` evaluates itself with params.margin and params.triplet_loss_squared; `angular_triplet_loss` is
    evaluated as e2e_valid_loss in validation (save_and_set_valid_loss) and by its own parameters otherwise;
    `generalized_angular_triplet_loss` and `ge2e` are refused, as is everything losses.py owns."""
    d = _dict(params)
    func = d.get("loss_func")
    if func == "semihard_triplet_loss":
        margin, squared = float(d["margin"]), bool(d["triplet_loss_squared"])
        return lambda x, labels, offsets=None: semihard_triplet_loss(x, labels, margin, squared, True, offsets, device)
    if func == "angular_triplet_loss":
        if validation:
            return lambda x, labels, offsets=None: e2e_valid_loss(x, labels, offsets, device)
        loss_type, triplet_type = d["loss_type"], d["triplet_type"]
        if loss_type not in _ANGULAR_HEADS:
            raise ValueError("loss_type %r: one of %s" % (loss_type, ", ".join(sorted(_ANGULAR_HEADS))))
        margin = float(d["margin"])                                                # loss.py:549
        if loss_type == "asoftmax" and margin == int(margin):
            margin = int(margin)
        _angular_head(loss_type, margin)
        return lambda x, labels, offsets=None: angular_triplet_loss(x, labels, loss_type, margin, triplet_type, offsets, device)
    if func in ("generalized_angular_triplet_loss", "ge2e"):
        raise NotImplementedError("loss_func %r is not implemented (semihard_triplet_loss and angular_triplet_loss are)" % func)
    if func in _HEADS:
        raise NotImplementedError("loss_func %r is a classifier head: losses.ClassifierHead evaluates it" % func)
    raise NotImplementedError("Not implement %s loss" % func)                     # trainer.py:129


def _run_grad(x, labels, offsets, kind, pos_head, margin, squared, normalize, grad_scale, device, as_tensor, sync=True):
    if not hasattr(labels, "shape"):
        labels = np.asarray(labels)
    n, d, off = _check_groups(x, labels, offsets)
    if np.diff(off).max() > MAX_GRAD_ROWS:
        raise ValueError("a group of %d rows: the gradient takes at most %d" % (int(np.diff(off).max()), MAX_GRAD_ROWS))
    if not np.isfinite(grad_scale):
        raise ValueError("grad_scale must be finite, got %r" % (grad_scale,))
    torch = _need_device()
    lib = _lib.load()
    device = int(device)
    with torch.cuda.device(device):
        xd = _f32(x, device, torch)
        if isinstance(labels, torch.Tensor):
            ld = labels.to(device=xd.device, dtype=torch.int32).contiguous().reshape(-1)
        else:
            ld = torch.from_numpy(np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)).to(xd.device)
        groups = len(off) - 1
        need = int(lib.xv_metric_loss_grad_workspace(groups, off.ctypes.data_as(C.c_void_p), d, kind))
        if need < 0:
            _lib.check(need)
        # one slot (dL/dM [B, B] and its product with the rows [B, d]) is in `need`; every further one lets one more group run
        b = int(np.diff(off).max())
        slot = (8 * b * (b + d) + 255) // 256 * 256
        extra = max(min(groups, 64, MAX_GRAD_SLOT_BYTES // slot) - 1, 0)
        ws = torch.empty(need + slot * extra, dtype=torch.uint8, device=xd.device)
        rows = torch.empty(n, dtype=torch.float64, device=xd.device)
        counts = torch.empty(n, dtype=torch.int64, device=xd.device)
        gloss = torch.empty(groups, dtype=torch.float64, device=xd.device)
        gcount = torch.empty((groups, 2), dtype=torch.int64, device=xd.device)
        gx = torch.empty((n, d), dtype=torch.float32, device=xd.device)
        _lib.check(lib.xv_metric_loss_grad(device, ptr(xd), int(xd.shape[1]), off.ctypes.data_as(C.c_void_p), groups, d, ptr(ld),
                                           kind, int(pos_head), float(margin), int(bool(squared)), int(bool(normalize)),
                                           float(grad_scale), ptr(rows), ptr(counts), ptr(gloss), ptr(gcount), ptr(gx), d, ptr(ws),
                                           ws.numel(), _lib.stream(device)))
        if as_tensor and not sync:                                   # a trainer's step: nothing is read back here
            return MetricGrad(None, rows, counts, None, gloss, gcount, gx)
        gl = gloss.cpu().numpy()
        loss = float(np.mean(gl))
        if as_tensor:
            return MetricGrad(loss, rows, counts, None, gloss, gcount, gx)
        return MetricGrad(loss, rows.cpu().numpy(), counts.cpu().numpy(), None, gl, gcount.cpu().numpy(), gx.cpu().numpy())


class MetricHead:
    """The training side of the switch of model/trainer.py:113-129 for the two triplet losses: the options from_params(params,
    validation=False) takes (`normalize` for the semi-hard loss, params.margin, triplet_loss_squared, loss_type, triplet_type).
    loss_and_grad(x, labels, offsets=None, grad_scale=1.0) -> MetricGrad: MetricResult's fields, bit for bit those of the
    forward functions, and grad_x [n, d] = float32(grad_scale dL_g / dx) for the loss L_g of each row's group."""

    def __init__(self, params, device=0):
        d = _dict(params)
        self.loss_func = d.get("loss_func")
        self.forward = from_params(params, validation=False, device=device)      # refuses what has no triplet head
        self.device = device
        self.margin = float(d["margin"])
        self.squared, self.normalize, self.pos_head = False, True, 0
        if self.loss_func == "semihard_triplet_loss":
            self.kind, self.squared = _lib.XV_METRIC_SEMIHARD, bool(d["triplet_loss_squared"])
        else:
            if d["triplet_type"] not in ("all", "hard"):
                raise ValueError("triplet_type %r: all or hard" % (d["triplet_type"],))
            self.kind, self.pos_head = _KINDS[d["triplet_type"]], _ANGULAR_HEADS[d["loss_type"]]

    def loss(self, x, labels, offsets=None):
        return self.forward(x, labels, offsets)

    def loss_and_grad(self, x, labels, offsets=None, grad_scale=1.0, as_tensor=False, sync=True):
        """as_tensor: the arrays stay device tensors; with sync=False as well the call only enqueues and `loss` is None (read
        group_loss when it is needed)."""
        return _run_grad(x, labels, offsets, self.kind, self.pos_head, self.margin, self.squared, self.normalize, grad_scale,
                         self.device, as_tensor, sync)
