"""Float64 restatement of the four classifier heads of the reference as TensorFlow evaluates them (model/loss.py:9-48 softmax,
:80-198 asoftmax, :201-286 additive_margin_softmax, :289-384 additive_angular_margin_softmax), each followed by
tf.losses.sparse_softmax_cross_entropy: loss_i = logsumexp_c(z_ic) - z_i,label, here with an explicit log-sum-exp.

This is the oracle of the GPU tests; it is itself pinned to the reference's numpy twins (model/test_utils.py:157-318) through
the fixtures tests/golden/loss_*.npz (tests/test_loss_host.py).  It also restates the error bound derived in the header of
csrc/loss.hip, so that the tests compute their tolerance from the formula."""
import math

import numpy as np

U = 2.0 ** -24

HEADS = ("softmax", "asoftmax", "additive_margin_softmax", "additive_angular_margin_softmax")


def annealing_fa(lambda_min, lambda_base, lambda_gamma, lambda_power, step):
    """fa = 1 / (1 + lambda), lambda = max(lambda_min, lambda_base (1 + gamma step)^-power) (model/loss.py:173-176)."""
    lamb = max(float(lambda_min), float(lambda_base) * (1.0 + float(lambda_gamma) * float(step)) ** (-float(lambda_power)))
    return 1.0 / (1.0 + lamb)


def l2_scaling(x, s):
    """model/common.py:45-58."""
    x = np.asarray(x, dtype=np.float64)
    return s * x / np.sqrt(np.maximum(np.sum(x * x, axis=1, keepdims=True), 1e-12))


def phi(head, c, margin):
    """The margin function of the clipped target cosine, and its derivative (for the conditioning of the target logit)."""
    c = np.asarray(c, dtype=np.float64)
    if head == "asoftmax":
        m = int(margin)
        if m == 1:
            return c.copy(), np.ones_like(c)
        s0 = np.sign(c)
        c2 = c * c
        if m == 2:
            return 2.0 * s0 * c2 - 1.0, 4.0 * np.abs(c)
        if m != 4:
            raise NotImplementedError("[ERROR] m=%d is not unsupported." % m)
        s3 = np.sign(2.0 * c2 - 1.0) * s0
        s4 = 2.0 * s0 + s3 - 3.0
        return s3 * (8.0 * c2 * c2 - 8.0 * c2 + 1.0) + s4, np.abs(32.0 * c2 * c - 16.0 * c)
    if head == "additive_margin_softmax":
        return c - margin, np.ones_like(c)
    if head == "additive_angular_margin_softmax":
        sn = np.sqrt(np.maximum(1.0 - c * c, 1e-12))
        cpm = c * math.cos(margin) - sn * math.sin(margin)
        return np.where(c > math.cos(math.pi - margin), cpm, -cpm - 2.0), np.abs(math.cos(margin) + c / sn * math.sin(margin))
    raise ValueError(head)


def classifier_loss(x, labels, kernel, bias=None, head="softmax", margin=0.0, fa=0.0):
    """-> dict of float64 arrays: loss, target_logit (after the margin), lse, top1 (argmax of the logits before the margin), and
    for the bound: xnorm, wnorm_max (of the rows the product runs over), bias_abs_max, lipschitz (max(1, fs + fa |phi'|))."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(kernel, dtype=np.float64)
    labels = np.asarray(labels).astype(np.int64)
    n = x.shape[0]
    rows = np.arange(n)
    xnorm = np.sqrt(np.sum(x * x, axis=1))
    lips = np.ones(n)
    if head == "softmax":
        z = x @ w
        if bias is not None:
            z = z + np.asarray(bias, dtype=np.float64)[None, :]
        upd = z
        wn = np.sqrt(np.sum(w * w, axis=0)).max()
    else:
        assert bias is None
        wh = w / np.sqrt(np.maximum(np.sum(w * w, axis=0, keepdims=True), 1e-12))      # tf.nn.l2_normalize(w, dim=0)
        z = x @ wh
        wn = np.sqrt(np.sum(wh * wh, axis=0)).max()
        upd = z
        if not (head == "asoftmax" and int(margin) == 1):
            if head == "asoftmax" and int(margin) not in (2, 4):
                raise NotImplementedError("[ERROR] m=%d is not unsupported." % int(margin))
            sel = z[rows, labels]
            fn = np.maximum(xnorm, 1e-12)
            c = np.clip(sel / fn, -1.0 + 1e-12, 1.0 - 1e-12)
            p, dp = phi(head, c, margin)
            fs = 1.0 - fa
            upd = z.copy()
            upd[rows, labels] = fs * sel + fa * (p * fn)       # fs logits + fa (logits + scatter(scaled - sel))
            lips = np.maximum(1.0, fs + fa * dp)
    mx = upd.max(axis=1)
    lse = mx + np.log(np.sum(np.exp(upd - mx[:, None]), axis=1))
    tgt = upd[rows, labels]
    return dict(loss=lse - tgt, target_logit=tgt, lse=lse, top1=np.argmax(z, axis=1), xnorm=xnorm, wnorm_max=float(wn),
                bias_abs_max=0.0 if bias is None else float(np.abs(bias).max()), lipschitz=lips)


def bound_k(num_classes):
    """k(C) of csrc/loss.hip: 30 + ceil(ceil(C / 128) / 64) + 4 ceil(ln C)."""
    tiles = -(-int(num_classes) // 128)
    return 30 + -(-tiles // 64) + 4 * int(math.ceil(math.log(num_classes)))


def bounds(ref, embed_dim, num_classes):
    """Per-row bounds of csrc/loss.hip from a classifier_loss() result -> (target, lse, loss)."""
    logit = (embed_dim + 8) * U * ref["xnorm"] * ref["wnorm_max"] + ref["bias_abs_max"] * U
    target = ref["lipschitz"] * logit
    lse = np.maximum(logit, target) + bound_k(num_classes) * U * (1.0 + np.abs(ref["lse"]))
    return target, lse, target + lse
