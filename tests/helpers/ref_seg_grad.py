"""The rule of xv_seg_forward / xv_seg_backward (include/xvec_hip.h) in float64 numpy, the per-element error bound derived in
the header of csrc/seg_grad.hip restated as bounds(), and the replay of one whole training step of the two segment-level layers
and the head (tf_kaldi_speaker_amd/tail_train.py) from float32 parameters: the gradients by the float64 rule (tail_grads), rounded
to float32, the update by ref_loss_grad.opt_step in the kernel's float32 order, and the bound that step carries
(tail_grad_bounds composed stage by stage, then update_bound through the optimizer).

The gradient rule is checked against torch.autograd in float64 (tests/test_seg_grad_host.py)."""
import numpy as np

import ref_loss_grad as rg

U = 2.0 ** -24
EPS = 1e-3
NONE, RELU, LRELU = 0, 1, 2
F = np.float32
SLOPE = float(F(0.2))                      # the kernel multiplies by float32(0.2)


def _bn(bn):
    """bn = None or (gamma, beta, moving_mean, moving_variance) -> float64 arrays or None."""
    return None if bn is None else tuple(np.asarray(v, dtype=np.float64) for v in bn)


def forward(x, w, b, bn=None, act=NONE, slope=0.2):
    """x [n, K], w [N, K] (the rows: the transpose of the TensorFlow kernel), b [N] -> dict(z, h, y, r), float64."""
    x, w, b = (np.asarray(v, dtype=np.float64) for v in (x, w, b))
    z = x @ w.T + b[None, :]
    bn = _bn(bn)
    if bn is None:
        r, h = None, z
    else:
        gamma, beta, mm, mv = bn
        r = 1.0 / np.sqrt(mv + EPS)
        h = (gamma * r)[None, :] * (z - mm[None, :]) + beta[None, :]
    y = h if act == NONE else np.where(h > 0, h, 0.0 if act == RELU else slope * h)
    return dict(x=x, w=w, b=b, bn=bn, act=act, z=z, h=h, y=y, r=r)


def backward(fwd, gy, slope=0.2):
    """-> dict(a, gz, gx [n, K], gw [N, K], gbias, ggamma, gbeta [N]; the last two None without batch norm), float64."""
    gy = np.asarray(gy, dtype=np.float64)
    x, w, bn, act, z, h = fwd["x"], fwd["w"], fwd["bn"], fwd["act"], fwd["z"], fwd["h"]
    if act == NONE:
        a = gy.copy()
    else:
        a = gy * np.where(h > 0, 1.0, 0.0 if act == RELU else slope)        # zero belongs to the lower branch
    if bn is None:
        gz, ggamma, gbeta = a, None, None
    else:
        gamma, _, mm, _ = bn
        r = fwd["r"]
        gbeta = a.sum(axis=0)
        ggamma = (a * (r[None, :] * (z - mm[None, :]))).sum(axis=0)
        gz = a * (gamma * r)[None, :]
    return dict(a=a, gz=gz, gx=gz @ w, gw=gz.T @ x, gbias=gz.sum(axis=0), ggamma=ggamma, gbeta=gbeta, gy=gy)


def bounds(fwd, bwd=None):
    """The header of csrc/seg_grad.hip -> dict of per-element bounds: z, h, y, and with `bwd` gx, gw, gbias, ggamma, gbeta."""
    x, w, b, bn, act = fwd["x"], fwd["w"], fwd["b"], fwd["bn"], fwd["act"]
    n, K = x.shape
    N = w.shape[0]
    t = 2.0 ** -53 * (n + 64)
    bz = (K + 2) * U * (np.abs(x) @ np.abs(w).T + np.abs(b)[None, :])
    if bn is None:
        bh, sr, dev = bz, None, None
    else:
        gamma, _, mm, _ = bn
        sr = np.abs(gamma * fwd["r"])[None, :]
        dev = fwd["r"][None, :] * (fwd["z"] - mm[None, :])                # r (z - mm)
        bh = 1.01 * sr * bz + 4.0 * U * np.abs(gamma[None, :] * dev) + U * np.abs(fwd["h"])
    out = dict(z=bz, h=bh, y=bh + 2.0 * U * np.abs(fwd["y"]))
    if bwd is None:
        return out
    a, gz = np.abs(bwd["a"]), np.abs(bwd["gz"])
    ba = 2.0 * U * a if act == LRELU else np.zeros_like(a)
    bg = ba if bn is None else sr * ba + 3.01 * U * gz
    if bn is not None:
        out["gbeta"] = ba.sum(axis=0) + (U + t) * a.sum(axis=0)
        out["ggamma"] = ((ba * np.abs(dev) + a * np.abs(fwd["r"])[None, :] * bz).sum(axis=0)
                         + (2.0 * U + t) * (a * np.abs(dev)).sum(axis=0))
    out["gbias"] = bg.sum(axis=0) + (U + t) * gz.sum(axis=0)
    out["gw"] = bg.T @ np.abs(x) + (n + 32) * U * (gz.T @ np.abs(x))
    out["gx"] = bg @ np.abs(w) + (N + 2) * U * (gz @ np.abs(w))
    return out


# ---------------------------------------------------------------------------------------------- one training step
class Layer(object):
    """One layer's float32 state for the replay: w [N, K] rows, b, bn (gamma, beta, mm, mv) or None, act."""

    def __init__(self, w, b, bn, act):
        self.w, self.b = np.asarray(w, dtype=F).copy(), np.asarray(b, dtype=F).copy()
        self.bn = None if bn is None else [np.asarray(v, dtype=F).copy() for v in bn]
        self.act = act


def tail_grads(layers, head_w, head_b, pooled, labels, head="softmax", margin=0.0, fa=0.0):
    """The float64 rule of one step at the given (float32) parameters: both layers forward, the head's loss and gradients
    (ref_loss_grad.classifier_grad, the mean loss), both layers backward -> (fwd1, fwd2, head result, bwd1, bwd2)."""
    l1, l2 = layers
    f1 = forward(pooled, l1.w, l1.b, l1.bn, l1.act, SLOPE)
    f2 = forward(f1["y"], l2.w, l2.b, l2.bn, l2.act, SLOPE)
    hd = rg.classifier_grad(f2["y"], labels, np.asarray(head_w, dtype=np.float64), head_b, head, margin, fa)
    b2 = backward(f2, hd["grad_x"], SLOPE)
    b1 = backward(f1, b2["gx"], SLOPE)
    return f1, f2, hd, b1, b2


def tail_grad_bounds(f1, f2, hd, b1, b2, embed_dim, num_classes):
    """How far a float32 evaluation of the step (the kernels, or any other summation order of the same lengths) may lie from
    tail_grads, per element, to first order: every stage's own bound (bounds(), ref_loss_grad.bounds) plus what the stage in
    front of it hands on, carried through the exact linear maps of the oracle.  -> (layer 1 dict, layer 2 dict, head kernel
    [E, C], head bias [C]); the dicts hold w, b, gamma, beta."""
    n = f1["x"].shape[0]
    e1 = bounds(f1, b1)
    # the input of layer 2 is off by e1[y]: z2 moves by |w2| e1[y], on top of its own bound
    e2 = bounds(f2, b2)
    in2 = e1["y"] @ np.abs(f2["w"]).T
    sr2 = 1.0 if f2["bn"] is None else np.abs(f2["bn"][0] * f2["r"])[None, :]
    y2 = e2["y"] + sr2 * in2
    # the head (plain softmax): its own bounds plus its Jacobian on y2.  Logits off by dz_ic <= sum_e y2_ie |w_ec| move
    # p_ic = softmax by |dp_ic| = p_ic |dz_ic - sum_c' p_ic' dz_ic'| <= 2 p_ic max_c |dz_ic|, and G = s (p - [c = l])
    assert hd["q"] is None, "the composed bound is written for the plain softmax head"
    bx, bk, bb = rg.bounds(hd, embed_dim, num_classes)
    wh = np.abs(hd["wh"])
    du = np.max(y2 @ wh, axis=1)                                        # max_c |dz_ic|
    dG = 2.0 * np.abs(hd["G"]) * du[:, None]
    lab = hd["labels"]
    dG[np.arange(n), lab] = 2.0 * abs(hd["scale"]) * hd["p_label"] * du
    hk = bk + np.abs(hd["x"]).T @ dG + y2.T @ np.abs(hd["G"])
    hb = bb + dG.sum(axis=0)
    gy2 = bx + dG @ wh.T
    # layer 2 backward on gy2 (and on z2 moved by in2: the masks hold by the cases' precondition, r (z - mm) moves by r in2)
    out2 = _carry(f2, b2, e2, gy2, in2, e1["y"])
    gy1 = out2.pop("gx_total")
    out1 = _carry(f1, b1, e1, gy1, np.zeros_like(f1["z"]), np.zeros_like(f1["x"]))
    out1.pop("gx_total")
    return out1, out2, hk, hb


def _carry(fwd, bwd, own, dgy, dz_in, dx_in):
    """A layer's own backward bounds plus what an input gradient off by dgy, a z off by dz_in and an x off by dx_in add."""
    bn, act = fwd["bn"], fwd["act"]
    slope = np.ones_like(fwd["h"]) if act == NONE else np.where(fwd["h"] > 0, 1.0, 0.0 if act == RELU else SLOPE)
    da = dgy * slope
    a, gz = np.abs(bwd["a"]), np.abs(bwd["gz"])
    out = {}
    if bn is None:
        dgz = da
    else:
        sr = np.abs(bn[0] * fwd["r"])[None, :]
        r = np.abs(fwd["r"])[None, :]
        dev = np.abs(fwd["r"][None, :] * (fwd["z"] - bn[2][None, :]))
        dgz = da * sr
        out["beta"] = own["gbeta"] + da.sum(axis=0)
        out["gamma"] = own["ggamma"] + (da * dev + a * r * dz_in).sum(axis=0)
    out["b"] = own["gbias"] + dgz.sum(axis=0)
    out["w"] = own["gw"] + dgz.T @ np.abs(fwd["x"]) + gz.T @ dx_in
    out["gx_total"] = own["gx"] + dgz @ np.abs(fwd["w"])
    return out


def update_bound(kind, g, dg, slot0, slot1, lr, clip_norm, momentum, nesterov, step, w, l2):
    """How far two runs of xv_opt_step's float32 rule (ref_loss_grad.opt_step) lie apart when they start from the same w and
    slots and their gradients differ by at most dg per element: the rule's derivative with respect to g, times 1.01 for the
    second order, plus 4 u (|w| + |update|) for roundings that fall differently.  g is the oracle's gradient (float64)."""
    g = np.asarray(g, dtype=np.float64) + float(F(l2)) * np.asarray(w, dtype=np.float64)
    dg = np.asarray(dg, dtype=np.float64)
    if clip_norm > 0:
        norm = np.sqrt(np.sum(g * g))
        dn = np.sqrt(np.sum(dg * dg))
        den = max(norm - dn, clip_norm)
        dg = clip_norm / den * (dg + np.abs(g) * dn / den)
        g = g * clip_norm / max(norm, clip_norm)
    lr = float(F(lr))
    if kind == rg.SGD:
        upd, dupd = lr * np.abs(g), lr * dg
    elif kind == rg.MOMENTUM:
        m = float(F(momentum))
        acc = m * np.asarray(slot0, dtype=np.float64) + g
        if nesterov:
            upd, dupd = lr * np.abs(g + m * acc), lr * (1.0 + m) * dg
        else:
            upd, dupd = lr * np.abs(acc), lr * dg
    else:
        lrt = float(rg.adam_lr(lr, step))
        m1 = 0.9 * np.asarray(slot0, dtype=np.float64) + 0.1 * g
        v1 = 0.999 * np.asarray(slot1, dtype=np.float64) + 0.001 * g * g
        dm = 0.1 * dg
        dv = 0.001 * (2.0 * np.abs(g) + dg) * dg
        lo = np.sqrt(np.maximum(v1 - dv, 0.0))
        dsq = np.sqrt(v1 + dv) - lo                                    # sqrt is monotone: the widest the root can move
        den = lo + 1e-8
        upd = lrt * np.abs(m1) / (np.sqrt(v1) + 1e-8)
        dupd = lrt * (dm / den + (np.abs(m1) + dm) * dsq / (den * den))
    return 1.01 * dupd + 4.0 * U * (np.abs(np.asarray(w, dtype=np.float64)) + upd)


def f32(a):
    return np.asarray(a, dtype=F)
