"""The rules of xv_loss_classifier_grad and xv_opt_step (include/xvec_hip.h) in numpy: the gradients in float64, the optimizer
in float32 in the operation order the header states (so that its bits are the kernel's), and the per-element error bound
derived in the header of csrc/loss_grad.hip restated as bounds().

The gradient rule is checked against torch.autograd in float64 on a torch transcription of ref_loss.classifier_loss
(tests/test_loss_grad_host.py)."""
import math

import numpy as np

import ref_loss

U = ref_loss.U
LO, HI = -1.0 + 1e-12, 1.0 - 1e-12


def _phi_d(head, c, margin):
    """phi, the SIGNED phi' and |phi''| at the clipped cosine c."""
    if head == "asoftmax":
        m = int(margin)
        s0 = np.sign(c)
        c2 = c * c
        if m == 2:
            return 2.0 * s0 * c2 - 1.0, 4.0 * np.abs(c), np.full_like(c, 4.0)
        if m != 4:
            raise NotImplementedError("[ERROR] m=%d is not unsupported." % m)
        s3 = np.sign(2.0 * c2 - 1.0) * s0
        s4 = 2.0 * s0 + s3 - 3.0
        return s3 * (8.0 * c2 * c2 - 8.0 * c2 + 1.0) + s4, s3 * (32.0 * c2 * c - 16.0 * c), np.abs(96.0 * c2 - 16.0)
    if head == "additive_margin_softmax":
        return c - margin, np.ones_like(c), np.zeros_like(c)
    if head == "additive_angular_margin_softmax":
        s2 = 1.0 - c * c
        sn = np.sqrt(np.maximum(s2, 1e-12))
        dsn = np.where(s2 > 1e-12, -c / sn, 0.0)
        cpm = c * math.cos(margin) - sn * math.sin(margin)
        dcpm = math.cos(margin) - dsn * math.sin(margin)
        first = c > math.cos(math.pi - margin)
        return np.where(first, cpm, -cpm - 2.0), np.where(first, dcpm, -dcpm), np.abs(math.sin(margin)) / sn ** 3
    raise ValueError(head)


def classifier_grad(x, labels, kernel, bias=None, head="softmax", margin=0.0, fa=0.0, grad_scale=None):
    """-> dict: the per-row outputs of ref_loss.classifier_loss, grad_x [n, E], grad_kernel [E, C] (grad_rows is its transpose),
    grad_bias [C] or None, and what bounds() needs."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(kernel, dtype=np.float64)
    labels = np.asarray(labels).astype(np.int64)
    n, C = x.shape[0], w.shape[1]
    s = (1.0 / n) if grad_scale is None else float(grad_scale)
    rows = np.arange(n)
    fwd = ref_loss.classifier_loss(x, labels, w, bias, head, margin, fa)
    xnorm = fwd["xnorm"]
    plain = head == "softmax" or (head == "asoftmax" and int(margin) == 1) or fa == 0.0
    if head == "softmax":
        wh, q = w, None
        z = x @ w + (0.0 if bias is None else np.asarray(bias, dtype=np.float64)[None, :])
    else:
        q = np.sum(w * w, axis=0)
        wh = w / np.sqrt(np.maximum(q, 1e-12))
        z = x @ wh
    u = z.copy()
    u[rows, labels] = fwd["target_logit"]
    p = np.exp(u - fwd["lse"][:, None])
    G = s * p
    d = s * (p[rows, labels] - 1.0)
    zero = np.zeros(n)
    if plain:
        G[rows, labels] = d
        r = zero
        info = dict(dphi=np.ones(n) * (0.0 if head == "softmax" else 1.0), ddphi=zero, phi=zero, c=zero, fa=0.0)
    else:
        fn = np.maximum(xnorm, 1e-12)
        craw = z[rows, labels] / fn
        inside = ((craw >= LO) & (craw <= HI)).astype(np.float64)
        c = np.clip(craw, LO, HI)
        phi, dphi, ddphi = _phi_d(head, c, margin)
        dphi = dphi * inside
        G[rows, labels] = d * ((1.0 - fa) + fa * dphi)
        r = d * fa * (phi - dphi * craw)
        info = dict(dphi=dphi, ddphi=ddphi * inside, phi=phi, c=craw, fa=fa)
    unit = np.where((xnorm > 1e-12)[:, None], x / np.maximum(xnorm, 1e-300)[:, None], 0.0)
    grad_x = G @ wh.T + r[:, None] * unit
    gw = x.T @ G                                           # [E, C]
    if head == "softmax":
        grad_kernel = gw
    else:
        big = q > 1e-12
        proj = (gw - wh * np.sum(wh * gw, axis=0, keepdims=True)) / np.sqrt(np.maximum(q, 1e-300))
        grad_kernel = np.where(big[None, :], proj, gw / 1e-6)
    pb = p.copy()
    pb[rows, labels] -= 1.0
    out = dict(fwd)
    out.update(grad_x=grad_x, grad_kernel=grad_kernel, grad_bias=None if bias is None else s * pb.sum(axis=0),
               G=G, d=d, r=r, p_label=p[rows, labels], wh=wh, q=q, gw=gw, unit=unit, scale=s, info=info, x=x, labels=labels)
    return out


def bounds(ref, embed_dim, num_classes):
    """Per-element bounds of csrc/loss_grad.hip from a classifier_grad() result -> (grad_x [n, E], grad_kernel [E, C],
    grad_bias [C])."""
    x, wh, G, labels, info = ref["x"], ref["wh"], ref["G"], ref["labels"], ref["info"]
    n, C = G.shape
    rows = np.arange(n)
    s = abs(ref["scale"])
    fa = info["fa"]
    fs = 1.0 - fa
    logit = (embed_dim + 8) * U * ref["xnorm"] * ref["wnorm_max"] + ref["bias_abs_max"] * U
    # L_i of the forward bound with the phi' the backward uses: 0 outside the clip range, where the target is fs z + const
    fwd = dict(ref)
    fwd["lipschitz"] = np.maximum(1.0, fs + fa * np.abs(info["dphi"]))
    bt, bl, _ = ref_loss.bounds(fwd, embed_dim, num_classes)
    e = 1.01 * (logit + bl + U * (ref["xnorm"] * ref["wnorm_max"] + np.abs(ref["lse"]))) + 6.0 * U
    dG = np.abs(G) * e[:, None]
    dd = s * ref["p_label"] * 1.01 * (bt + bl)
    adphi = np.abs(info["dphi"])
    Gl = np.abs(G[rows, labels])
    dG[rows, labels] = dd * (fs + fa * adphi) + np.abs(ref["d"]) * fa * info["ddphi"] * U + U * Gl
    dr = dd * fa * np.abs(info["phi"] - info["dphi"] * info["c"]) + np.abs(ref["d"]) * fa * (2.0 * adphi + np.abs(info["c"]) * info["ddphi"]) * U
    awh = np.abs(wh)
    bx = dG @ awh.T + (C + 2) * U * (np.abs(G) @ awh.T) + dr[:, None] * np.abs(ref["unit"]) + 2.0 * U * np.abs(ref["grad_x"])
    a = np.abs(x).T @ dG + (n + 32) * U * (np.abs(x).T @ np.abs(G))           # [E, C]
    if ref["q"] is None:
        bk = a + U * np.abs(ref["grad_kernel"])
    else:
        q = ref["q"]
        D = np.sum(awh * a, axis=0, keepdims=True)
        big = (a + awh * D) / np.sqrt(np.maximum(q, 1e-300)) + 2.0 * U * np.abs(ref["grad_kernel"])
        bk = np.where((q > 1e-12)[None, :], big, a / 1e-6 + U * np.abs(ref["grad_kernel"]))
    bb = dG.sum(axis=0) + U * (0.0 if ref["grad_bias"] is None else np.abs(ref["grad_bias"]))
    return bx, bk, bb


# ---------------------------------------------------------------------------------------------- optimizer, float32
F = np.float32
SGD, MOMENTUM, ADAM = 0, 1, 2
CHUNK = 4096


def _tree64(v):
    """lane 0 of a shuffle-down tree over the last axis of 64 doubles (offsets 32 .. 1)."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def grad_norm(g):
    """||g|| as xv_opt_step sums it: float32(sqrt(sum in double, in the order of the header))."""
    g = np.asarray(g, dtype=F).reshape(-1)
    nb = -(-g.size // CHUNK)
    sq = np.zeros(nb * CHUNK)
    sq[:g.size] = g.astype(np.float64) ** 2
    sq = sq.reshape(nb, CHUNK // 256, 256)
    acc = np.zeros((nb, 256))
    for i in range(CHUNK // 256):
        acc = acc + sq[:, i, :]
    wv = _tree64(acc.reshape(nb, 4, 64))
    part = ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]
    lanes = np.zeros(64)
    for c0 in range(0, nb, 64):
        blk = part[c0:c0 + 64]
        lanes[:blk.size] = lanes[:blk.size] + blk
    return F(np.sqrt(_tree64(lanes)))


def adam_lr(lr, step):
    return F(float(lr) * math.sqrt(1.0 - 0.999 ** float(step)) / (1.0 - 0.9 ** float(step)))


def opt_step(kind, w, g, slot0=None, slot1=None, lr=0.1, l2=0.0, clip_norm=0.0, momentum=0.9, use_nesterov=False, step=1):
    """-> (w, slot0, slot1) after one step, float32, new arrays."""
    w = np.asarray(w, dtype=F).copy()
    g = np.asarray(g, dtype=F).copy()
    lr32, l232, clip, mom = F(lr), F(l2), F(clip_norm), F(momentum)
    if l232 != 0:
        g = g + l232 * w
    if clip > 0:
        den = max(grad_norm(g), clip)
        g = (g * clip) / den
    if kind == SGD:
        return w - lr32 * g, slot0, slot1
    if kind == MOMENTUM:
        a = mom * np.asarray(slot0, dtype=F) + g
        if use_nesterov:
            return w - lr32 * (g + mom * a), a, slot1
        return w - lr32 * a, a, slot1
    b1, b2 = F(0.9), F(0.999)
    omb1, omb2 = F(1.0 - 0.9), F(1.0 - 0.999)
    m = b1 * np.asarray(slot0, dtype=F) + omb1 * g
    v = b2 * np.asarray(slot1, dtype=F) + omb2 * (g * g)
    w = w - (adam_lr(lr, step) * m) / (np.sqrt(v) + F(1e-8))
    return w, m, v
