"""The gradient of the triplet heads in numpy float64, as include/xvec_hip.h states it (xv_metric_loss_grad): closed form,
anchor by anchor, so a group of 1024 rows builds nothing larger than [B, B].  The forward is ref_metric_loss's; this file adds
the coefficient counts of the mining, W = dL / dM before normalisation (M = D2 resp. the clipped cosine), the second pass
H = W + W^T and the normalisation backward.  One group per call.

Choices the rule fixes (where TensorFlow's is not unique or not finite): a hinge passes iff t > 0, the clamp of D2 included;
a selection sends its gradient to the lowest column among equals; D2 == 0 and |c| = 1 carry nothing; the pair (i, i) carries
nothing; the max branch of the normalisation is a constant.

margins() reports how far every decision is from flipping; bounds() states the per-element bar of csrc/metric_loss_grad.hip."""
import numpy as np

import ref_metric_loss as rm

UNIT = rm.UNIT


def pos_slope(c, head, margin):
    """d pos / dc on -1 < c < 1; the signs of pos_value are constants."""
    if head == "asoftmax":
        if margin == 1:
            return np.ones_like(c)
        if margin == 2:
            return 4.0 * np.abs(c)
        s3 = np.sign(2.0 * c * c - 1.0) * np.sign(c)
        return s3 * (32.0 * c * c * c - 16.0 * c)
    if head == "additive_margin_softmax":
        return np.ones_like(c)
    dt = np.cos(margin) + c * np.sin(margin) / np.sqrt(1.0 - c * c)
    return np.where(c <= np.cos(np.pi - margin), -dt, dt)


def pos_curvature(c, head, margin):
    """|d^2 pos / dc^2|: how far an error of c moves pos'."""
    if head == "asoftmax" and margin == 2:
        return np.full_like(c, 4.0)
    if head == "asoftmax" and margin == 4:
        return np.abs(96.0 * c * c - 16.0)
    if head == "additive_angular_margin_softmax":
        return np.sin(margin) / (1.0 - c * c) ** 1.5
    return np.zeros_like(c)


def _gap(values, largest=False):
    """How far the selected (least, or largest) value is from the next different one."""
    s = np.unique(values)
    if s.size < 2:
        return np.inf
    return s[-1] - s[-2] if largest else s[1] - s[0]


def grad(kind, x, labels, grad_scale=1.0, **o):
    """-> dict(res = the forward of ref_metric_loss.evaluate, grad [B, d] float64 (grad_scale dL/dx, not rounded), W, dW (the
    bound on W's error from the derivative factors, per unit of relative product error), kappa, v, s, and the margins)."""
    x = rm._f32(x)
    labels = np.asarray(labels)
    B, d = x.shape
    res = rm.evaluate(kind, x, labels, **o)
    normalize = True if kind != "semihard" else o.get("normalize", True)
    n = np.array([rm.G(r, r) for r in x])
    s = 1.0 / np.sqrt(np.maximum(n, rm.EPS)) if normalize else np.ones(B)
    v = x * s[:, None]
    W, dW = np.zeros((B, B)), np.zeros((B, B))
    hinge, sel = np.inf, np.inf           # the least |t| of a hinge, the least gap behind a selection
    if kind == "semihard":
        margin, squared = o.get("margin", 0.2), o.get("squared", False)
        M = res["dist"]
        nmax = max(res["nmax"], 1.0)
        for i in range(B):
            same = labels == labels[i]
            neg = np.nonzero(~same)[0]
            same[i] = False
            pos = np.nonzero(same)[0]
            if neg.size == 0 or pos.size == 0:
                continue
            dn = M[i, neg]
            coef = np.zeros(B)
            for j in pos:
                above = dn > M[i, j]
                if above.any():
                    k = neg[above][np.argmin(dn[above])]          # the first of equals: the lowest column
                    sel = min(sel, _gap(dn[above]))
                else:
                    k = neg[np.argmax(dn)]
                    sel = min(sel, _gap(dn, largest=True))
                t = margin + M[i, j] - M[i, k]
                hinge = min(hinge, abs(t))
                if t > 0:
                    coef[j] += 1.0
                    coef[k] -= 1.0
            with np.errstate(divide="ignore", invalid="ignore"):
                if squared:
                    f = (M[i] > 0).astype(np.float64)
                    c3 = np.zeros(B)
                else:
                    f = np.where(M[i] > 0, 1.0 / (2.0 * M[i]), 0.0)
                    c3 = np.where(M[i] > 0, nmax / M[i] ** 3, 0.0)      # |d(1 / (2 d)) / dD2| = 1 / (4 d^3), D2 within 4 unit nmax
            W[i] = coef * f
            dW[i] = np.abs(coef) * c3
        denom = max(float(res["group_counts"][0]), 1e-16)
    else:
        head, margin = o["loss_type"], o["margin"]
        M = res["cos"]
        inside = (M > -1.0) & (M < 1.0)
        for i in range(B):
            same = labels == labels[i]
            neg = np.nonzero(~same)[0]
            if neg.size == 0:
                continue
            coef, curv = np.zeros(B), np.zeros(B)
            safe = np.where(inside[i], M[i], 0.0)
            slope = np.where(inside[i], pos_slope(safe, head, margin), 0.0)
            curve = np.where(inside[i], pos_curvature(safe, head, margin), 0.0)
            if kind == "hard":
                own = np.nonzero(same)[0]
                pv = np.array([rm.pos_value(M[i, j], head, margin) for j in own])
                j = own[np.argmin(pv)]
                k = neg[np.argmax(M[i, neg])]
                sel = min(sel, _gap(pv), _gap(M[i, neg], largest=True))
                t = M[i, k] - pv.min()
                hinge = min(hinge, abs(t))
                if t > 0:
                    coef[k] += 1.0 if inside[i, k] else 0.0
                    if j != i:
                        coef[j] -= slope[j]
                        curv[j] = curve[j]
            else:
                same[i] = False
                pos = np.nonzero(same)[0]
                if pos.size == 0:
                    continue
                pv = np.array([rm.pos_value(M[i, j], head, margin) for j in pos])
                act = (M[i, neg][None, :] - pv[:, None]) > 0
                coef[neg] = act.sum(axis=0) * inside[i, neg]
                coef[pos] = -act.sum(axis=1) * slope[pos]
                curv[pos] = act.sum(axis=1) * curve[pos]
            W[i] = coef
            dW[i] = curv
        if kind == "hard":
            denom = float(B)
        else:
            hinge = res["min_abs_t"]
            denom = float(res["group_counts"][0]) + 1e-16
    kappa = grad_scale / denom
    H = W + W.T
    gv = 2.0 * (H.sum(axis=1)[:, None] * v - H @ v) if kind == "semihard" else H @ v
    if normalize:
        proj = gv - np.sum(gv * v, axis=1)[:, None] * v
        gx = s[:, None] * np.where((n > rm.EPS)[:, None], proj, gv)
    else:
        gx = gv
    off = ~np.eye(B, dtype=bool)
    out = dict(res=res, grad=kappa * gx, W=W, dW=dW, kappa=kappa, v=v, s=s, normalize=normalize, kind=kind,
               min_gap=res.get("min_gap", np.inf), min_abs_t=hinge, sel_gap=sel)
    if kind == "semihard":
        out["min_d2"] = M[off & (M > 0)].min() if (off & (M > 0)).any() else np.inf
        out["min_1mc"] = np.inf
    else:
        out["min_d2"] = np.inf
        away = np.abs(M[off & inside]) if (off & inside).any() else np.zeros(0)
        out["min_1mc"] = (1.0 - away).min() if away.size else np.inf
    return out


def margins(out):
    """How far the decisions are from flipping: the gap between a positive's and a negative's distance (min_gap), the least
    |t| of a hinge (min_abs_t), the gap behind a selection (sel_gap), the least D2 > 0 and the least 1 - |c| inside the clip."""
    return {k: float(out[k]) for k in ("min_gap", "min_abs_t", "sel_gap", "min_d2", "min_1mc")}


def bounds(out, d):
    """-> the bar on |float32 grad_x - out["grad"]| per element, as the header of csrc/metric_loss_grad.hip derives it: the final
    float32 rounding; 2^-53 (B + d + 32) times the absolute sum of the element's terms, projection included, taken twice since
    this oracle's own float64 sums carry the same error; and the derivative factors evaluated on a computed c or D2, which
    are within unit = (d + 8) 2^-53 of the exact ones, through |pos''| resp. 1 / d^3 (out["dW"])."""
    B = out["W"].shape[0]
    unit = (d + 8) * UNIT
    av, s, k = np.abs(out["v"]), out["s"], abs(out["kappa"])

    def through(absH):
        if out["kind"] == "semihard":
            return 2.0 * (absH.sum(axis=1)[:, None] * av + absH @ av)
        return absH @ av

    def projected(e):
        if not out["normalize"]:
            return e
        return s[:, None] * (e + np.sum(e * av, axis=1)[:, None] * av)

    a = projected(through(np.abs(out["W"]) + np.abs(out["W"]).T))
    da = projected(through(unit * (out["dW"] + out["dW"].T)))
    g = np.abs(out["grad"])
    return 2.0 ** -24 * g + k * (2.0 * (B + d + 32) * UNIT * a + da) + 1e-45
