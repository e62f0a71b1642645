"""The rule of xv_stat_pool_forward / xv_stat_pool_backward (include/xvec_hip.h) in float64 numpy, the per-element bound of the
backward derived in the header of csrc/pool_grad.hip, a float32 emulation of both kernels in the order that header states, and
the replay of one whole training step of tf_kaldi_speaker_amd/frame_train.py: frame layers -> statistics pooling -> segment
layers -> softmax head (frame_grads), with the bound that step carries composed stage by stage (frame_grad_bounds).

Forward (model/pooling.py:27-52): m = mean_t x_t, v = mean_t (x_t - m)^2, std = sqrt(v <= 1e-12 ? 1e-12 : v).
Backward: gx_t = gm / n + [v > 1e-12] gs (x_t - m) / (n std); the floor mask is a constant to TensorFlow, and the term of
d v / d m multiplies sum_t (x_t - m) = 0.  tests/test_pool_grad_host.py holds this against torch.autograd in float64.

The forward's bars are mean_bar / var_bar / std_ratio of ref_pool.py with k = K = 16: the kernel forms 16 partial sums per channel
(partial s: the frames s, s + 16, ... in ascending order) and merges them by a binary tree, neighbours first.
The backward's bound, against the float64 rule at the same float32 m, std, v and gp:
    |gx^ - gx| <= u (2 |a| + 4 |b d|)(1 + 2^-20) + 2^-149,   a = gm / n, b = gs / (n std) or 0, d = x - m
(one rounding on a, two on b, one on d, one on the fma)."""
import numpy as np

import ref_loss_grad as rg
import ref_pool as rp
import ref_seg_grad as rs

U = 2.0 ** -24
ETA = 2.0 ** -149
FLOOR = 1e-12
K = 16                                        # partial sums per channel
F = np.float32
MARGIN = 64.0


# ------------------------------------------------------------------------------------------------ the float64 rule
def forward(x):
    """x [n, C] of ONE utterance -> (m, v, std) float64; n = 0: m = v = 0, std = sqrt(1e-12)."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        z = np.zeros(x.shape[1])
        return z, z.copy(), np.sqrt(rp.floor_var(z))
    return rp.stat_pool(x)


def terms(x, m, std, v, gp):
    """a [C], b [C], d [n, C] of the backward rule at the given m, std, v (the mask reads v)."""
    x, m, std, v, gp = (np.asarray(t, dtype=np.float64) for t in (x, m, std, v, gp))
    n, C = x.shape
    a = gp[:C] / n
    b = np.where(v > FLOOR, gp[C:] / (n * std), 0.0)
    return a, b, x - m[None, :]


def backward(x, m, std, v, gp):
    """gx [n, C] of ONE utterance, float64, at the given m, std, v and gp [2 C] = [gm | gs]."""
    a, b, d = terms(x, m, std, v, gp)
    return a[None, :] + b[None, :] * d


def backward_bound(x, m, std, v, gp):
    a, b, d = terms(x, m, std, v, gp)
    return U * (2.0 * np.abs(a)[None, :] + 4.0 * np.abs(b[None, :] * d)) * (1.0 + 2.0 ** -20) + ETA


def forward_ratios(x, got_mean, got_var, got_std):
    """Per-element error / bar of one utterance's (mean, variance before the floor, std) against the float64 pooling of x."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    m, v, _ = forward(x)
    a = np.abs(x).mean(axis=0)
    e_m, e_v = rp.mean_bar(n, K, a), rp.var_bar(n, K, a, v)
    err_v = np.abs(np.asarray(got_var, dtype=np.float64) - v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_v = np.where(e_v > 0, err_v / e_v, np.where(err_v == 0, 0.0, np.inf))
    return rp.mean_ratio(got_mean, m, e_m), r_v, rp.std_ratio(got_std, v, e_v)


def pool_packed(x, offsets):
    """x [rows, C], offsets [B + 1] -> (pooled [B, 2 C], var [B, C]) float64."""
    x = np.asarray(x, dtype=np.float64)
    B, C = len(offsets) - 1, x.shape[1]
    pooled, var = np.zeros((B, 2 * C)), np.zeros((B, C))
    for u in range(B):
        m, v, s = forward(x[offsets[u]:offsets[u + 1]])
        pooled[u, :C], pooled[u, C:], var[u] = m, s, v
    return pooled, var


def backward_packed(x, offsets, pooled, var, gp):
    """-> gx [rows, C] float64 (rows no utterance owns stay zero)."""
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[1]
    gx = np.zeros_like(x)
    for u in range(len(offsets) - 1):
        r0, r1 = offsets[u], offsets[u + 1]
        if r1 > r0:
            gx[r0:r1] = backward(x[r0:r1], pooled[u, :C], pooled[u, C:], var[u], gp[u])
    return gx


# ------------------------------------------------------------------------------------------------ float32 emulations
def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def _tree16(acc):
    parts = [acc[i] for i in range(K)]
    while len(parts) > 1:
        parts = [(parts[i] + parts[i + 1]).astype(F) for i in range(0, len(parts), 2)]
    return parts[0]


def emu_forward(x, one_pass=False):
    """stat_pool_fwd_kernel on one utterance -> (mean, var, std) float32.  one_pass: the mutant E[x^2] - m^2."""
    x = np.asarray(x, dtype=F)
    n, C = x.shape
    if n == 0:
        z = np.zeros(C, dtype=F)
        return z, z.copy(), np.sqrt(np.full(C, F(FLOOR), dtype=F))
    acc = np.zeros((K, C), dtype=F)
    for i in range(0, n, K):
        c = x[i:i + K]
        acc[:c.shape[0]] = acc[:c.shape[0]] + c
    mean = (_tree16(acc) / F(n)).astype(F)
    acc = np.zeros((K, C), dtype=F)
    for i in range(0, n, K):
        c = x[i:i + K]
        d = c if one_pass else (c - mean[None, :]).astype(F)
        acc[:c.shape[0]] = _fma(d, d, acc[:c.shape[0]])
    var = (_tree16(acc) / F(n)).astype(F)
    if one_pass:
        var = (var - (mean * mean).astype(F)).astype(F)
    with np.errstate(invalid="ignore"):
        std = np.sqrt(np.where(var <= F(FLOOR), F(FLOOR), var).astype(F)).astype(F)
    return mean, var, std


def emu_backward(x, m, std, v, gp, n_minus_1=False, no_mask=False, drop_a=False, flip_b=False):
    """stat_pool_bwd_kernel on one utterance, float32, every operation rounded once; the keywords are the mutants."""
    x, m, std, v, gp = (np.asarray(t, dtype=F) for t in (x, m, std, v, gp))
    n, C = x.shape
    fn = F(n - 1 if n_minus_1 else n)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (gp[:C] / fn).astype(F)
        b = (gp[C:] / (fn * std).astype(F)).astype(F)
    if not no_mask:
        b = np.where(v > F(FLOOR), b, F(0.0)).astype(F)
    if drop_a:
        a = np.zeros_like(a)
    if flip_b:
        b = -b
    d = (x - m[None, :]).astype(F)
    return _fma(b[None, :], d, a[None, :])


# ------------------------------------------------------------------------------------------------ one training step
def frame_grads(frame_layers, seg_layers, head_w, head_b, frames, offsets, labels):
    """The float64 rule of one step at the given (float32) parameters: the frame layers (ref_seg_grad.Layer, in forward order) on
    the packed rows, statistics pooling per utterance, both segment layers, the plain softmax head's mean loss and gradients
    (ref_loss_grad.classifier_grad), then everything backward -> dict(frame_fwd, frame_bwd [lists in forward order], pool,
    seg_fwd, seg_bwd, head)."""
    offsets = [int(o) for o in offsets]
    x = np.asarray(frames, dtype=np.float64)
    ffwd = []
    for l in frame_layers:
        ffwd.append(rs.forward(x, l.w, l.b, l.bn, l.act, rs.SLOPE))
        x = ffwd[-1]["y"]
    pooled, var = pool_packed(x, offsets)
    s1, s2 = seg_layers
    f1 = rs.forward(pooled, s1.w, s1.b, s1.bn, s1.act, rs.SLOPE)
    f2 = rs.forward(f1["y"], s2.w, s2.b, s2.bn, s2.act, rs.SLOPE)
    hd = rg.classifier_grad(f2["y"], labels, np.asarray(head_w, dtype=np.float64), head_b, "softmax", 0.0, 0.0)
    b2 = rs.backward(f2, hd["grad_x"], rs.SLOPE)
    b1 = rs.backward(f1, b2["gx"], rs.SLOPE)
    gx = backward_packed(x, offsets, pooled, var, b1["gx"])
    pool = dict(x=x, offsets=offsets, pooled=pooled, var=var, gp=b1["gx"], gx=gx)
    fbwd, g = [], gx
    for f in reversed(ffwd):
        fbwd.insert(0, rs.backward(f, g, rs.SLOPE))
        g = fbwd[0]["gx"]
    return dict(frame_fwd=ffwd, frame_bwd=fbwd, pool=pool, seg_fwd=[f1, f2], seg_bwd=[b1, b2], head=hd)


def _slope(f):
    if f["act"] == rs.NONE:
        return np.ones_like(f["h"])
    return np.where(f["h"] > 0, 1.0, 0.0 if f["act"] == rs.RELU else rs.SLOPE)


def _forward_carry(f, own, dx):
    """A layer's forward with an input off by dx [n, K] -> (what z moves by beyond its own bound, what h moves by beyond its own
    bound, the whole error of y).  Where the sign of h is certain (|h| above its whole error) y's error is the activation's
    slope there times h's, plus the activation's own roundings; elsewhere the slope is taken as 1."""
    inz = dx @ np.abs(f["w"]).T
    sr = 1.0 if f["bn"] is None else np.abs(f["bn"][0] * f["r"])[None, :]
    extra_h = sr * inz
    dh = own["h"] + extra_h
    slope = np.where(np.abs(f["h"]) > dh, _slope(f), 1.0)
    return inz, extra_h, slope * dh + 2.0 * U * np.abs(f["y"])


def frame_grad_bounds(res, embed_dim, num_classes):
    """How far a float32 evaluation of the step may lie from frame_grads, per element and to first order: every stage's own bound
    (ref_seg_grad.bounds, the bars of ref_pool with k = 16, backward_bound, ref_loss_grad.bounds) plus what the stage in front
    hands on.  Through the pooling: an input off by dy moves m by mean_t dy, v by 2 mean_t |x - m| (dy + dm), std by
    dv / (2 std); in the backward dgx = own + dgm / n + |d| (dgs / (n std) + |b| dstd / std) + |b| (dy + dm).
    -> dict(frame=[dict(w, b, gamma, beta)], seg=[...], head_kernel [E, C], head_bias [C], extra_h=[per layer, frame layers
    first], pool=dict(dm, dv, dstd, live, v, std))."""
    ffwd, fbwd, pool = res["frame_fwd"], res["frame_bwd"], res["pool"]
    (f1, f2), (b1, b2), hd = res["seg_fwd"], res["seg_bwd"], res["head"]
    # ---- forward
    dy = np.zeros_like(ffwd[0]["x"])
    fown, fin, extra = [], [], []
    for f, b in zip(ffwd, fbwd):
        own = rs.bounds(f, b)
        inz, eh, dy_out = _forward_carry(f, own, dy)
        fown.append(own)
        fin.append((inz, dy))
        extra.append(eh)
        dy = dy_out
    x, offsets = pool["x"], pool["offsets"]
    B, C = len(offsets) - 1, x.shape[1]
    dm, dv, dstd = np.zeros((B, C)), np.zeros((B, C)), np.zeros((B, C))
    std, v = pool["pooled"][:, C:], pool["var"]
    live = v > FLOOR
    for u in range(B):
        r0, r1 = offsets[u], offsets[u + 1]
        n = r1 - r0
        if n == 0:
            continue
        xu, du = x[r0:r1], dy[r0:r1]
        a = np.abs(xu).mean(axis=0)
        dm[u] = rp.mean_bar(n, K, a) + du.mean(axis=0)
        dv[u] = rp.var_bar(n, K, a, v[u]) + 2.0 * (np.abs(xu - pool["pooled"][u, :C][None, :]) * (du + dm[u][None, :])).mean(axis=0)
    # sqrtf and the float32 floor constant: 2 u std; a live std moves by dv / (2 std), 1.02 for the curvature while std >= 64 dstd
    dstd = 2.0 * U * std + np.where(live, 1.02 * dv / (2.0 * std), 0.0)
    dpool = np.concatenate([dm, dstd], axis=1)
    e1, e2 = rs.bounds(f1, b1), rs.bounds(f2, b2)
    in1, eh1, dy1 = _forward_carry(f1, e1, dpool)
    in2, eh2, dy2 = _forward_carry(f2, e2, dy1)
    extra += [eh1, eh2]
    # ---- the head (plain softmax), as ref_seg_grad.tail_grad_bounds composes it
    assert hd["q"] is None, "the composed bound is written for the plain softmax head"
    nb = f1["x"].shape[0]
    bx, bk, bb = rg.bounds(hd, embed_dim, num_classes)
    wh = np.abs(hd["wh"])
    du = np.max(dy2 @ wh, axis=1)
    dG = 2.0 * np.abs(hd["G"]) * du[:, None]
    dG[np.arange(nb), hd["labels"]] = 2.0 * abs(hd["scale"]) * hd["p_label"] * du
    hk = bk + np.abs(hd["x"]).T @ dG + dy2.T @ np.abs(hd["G"])
    hb = bb + dG.sum(axis=0)
    gy2 = bx + dG @ wh.T
    # ---- backward
    out2 = rs._carry(f2, b2, e2, gy2, in2, dy1)
    out1 = rs._carry(f1, b1, e1, out2.pop("gx_total"), in1, dpool)
    dgp = out1.pop("gx_total")
    dgx = np.zeros_like(x)
    for u in range(B):
        r0, r1 = offsets[u], offsets[u + 1]
        n = r1 - r0
        if n == 0:
            continue
        xu = x[r0:r1]
        m_u, s_u = pool["pooled"][u, :C], std[u]
        a, b, d = terms(xu, m_u, s_u, v[u], pool["gp"][u])
        own = U * (2.0 * np.abs(a)[None, :] + 4.0 * np.abs(b[None, :] * d)) * (1.0 + 2.0 ** -20) + ETA
        dgs = np.where(live[u], dgp[u, C:] / (n * s_u), 0.0)
        dgx[r0:r1] = (own + (dgp[u, :C] / n)[None, :] + np.abs(d) * (dgs + np.abs(b) * dstd[u] / s_u)[None, :]
                      + np.abs(b)[None, :] * (dy[r0:r1] + dm[u][None, :]))
    fout, g = [], dgx
    for f, b, own, (inz, dx) in reversed(list(zip(ffwd, fbwd, fown, fin))):
        o = rs._carry(f, b, own, g, inz, dx)
        g = o.pop("gx_total")
        fout.insert(0, o)
    return dict(frame=fout, seg=[out1, out2], head_kernel=hk, head_bias=hb, extra_h=extra,
                pool=dict(dm=dm, dv=dv, dstd=dstd, live=live, v=v, std=std), forward_output=dy2)


def pool_precondition(pb):
    """Every variance lies outside 1e-12 +- dv (the floor mask of the step is certain), every live std is at least 64 dstd (the
    first-order carry through the square root holds) -> the number of live elements."""
    assert np.all(np.abs(pb["v"] - FLOOR) > pb["dv"]), "a variance lies within its bound of the floor"
    assert np.all(pb["std"][pb["live"]] >= MARGIN * pb["dstd"][pb["live"]]), "a live std lies within 64 bounds of zero"
    return int(pb["live"].sum())
