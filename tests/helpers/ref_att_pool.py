"""The rule of xv_att_pool_forward / xv_att_pool_backward (include/xvec_hip.h) in float64 numpy and the per-element bounds
derived in the header of csrc/att_pool_grad.hip.

Shapes of ONE utterance: key [n, Dk], value [n, Dv], query [H, dq], w [n, H]; m, var, std, gm, gs [P], P = H dv, column h dv + d.
Head h reads the key columns h dq + d when the key is split, else d; the value columns likewise (model/pooling.py:150-218).

    s[t,h]   = scale sum_d key q                    w = softmax over the frames (max subtracted)
    m[h,d]   = sum_t w v                            var = sum_t w (v - m)^2          std = sqrt(var <= floor ? floor : var)
    gvar     = var > floor ? gs / (2 std) : 0       (the floor mask is a constant to TensorFlow)
    gvalue   = sum_h w (gm + 2 gvar (v - m))        gw = sum_d (gm v + gvar (v - m)^2)    c = sum_d (gm m + gvar var)
    gscore   = w (gw - c)                           gkey = sum_h scale gscore q           gquery = scale sum_t gscore key
The term of d var / d m multiplies sum_t w (v - m) = 0 and is dropped; c equals sum_t w gw when m and var are the exact moments.
tests/test_att_pool_host.py holds all of this against torch.autograd in float64.  The floor is the float32 constant 1e-12f the
kernel compares with (it differs from 1e-12 by less than one float32 rounding; a float32 variance never lies between them).

Bounds (u = 2^-24, eta = 2^-149, gamma_k = k u / (1 - k u)); each is against the float64 rule at the float32 values named:
    score    E = gamma_K |scale| sum_d |key q| + (dq |scale| + 1) eta,  K = ceil(dq / 64) + 7      (same key, query)
    weights  w (exp(2 Emax)(1 + u + 2^-27) - 1) + eta,  Emax over the frames of the utterance        (same key, query)
    mean     gamma_Kn sum_t |w v| + n eta,  Kn = ceil(n / 16) + 4                                   (the w the kernel wrote)
    var      gamma_(Kn+3) var + (n + 2) eta                                                         (the w and m it wrote)
    std      2 u std                                                                                (the var it wrote)
    gvalue   u (Hs + 4)(1 + 2^-20) sum_h w (|gm| + |2 gvar (v - m)|) + eta sum_h (1 + w |v - m|),  Hs = 1 when the value is
             split, else H
    gscore   Eg = u |gscore| + w (u sum_d |gvar| ((v - m)^2 + var) + (dv + 16) 2^-50 A) + eta,
             A = sum_d (|gm v| + |gvar| (v - m)^2 + |gm m| + |gvar| var)
    gkey     (1 + 2^-20)(sum_h |scale q| Eg + u (Hk + 2) sum_h |scale gscore q|) + eta sum_h (1 + |q|),  Hk likewise
    gquery   (1 + 2^-20) |scale| sum_t Eg |key| + u |gquery| + (rows + 32) 2^-50 |scale| sum_t |gscore key| + eta
(the backward's at the w, m, std, var the forward wrote).  The eta terms are the underflow part of fl(x) = x (1 + delta) + eta',
|eta'| <= eta / 2: an operation whose result is subnormal errs absolutely, so they count per operation (dq or n fmas), not per
path as the relative part does."""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -149
F = np.float32
FLOOR = float(np.float32(1e-12))
SLACK = 1.0 + 2.0 ** -20


def gamma(k):
    return k * U / (1.0 - k * U)


class Cfg:
    """heads, per-head widths and the split flags of one call."""

    def __init__(self, H, dq, dv, split_k, split_v, use_scale):
        self.H, self.dq, self.dv, self.split_k, self.split_v, self.use_scale = H, dq, dv, bool(split_k), bool(split_v), bool(use_scale)
        self.Dk = H * dq if split_k else dq
        self.Dv = H * dv if split_v else dv
        self.P = H * dv
        self.scale = float(F(1.0 / np.sqrt(float(dq)))) if use_scale else 1.0     # 1 / sqrt(dq) rounded to float32

    def __repr__(self):
        return "H%d dq%d dv%d %s%s%s" % (self.H, self.dq, self.dv, "K" if self.split_k else "k", "V" if self.split_v else "v",
                                         "s" if self.use_scale else "")

    def key_head(self, key, h):
        return key[:, h * self.dq:(h + 1) * self.dq] if self.split_k else key

    def value_head(self, value, h):
        return value[:, h * self.dv:(h + 1) * self.dv] if self.split_v else value

    def pcols(self, h):
        return slice(h * self.dv, (h + 1) * self.dv)


def f64(*a):
    return tuple(np.asarray(t, dtype=np.float64) for t in a)


# ------------------------------------------------------------------------------------------------ forward
def scores(cfg, key, query):
    key, query = f64(key, query)
    return np.stack([cfg.scale * (cfg.key_head(key, h) @ query[h]) for h in range(cfg.H)], axis=1)


def score_bound(cfg, key, query):
    key, query = f64(key, query)
    K = -(-cfg.dq // 64) + 7
    a = np.stack([np.abs(cfg.key_head(key, h)) @ np.abs(query[h]) for h in range(cfg.H)], axis=1)
    return gamma(K) * abs(cfg.scale) * a + (cfg.dq * abs(cfg.scale) + 1) * ETA


def softmax(s):
    e = np.exp(s - s.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def weights_bound(w, E):
    """w [n, H] the float64 weights, E [n, H] the score bounds."""
    e2 = 2.0 * E.max(axis=0, keepdims=True)
    return w * (np.expm1(e2) + np.exp(e2) * (U + 2.0 ** -27)) + ETA


def moments(cfg, value, w, m=None):
    """-> (m, var) [P] float64 with the weights w; var about the given m (default: the one just computed)."""
    value, w = f64(value, w)
    n = value.shape[0]
    mean = np.zeros(cfg.P)
    if n:
        for h in range(cfg.H):
            mean[cfg.pcols(h)] = w[:, h] @ cfg.value_head(value, h)
    about = mean if m is None else np.asarray(m, dtype=np.float64)
    var = np.zeros(cfg.P)
    if n:
        for h in range(cfg.H):
            var[cfg.pcols(h)] = w[:, h] @ (cfg.value_head(value, h) - about[cfg.pcols(h)][None, :]) ** 2
    return mean, var


def floor_std(var):
    var = np.asarray(var, dtype=np.float64)
    return np.sqrt(np.where(var <= FLOOR, FLOOR, var))


def mean_bound(cfg, value, w):
    value, w = f64(value, w)
    n = value.shape[0]
    Kn = -(-n // 16) + 4
    a = np.zeros(cfg.P)
    for h in range(cfg.H):
        a[cfg.pcols(h)] = np.abs(w[:, h]) @ np.abs(cfg.value_head(value, h))
    return gamma(Kn) * a + n * ETA


def var_bound(n, var):
    Kn = -(-n // 16) + 4
    return gamma(Kn + 3) * np.asarray(var, dtype=np.float64) + ((n + 2) * ETA if n else 0.0)


def forward(cfg, key, value, query):
    """The whole forward of one utterance in float64 -> dict(s, w, m, var, std)."""
    s = scores(cfg, key, query)
    w = softmax(s) if s.shape[0] else s
    m, var = moments(cfg, value, w)
    return dict(s=s, w=w, m=m, var=var, std=floor_std(var))


# ------------------------------------------------------------------------------------------------ backward
def backward(cfg, key, value, query, w, m, std, var, gp):
    """One utterance, float64, at the given w, m, std, var and gp [2 P] = [gm | gs] ->
    dict(gvalue, gkey, gquery (this utterance's share, scaled), gscore, and the bounds b_gvalue, b_gscore, b_gkey; t_gquery holds
    the two sums the batch-level bound of gquery needs)."""
    key, value, query, w, m, std, var, gp = f64(key, value, query, w, m, std, var, gp)
    n = value.shape[0]
    H, P = cfg.H, cfg.P
    gm, gs = gp[:P], gp[P:]
    gvar = np.where(var > FLOOR, gs / (2.0 * std), 0.0)
    Hs, Hk = (1 if cfg.split_v else H), (1 if cfg.split_k else H)
    gvalue, b_gvalue, u_gvalue = np.zeros((n, cfg.Dv)), np.zeros((n, cfg.Dv)), np.zeros((n, cfg.Dv))
    gkey, b_gkey = np.zeros((n, cfg.Dk)), np.zeros((n, cfg.Dk))
    gscore, Eg = np.zeros((n, H)), np.zeros((n, H))
    gquery, t_err, t_abs = np.zeros((H, cfg.dq)), np.zeros((H, cfg.dq)), np.zeros((H, cfg.dq))
    sc = cfg.scale
    for h in range(H):
        pc = cfg.pcols(h)
        v = cfg.value_head(value, h)
        d = v - m[pc][None, :]
        wh = w[:, h:h + 1]
        vs = slice(h * cfg.dv, (h + 1) * cfg.dv) if cfg.split_v else slice(0, cfg.dv)
        gvalue[:, vs] += wh * (gm[pc] + 2.0 * gvar[pc] * d)
        b_gvalue[:, vs] += wh * (np.abs(gm[pc]) + np.abs(2.0 * gvar[pc] * d))
        u_gvalue[:, vs] += ETA * (1.0 + wh * np.abs(d))
        gw = (gm[pc] * v + gvar[pc] * d * d).sum(axis=1)
        c = (gm[pc] * m[pc] + gvar[pc] * var[pc]).sum()
        gscore[:, h] = w[:, h] * (gw - c)
        A = (np.abs(gm[pc] * v) + np.abs(gvar[pc]) * d * d + np.abs(gm[pc] * m[pc]) + np.abs(gvar[pc]) * var[pc]).sum(axis=1)
        G = (np.abs(gvar[pc]) * (d * d + var[pc])).sum(axis=1)
        Eg[:, h] = U * np.abs(gscore[:, h]) + w[:, h] * (U * G + (cfg.dv + 16) * 2.0 ** -50 * A) + ETA
        k = cfg.key_head(key, h)
        ks = slice(h * cfg.dq, (h + 1) * cfg.dq) if cfg.split_k else slice(0, cfg.dq)
        gkey[:, ks] += sc * gscore[:, h:h + 1] * query[h][None, :]
        b_gkey[:, ks] += SLACK * (np.abs(sc * query[h])[None, :] * Eg[:, h:h + 1]
                                  + U * (Hk + 2) * np.abs(sc * gscore[:, h:h + 1] * query[h][None, :])) \
            + ETA * (1.0 + np.abs(query[h]))[None, :]
        gquery[h] = sc * (gscore[:, h] @ k)
        t_err[h] = abs(sc) * (Eg[:, h] @ np.abs(k))
        t_abs[h] = abs(sc) * (np.abs(gscore[:, h]) @ np.abs(k))
    b_gvalue = U * (Hs + 4) * SLACK * b_gvalue + u_gvalue
    return dict(gvalue=gvalue, gkey=gkey, gquery=gquery, gscore=gscore, b_gvalue=b_gvalue, b_gscore=Eg, b_gkey=b_gkey,
                t_gquery=(t_err, t_abs))


def gquery_bound(gquery, t_err, t_abs, rows):
    """The batch-level bound: gquery and the two sums of backward()'s t_gquery added over the utterances."""
    return SLACK * t_err + U * np.abs(gquery) + (rows + 32) * 2.0 ** -50 * t_abs + ETA


# ------------------------------------------------------------------------------------------------ a packed batch
def check_batch(cfg, key, value, query, offsets, gp, got):
    """Every element of what the device returned (got: weights [rows, H], pooled [B, 2 P], var [B, P], gvalue, gkey [rows, .],
    gquery [H, dq], all float32) against its bound -> dict of the largest error / bound per output.  The forward's references
    are chained as the header states: weights against the float64 forward, the moments at the written weights, the variance
    about the written mean, std from the written variance, the backward at everything the forward wrote."""
    P = cfg.P
    worst = dict(weights=0.0, mean=0.0, var=0.0, std=0.0, gvalue=0.0, gkey=0.0, gquery=0.0)

    def upd(name, err, bound):
        if err.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
            assert not np.any(np.isnan(r)), name
            worst[name] = max(worst[name], float(np.max(r)))

    gq, t_err, t_abs = np.zeros((cfg.H, cfg.dq)), np.zeros((cfg.H, cfg.dq)), np.zeros((cfg.H, cfg.dq))
    for u in range(len(offsets) - 1):
        r0, r1 = int(offsets[u]), int(offsets[u + 1])
        k, v = key[r0:r1], value[r0:r1]
        w = got["weights"][r0:r1].astype(np.float64)
        mean, std, var = (got["pooled"][u, :P].astype(np.float64), got["pooled"][u, P:].astype(np.float64),
                          got["var"][u].astype(np.float64))
        if r1 > r0:
            ref = forward(cfg, k, v, query)
            upd("weights", np.abs(w - ref["w"]), weights_bound(ref["w"], score_bound(cfg, k, query)))
        m_ref, _ = moments(cfg, v, w)
        upd("mean", np.abs(mean - m_ref), mean_bound(cfg, v, w))
        _, v_ref = moments(cfg, v, w, m=mean)
        upd("var", np.abs(var - v_ref), var_bound(r1 - r0, v_ref))
        s_ref = floor_std(var)
        upd("std", np.abs(std - s_ref), 2.0 * U * s_ref)
        if r1 > r0:
            b = backward(cfg, k, v, query, w, mean, std, var, gp[u])
            upd("gvalue", np.abs(got["gvalue"][r0:r1] - b["gvalue"]), b["b_gvalue"])
            upd("gkey", np.abs(got["gkey"][r0:r1] - b["gkey"]), b["b_gkey"])
            gq += b["gquery"]
            t_err += b["t_gquery"][0]
            t_abs += b["t_gquery"][1]
    rows = int(offsets[-1]) - int(offsets[0])
    upd("gquery", np.abs(got["gquery"] - gq), gquery_bound(gq, t_err, t_abs, rows))
    return worst
