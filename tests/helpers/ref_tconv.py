"""The rule of xv_tconv_forward / xv_tconv_backward (include/xvec_hip.h) in float64 numpy and the per-element error bound derived
in the header of csrc/tconv_grad.hip restated as bounds().

A W-tap temporal convolution on packed utterances is the dense layer of ref_seg_grad on the im2col matrix X [total_out, W C],
X[out_off[b] + t, tau C + c] = x[off[b] + t + tau, c]; its input gradient is the col2im of the dense layer's.  forward() builds X
explicitly (the kernels never do), so W = 1 IS ref_seg_grad.  The rule is checked against torch.autograd of conv1d + eval-mode
batch_norm + relu / leaky_relu(0.2) in float64 (tests/test_tconv_host.py)."""
import numpy as np

import ref_seg_grad as rs

U = rs.U
F = np.float32
NONE, RELU, LRELU = rs.NONE, rs.RELU, rs.LRELU
SLOPE = rs.SLOPE


def out_offsets(offsets, taps):
    """offsets [B + 1] of the input rows -> offsets [B + 1] of the packed output rows, n_out = max(n_in - (taps - 1), 0)."""
    n = np.maximum(np.diff(np.asarray(offsets, dtype=np.int64)) - (taps - 1), 0)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def rows_of(offsets, taps):
    """-> the first input row of every output row, int64 [total_out]."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = np.maximum(np.diff(offsets) - (taps - 1), 0)
    return np.concatenate([offsets[b] + np.arange(n[b]) for b in range(n.size)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)


def im2col(x, offsets, taps):
    """x [rows, C] -> X [total_out, taps C], k = tau C + c."""
    x = np.asarray(x)
    first = rows_of(offsets, taps)
    return np.concatenate([x[first + tau] for tau in range(taps)], axis=1) if first.size else np.zeros((0, taps * x.shape[1]), x.dtype)


def col2im(G, offsets, taps, rows, C):
    """G [total_out, taps C] -> [rows, C]: every element added to the input row and channel it was read from."""
    first = rows_of(offsets, taps)
    out = np.zeros((rows, C), dtype=G.dtype)
    for tau in range(taps):
        np.add.at(out, first + tau, G[:, tau * C:(tau + 1) * C])
    return out


def forward(x, offsets, taps, w, b, bn=None, act=NONE, slope=SLOPE):
    """x [rows, C], w [N, taps C] rows, b [N] -> ref_seg_grad.forward of the im2col matrix, plus offsets, taps, the input."""
    x = np.asarray(x, dtype=np.float64)
    fwd = rs.forward(im2col(x, offsets, taps), w, b, bn, act, slope)
    fwd.update(offsets=np.asarray(offsets, dtype=np.int64), taps=int(taps), input=x)
    return fwd


def backward(fwd, gy, slope=SLOPE):
    """-> ref_seg_grad.backward with gx [rows, C] in the row numbering of x (rows no utterance owns: zero)."""
    bwd = rs.backward(fwd, gy, slope)
    bwd["gX"] = bwd["gx"]
    bwd["gx"] = col2im(bwd["gX"], fwd["offsets"], fwd["taps"], fwd["input"].shape[0], fwd["input"].shape[1])
    return bwd


def bounds(fwd, bwd=None):
    """The header of csrc/tconv_grad.hip -> dict of per-element bounds: z, h, y, and with `bwd` gx, gw, gbias, ggamma, gbeta."""
    out = rs.bounds(fwd, bwd)
    if bwd is None:
        return out
    X, w, bn, act = fwd["x"], fwd["w"], fwd["bn"], fwd["act"]
    n, N, W = X.shape[0], w.shape[0], fwd["taps"]
    a, gz = np.abs(bwd["a"]), np.abs(bwd["gz"])
    ba = 2.0 * U * a if act == LRELU else np.zeros_like(a)
    bg = ba if bn is None else np.abs(bn[0] * fwd["r"])[None, :] * ba + 3.01 * U * gz
    out["gw"] = bg.T @ np.abs(X) + (n + 64) * U * (gz.T @ np.abs(X))
    rows, C = fwd["input"].shape
    out["gx"] = col2im(bg @ np.abs(w) + (W * (N + 3) + 2) * U * (gz @ np.abs(w)), fwd["offsets"], W, rows, C)
    return out


# ---------------------------------------------------------------------------------------------- the stated orders in float32
def split_of(total_out, K, N):
    """tc_split of csrc/tconv_grad.hip: (rows per range, ranges) of the chain of gw."""
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    want = max(1, min(512 // tiles, 32, (total_out + 255) // 256))
    rows = ((total_out + want - 1) // want + 31) // 32 * 32
    return rows, (total_out + rows - 1) // rows


def _chain(A, B):
    """sum_k A[:, k, None] * B[None, k, :]... as one float32 fma chain over k ascending: A [m, K], B [K, n] float32 -> [m, n]."""
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=F)
    for k in range(A.shape[1]):
        acc = (acc.astype(np.float64) + A[:, k:k + 1].astype(np.float64) * B[k:k + 1, :].astype(np.float64)).astype(F)
    return acc


def emulate(x, offsets, taps, w, b, bn, act, gy):
    """A float32 evaluation in the orders include/xvec_hip.h states (k ascending; tau then j; rows ascending in the ranges of
    split_of, the ranges added in order; column sums in double) -> dict(z, y, gx, gw, gbias, ggamma, gbeta)."""
    x, w, b, gy = (np.asarray(v, dtype=F) for v in (x, w, b, gy))
    X = im2col(x, offsets, taps)
    n, K = X.shape
    N = w.shape[0]
    z = (_chain(X, w.T.copy()) + b[None, :]).astype(F)
    if bn is None:
        h, s, r = z, None, None
    else:
        gamma, beta, mm, mv = (np.asarray(v, dtype=F) for v in bn)
        r = (1.0 / np.sqrt(mv.astype(np.float64) + rs.EPS)).astype(F)
        s = (gamma * r).astype(F)
        d = (z - mm[None, :]).astype(F)
        h = (s[None, :].astype(np.float64) * d.astype(np.float64) + beta[None, :].astype(np.float64)).astype(F)
    y = h if act == NONE else np.where(h > 0, h, F(0) if act == RELU else (F(0.2) * h).astype(F)).astype(F)
    a = gy if act == NONE else np.where(h > 0, gy, F(0) if act == RELU else (F(0.2) * gy).astype(F)).astype(F)
    gz = a if bn is None else (a * s[None, :]).astype(F)
    out = dict(z=z, y=y, ggamma=None, gbeta=None)
    if bn is not None:
        out["gbeta"] = a.astype(np.float64).sum(axis=0).astype(F)
        out["ggamma"] = (a.astype(np.float64) * (r[None, :].astype(np.float64) * (z.astype(np.float64) - mm[None, :]))).sum(axis=0).astype(F)
    out["gbias"] = gz.astype(np.float64).sum(axis=0).astype(F)
    rows, S = split_of(n, K, N)
    gw = None
    for i in range(S):
        part = _chain(gz[i * rows:(i + 1) * rows].T.copy(), X[i * rows:(i + 1) * rows])
        gw = part if gw is None else (gw + part).astype(F)
    out["gw"] = gw
    # gx: for every input row the chain over tau ascending, then j ascending
    off, oo = np.asarray(offsets, dtype=np.int64), out_offsets(offsets, taps)
    C = x.shape[1]
    gx = np.zeros(x.shape, dtype=F)
    for bi in range(off.size - 1):
        n_in, n_out = int(off[bi + 1] - off[bi]), int(oo[bi + 1] - oo[bi])
        G = np.zeros((n_in, taps * N), dtype=F)
        for tau in range(taps):
            lo, hi = tau, min(tau + n_out, n_in)
            if hi > lo:
                G[lo:hi, tau * N:(tau + 1) * N] = gz[oo[bi]:oo[bi] + hi - lo]
        Wp = np.concatenate([w[:, tau * C:(tau + 1) * C] for tau in range(taps)], axis=0)      # [taps N, C]
        gx[off[bi]:off[bi + 1]] = _chain(G, Wp)
    out["gx"] = gx
    return out


def f32(a):
    return np.asarray(a, dtype=F)
