"""The rule of xv_gconv_forward / xv_gconv_backward and of xv_add_act_* (include/xvec_hip.h) in float64 numpy, and the
per-element error bound derived in the header of csrc/gconv_grad.hip restated as bounds().

A grid convolution on packed utterances is the dense layer of ref_seg_grad on the gathered matrix X [rows_out, kh kw C]:
X[o, tap C + c] = x[idx[o, tap], c] with idx from ref_grid.gather_windows (-1 = a padding zero of TensorFlow's 'same'); its
input gradient is the col2im of the dense layer's.  forward() builds X explicitly (the kernels never do).  Values are packed,
unpadded rows [sum(L) F, C] -- utterance, frame, bin.  The rule is checked against torch.autograd of F.pad + F.conv2d + eval-mode
batch_norm + relu / leaky_relu(0.2) in float64 (tests/test_gconv_host.py)."""
import numpy as np

import ref_grid as rgd
import ref_seg_grad as rs

U = rs.U
F = np.float32
NONE, RELU, LRELU = rs.NONE, rs.RELU, rs.LRELU
SLOPE = rs.SLOPE


def out_lens(lens, kh, st):
    """Frames per utterance behind a convolution with `st` along time: TensorFlow's 'same'."""
    return [rgd.same_pad(int(n), kh, st)[0] for n in lens]


def gather(x, idx):
    """x [rows, C], idx [rows_out, T] -> X [rows_out, T C], k = tap C + c; row -1 is the zero border."""
    xz = np.concatenate([x, np.zeros((1, x.shape[1]), dtype=x.dtype)])
    return xz[idx].reshape(idx.shape[0], idx.shape[1] * x.shape[1])


def col2im(G, idx, rows, C):
    """G [rows_out, T C] -> [rows, C]: every element added to the input row and channel it was read from."""
    out = np.zeros((rows, C), dtype=G.dtype)
    for t in range(idx.shape[1]):
        ok = idx[:, t] >= 0
        np.add.at(out, idx[ok, t], G[ok, t * C:(t + 1) * C])
    return out


def forward(x, lens, F_in, window, w, b=None, bn=None, act=NONE, slope=SLOPE):
    """x [sum(lens) F_in, C], window = (kh, kw, st, sf), w [N, kh kw C] rows, b [N] or None -> ref_seg_grad.forward of the
    gathered matrix, plus idx, lens, out_lens, F_out, window, the input."""
    x = np.asarray(x, dtype=np.float64)
    kh, kw, st, sf = window
    idx, olens, F_out = rgd.gather_windows(lens, F_in, kh, kw, st, sf)
    w = np.asarray(w, dtype=np.float64)
    fwd = rs.forward(gather(x, idx), w, np.zeros(w.shape[0]) if b is None else b, bn, act, slope)
    fwd.update(idx=idx, lens=[int(n) for n in lens], out_lens=olens, F_in=int(F_in), F_out=int(F_out), window=tuple(window), input=x,
               has_bias=b is not None)
    return fwd


def backward(fwd, gy, slope=SLOPE):
    """-> ref_seg_grad.backward with gx [rows, C] in the row numbering of x."""
    bwd = rs.backward(fwd, gy, slope)
    bwd["gX"] = bwd["gx"]
    bwd["gx"] = col2im(bwd["gX"], fwd["idx"], fwd["input"].shape[0], fwd["input"].shape[1])
    return bwd


def bounds(fwd, bwd=None):
    """The header of csrc/gconv_grad.hip -> dict of per-element bounds: z, h, y, and with `bwd` gx, gw, gbias, ggamma, gbeta."""
    out = rs.bounds(fwd, bwd)
    if bwd is None:
        return out
    X, w, bn, act = fwd["x"], fwd["w"], fwd["bn"], fwd["act"]
    n, N, T = X.shape[0], w.shape[0], fwd["idx"].shape[1]
    a, gz = np.abs(bwd["a"]), np.abs(bwd["gz"])
    ba = 2.0 * U * a if act == LRELU else np.zeros_like(a)
    bg = ba if bn is None else np.abs(bn[0] * fwd["r"])[None, :] * ba + 3.01 * U * gz
    out["gw"] = bg.T @ np.abs(X) + (n + 64) * U * (gz.T @ np.abs(X))
    rows, C = fwd["input"].shape
    out["gx"] = col2im(bg @ np.abs(w) + (T * (N + 3) + 2) * U * (gz @ np.abs(w)), fwd["idx"], rows, C)
    return out


def split_of(rows_out, K, N):
    """gc_split of csrc/gconv_grad.hip: (rows per range, ranges) of the chain of gw."""
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    want = max(1, min((1024 + tiles - 1) // tiles, 256, (rows_out + 1023) // 1024))
    rows = ((rows_out + want - 1) // want + 31) // 32 * 32
    return rows, (rows_out + rows - 1) // rows


def unread_inputs(fwd):
    """bool [rows]: the input rows no output bin reads (their gx is an exact zero)."""
    read = np.zeros(fwd["input"].shape[0], dtype=bool)
    read[fwd["idx"][fwd["idx"] >= 0]] = True
    return ~read


# ---------------------------------------------------------------------------------------------- the residual join
def _act32(s, v, act):
    """v where s > 0, else the lower branch of `act` applied to v, in float32 (v = s: the activation; v = gy: its gradient)."""
    if act == NONE:
        return v
    return np.where(s > 0, v, F(0) if act == RELU else (F(0.2) * v).astype(F)).astype(F)


def add_act(p, q, act):
    """xv_add_act_forward in numpy float32: one addition, then the activation."""
    s = (np.asarray(p, dtype=F) + np.asarray(q, dtype=F)).astype(F)
    return _act32(s, s, act)


def add_act_grad(gy, p, q, act):
    """xv_add_act_backward in numpy float32: gy act'(p + q), zero in the lower branch."""
    s = (np.asarray(p, dtype=F) + np.asarray(q, dtype=F)).astype(F)
    return _act32(s, np.asarray(gy, dtype=F), act)


def f32(a):
    return np.asarray(a, dtype=F)
