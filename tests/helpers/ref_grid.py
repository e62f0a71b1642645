"""Float64 reference of one ResNet convolution on the GPU's own fp32 input, with a per-element error bar.

The arithmetic is tests/helpers/ref_layer.py's (splits, fp6 quantisers, term lists, sum_sq_partials, stage / stage_bar); this file
adds what the grid path has and the frame layers do not:

    gather_windows()    the 2-D gather: for every output bin the packed input row of each (kh, kw) tap, -1 where TensorFlow's 'same'
                        padding supplies a zero -- placement as oracle/ref_numpy.conv2d: before = pad_total // 2, so under stride 2 an
                        even size pads 0 / 1 and an odd size 1 / 1, along time (per utterance) and frequency independently
    terms()             rl.TERMS on the gathered operand, K = (kh, kw, cin) as the kernels walk it (csrc/api_forward.hip gemm_args:
                        three taps along time over the 3 cin contiguous channels of a kernel row; HWIO flattened)
    residual_stage()    v = fmaf(acc, scale, shift), then v + R (one more fp32 rounding), then the activation
                        (csrc/xv_epilogue.h `if (p.R)`, csrc/gemm_f32.hip splitk_reduce_kernel, csrc/xv_f6.h store_wave_tile_n32_res)
    conv0_direct()      conv0_direct_kernel (csrc/grid.hip): nine fp32 fmaf in (kh, kw) order, fmaf(v, scale, shift), the activation
    maxpool3x3()        grid_maxpool3x3_kernel: the maximum over the neighbours inside the map; the zero border takes no part

Values live as packed, unpadded rows [sum(L) F, C] -- utterance, frame, bin -- which is what Trainer.predict_packed returns for a
grid node.  Plain numpy, float64."""
import numpy as np

import ref_layer as rl

U = rl.U
LRELU = float(np.float32(0.2))            # kLreluAlpha as the kernels hold it


# ------------------------------------------------------------------------------------------------------------- the gather
def same_pad(n, k, s):
    """(output size, zeros in front) of TensorFlow's 'same' padding."""
    out = -(-n // s)
    return out, max((out - 1) * s + k - n, 0) // 2


def gather_windows(in_lens, F_in, kh, kw, st, sw, padding="same", pad_before=None, clip_time=True):
    """-> (idx [rows_out, kh kw] int64, out_lens, F_out): packed input row of every tap of every output bin, -1 = a padding zero.
    `pad_before` = (time, frequency) overrides the zeros in front and `clip_time=False` drops the test against the utterance's
    own first / last frame: the two faults tests/test_grid_bars_host.py injects."""
    idx, out_lens, base, F_out = [], [], 0, None
    total = int(sum(in_lens)) * F_in
    for L in in_lens:
        L = int(L)
        if padding == "same":
            Lo, pt = same_pad(L, kh, st)
            F_out, pf = same_pad(F_in, kw, sw)
        else:
            Lo, pt, F_out, pf = (L - kh) // st + 1, 0, (F_in - kw) // sw + 1, 0
        if pad_before is not None:
            pt, pf = pad_before
        t = np.arange(Lo)[:, None, None, None] * st - pt + np.arange(kh)[None, None, :, None]
        f = np.arange(F_out)[None, :, None, None] * sw - pf + np.arange(kw)[None, None, None, :]
        row = base + t * F_in + f
        ok = (f >= 0) & (f < F_in) & ((t >= 0) & (t < L) if clip_time else (row >= 0) & (row < total))
        idx.append(np.where(ok, row, -1).reshape(Lo * F_out, kh * kw))
        out_lens.append(Lo)
        base += L * F_in
    return np.concatenate(idx).astype(np.int64), out_lens, F_out


def kernel_taps(kernel, cin_pad=None):
    """[kh kw, cin(_pad), cout] float64 of an HWIO variable ([cin, cout] of a dense layer: one tap)."""
    k = np.asarray(kernel, dtype=np.float32).astype(np.float64)
    k = k.reshape((-1,) + k.shape[-2:])
    if cin_pad and cin_pad > k.shape[1]:
        k = np.concatenate([k, np.zeros((k.shape[0], cin_pad - k.shape[1], k.shape[2]))], axis=1)
    return k


def terms(acts, wts, arith, idx, kpad=None):
    """The term pairs (A [rows_out, taps cin], W [taps cin, cout]) of `arith` on the gathered operand; `kpad`: K zero-padded (conv0's
    nine taps in a K of 32)."""
    out = []
    for an, wn in rl.TERMS[arith]:
        a, w3 = acts[an], wts[wn]
        az = np.concatenate([a, np.zeros((1, a.shape[1]))])                   # row -1: the zero border
        A = az[idx].reshape(idx.shape[0], idx.shape[1] * a.shape[1])
        W = w3.reshape(-1, w3.shape[2])
        if kpad and kpad > A.shape[1]:
            A = np.concatenate([A, np.zeros((A.shape[0], kpad - A.shape[1]))], axis=1)
            W = np.concatenate([W, np.zeros((kpad - W.shape[0], W.shape[1]))])
        out.append((A, W))
    return out


# ----------------------------------------------------------------------------------------------------------- the epilogue
def vectors(weights, bn_scope, cout, bias=None, ws=1.0, in_exp=0):
    """(scale, shift) float32 of upload_layer's folded normalisation; the ResNet convolutions have no bias (conv5 and the dense
    layers do)."""
    w = dict(weights)
    w["__bias__"] = np.zeros(cout, np.float32) if bias is None else np.asarray(bias, np.float32)
    return rl.epilogue_vectors(w, None, "__bias__", bn_scope, ws, in_exp)["bn"]


def activate(v, act, alpha=None):
    """apply_act (csrc/xv_common.h) in float64."""
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "lrelu":
        return np.maximum(v, LRELU * v)
    if act == "prelu":
        return np.maximum(v, 0.0) + np.asarray(alpha, np.float32).astype(np.float64) * (v - np.abs(v)) * 0.5
    return v


def act_lipschitz(act, alpha=None):
    if act == "prelu":
        return np.maximum(1.0, np.abs(np.asarray(alpha, np.float32).astype(np.float64)))
    return 1.0


def act_bar(pre, act):
    """The activation's own roundings: none for ReLU (fmaxf), the one product 0.2 v of the leaky ReLU, and for PReLU what
    rl.stage_bar counts (alpha d and the sum: u |v| each)."""
    if act == "lrelu":
        return U * np.abs(LRELU * pre)
    if act == "prelu":
        return 2 * U * np.abs(pre)
    return 0.0


def residual_stage(acc, scale, shift, R=None, act=None, alpha=None):
    """-> (value, v = acc scale + shift, v + R): float64 on the float vectors; R the fp32 endpoint the GPU returned."""
    v = acc * scale.astype(np.float64) + shift.astype(np.float64)
    s = v if R is None else v + np.asarray(R, np.float32).astype(np.float64)
    return activate(s, act, alpha), v, s


def residual_bar(bacc, scale, v, s, R=None, act=None, alpha=None):
    """|scale| bar_acc + u |v| (the fmaf) + u |v + R| (the add, when there is a residual), carried through the activation (Lipschitz
    1, or |alpha| of a PReLU channel beyond 1), plus the activation's own roundings."""
    b = np.abs(scale.astype(np.float64)) * bacc + U * np.abs(v)
    if R is not None:
        b = b + U * np.abs(s)
    return b * act_lipschitz(act, alpha) + act_bar(s, act)


def emulate_residual(acc32, scale, shift, R=None, act=None, alpha=None, after=False):
    """The fp32 epilogue: fmaf, the fp32 add, apply_act with fp32 operations.  `after`: the residual added BEHIND the activation (a
    fault)."""
    f = np.float32
    v = (acc32.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(f)

    def a32(x):
        if act == "relu":
            return np.maximum(x, f(0))
        if act == "lrelu":
            return np.maximum(x, (f(LRELU) * x).astype(f))
        if act == "prelu":
            d = (x - np.abs(x)).astype(f)
            return (np.maximum(x, f(0)) + ((np.asarray(alpha, f) * d).astype(f) * f(0.5)).astype(f)).astype(f)
        return x
    if R is None:
        return a32(v)
    R = np.asarray(R, f)
    return (a32(v) + R).astype(f) if after else a32((v + R).astype(f))


# ------------------------------------------------------------------------------------------------------------------ conv0
def conv0_direct(x_rows, idx, kernel, scale, shift, act=None, alpha=None):
    """conv0_direct_kernel on the packed feature bins x_rows [sum(L) F]: (value, bar) [rows, cout].  The accumulator is nine fmaf
    in (kh, kw) order: |error| <= u sum_i |S_i| to first order (S_i the exact partial sums; 1 + 16 u covers the higher orders of a
    nine-step chain), then the stage as everywhere: |scale| that + u |v|, the activation."""
    xz = np.concatenate([rl.f32(x_rows).reshape(-1), [0.0]])
    A = xz[idx]                                                              # [rows, 9]
    W = np.asarray(kernel, np.float32).astype(np.float64).reshape(9, -1)
    P = A[:, :, None] * W[None]
    S = P.cumsum(1)
    acc, eacc = S[:, -1], U * np.abs(S).sum(1) * (1 + 16 * U)
    val, v, _ = residual_stage(acc, scale, shift, None, act, alpha)
    bar = (np.abs(scale.astype(np.float64)) * eacc + U * np.abs(v)) * act_lipschitz(act, alpha) + act_bar(v, act)
    return val, bar


def emulate_conv0_direct(x_rows, idx, kernel, scale, shift, act=None, alpha=None):
    f = np.float32
    xz = np.concatenate([np.asarray(x_rows, f).reshape(-1), [f(0)]]).astype(f)
    A = xz[idx]
    W = np.asarray(kernel, f).reshape(9, -1)
    acc = np.zeros((A.shape[0], W.shape[1]), f)
    for k in range(9):
        acc = (A[:, k, None].astype(np.float64) * W[k][None].astype(np.float64) + acc.astype(np.float64)).astype(f)
    return emulate_residual(acc, scale, shift, None, act, alpha)


# --------------------------------------------------------------------------------------------------------------- max-pool
def maxpool3x3(x_rows, lens, F, border_takes_part=False):
    """3 x 3 'same' max-pool of packed rows [sum(L) F, C]: the maximum over the neighbours inside the map.
    `border_takes_part`: the padding zero joins the maximum (the fault a negative activation shows)."""
    idx, _, _ = gather_windows(lens, F, 3, 3, 1, 1)
    x = np.asarray(x_rows, dtype=np.float64)
    xz = np.concatenate([x, np.full((1, x.shape[1]), 0.0 if border_takes_part else -np.inf)])
    return xz[idx].max(axis=1)


def maxpool_interval(lo_rows, hi_rows, lens, F):
    """[max_i lo_i, max_i hi_i] over the clipped neighbourhood: where an exact max of values known to lo <= x <= hi must lie."""
    return maxpool3x3(lo_rows, lens, F), maxpool3x3(hi_rows, lens, F)
