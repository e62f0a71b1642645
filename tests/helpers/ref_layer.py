"""Float64 reference of one frame-layer GEMM on the GPU's own fp32 input, with a per-element error bar.

Restates the library's rules (csrc/api_weights.hip upload_layer / act_exponent / host_quant32, csrc/xv_common.h split2t, csrc/xv_epilogue_n32.h the
folded epilogue, csrc/xv_f6.h): how a layer's weights and its fp32 input are split into the operands its kernel multiplies, and
which float scale / shift its epilogue applies.  The operands are exactly representable, so

    model = sum of the operand products, in float64                      (terms(), model_acc())
      f32                 x w
      bf16x3 / f16x3      a_lo w_hi + a_hi w_lo + a_hi w_hi               (the order of csrc/gemm_bf16x3.hip's K step)
      f16f6, two-unit     q6(a_hi) q6(w_lo) + q6(a_lo) q6(w_hi) + a_hi w_hi

is what the kernel would return with an exact accumulator, and everything the GPU adds is the rounding of its fp32 accumulation:

    bar_acc = lambda u sqrt(sum_i S_i^2),   u = 2^-24                     (sum_sq_partials(), hoeffding_lambda())

S_i the float64 partial sum after accumulation step i: K block by K block (32 channels of one tap), the split terms in turn, one
step per non-zero product.  That is Hoeffding's bound for independent, mean-zero roundings of at most u relative each, at a total
failure probability p over the N elements a whole test file checks: lambda = sqrt(2 ln(2 N / p)).  v_mfma_f32_32x32x2_f32 is a
k-ordered fmaf chain, so for fp32 a step is one product by construction; for the 16-bit and the block-scaled MFMAs it is not
documented whether the sum inside an instruction rounds per product, and the bar takes the per-product model for them as well
(more steps: the larger bar).  A stage endpoint v = fmaf(acc, scale, shift) adds one rounding: bar = |scale| bar_acc + u |v|.

Plain numpy, float64.  sum_sq_partials() uses only operations that numpy arrays and torch tensors share, so that the GPU test may
hand it float64 tensors on the device (the sweep is O(rows N K) with a square after every product; the values do not change)."""
import itertools

import numpy as np

U = 2.0 ** -24
P_FAIL = 1e-6
PRECISIONS = ("f32", "bf16x3", "f16x3", "f16f6")
BN_EPS = 1e-3


def hoeffding_lambda(n_elements, p=P_FAIL):
    return float(np.sqrt(2.0 * np.log(2.0 * float(n_elements) / p)))


# ------------------------------------------------------------------------------------------------------ number formats
def rn_bf16(x):
    """Round to nearest even to bfloat16 (f32_to_bf16_rn / v_cvt_pk_bf16_f32); float64 in and out."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32).astype(np.float64)


def rn_f16(x):
    """IEEE binary16, round to nearest even, subnormals kept, overflow to inf."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def e8m0_exponent(amax):
    """e of the block scale 2^e (e8m0_of / host_quant32): ceil(log2(amax / 7.5)) as the float code computes it, 0 for amax = 0."""
    a = np.ascontiguousarray(amax, dtype=np.float32)
    r = a * np.float32(1.0 / 7.5)
    e = ((r.view(np.uint32).astype(np.int64) + 0x7FFFFF) >> 23) - 127
    return np.where(a > 0, np.clip(e, -126, 126), 0)


def _blocks(v):
    v = np.asarray(v, dtype=np.float64)
    assert v.shape[-1] % 32 == 0
    return v.reshape(v.shape[:-1] + (v.shape[-1] // 32, 32))


def _decode(c):
    ef, m = c >> 3, c & 7
    return np.where(ef == 0, m / 8.0, (1.0 + m / 8.0) * 2.0 ** (ef - 1.0))


def q6_half_up(v):
    """e2m3 under one E8M0 scale per 32 values of the last axis, magnitudes rounded half up: host_e2m3 / e2m3_code bit for bit
    (the weight packer, and f6_from_sb_kernel)."""
    b = _blocks(v)
    e = e8m0_exponent(np.abs(b).max(-1))[..., None]
    ax = np.minimum((np.abs(b) * 2.0 ** (-e.astype(np.float64))).astype(np.float32), np.float32(7.5))
    sub = ax < 1
    t = np.where(sub, ax + np.float32(1.0), ax).astype(np.float32)
    c = ((t.view(np.uint32).astype(np.int64) + 0x80000) >> 20) - (126 << 3) - np.where(sub, 8, 0)
    c = np.minimum(c, 31)
    return (np.sign(b) * _decode(c) * 2.0 ** e).reshape(np.shape(v))


def q6_rne(v):
    """The same grid and scale, magnitudes rounded to nearest even and saturated at 7.5: what csrc/xv_f6.h says of the hardware
    converters v_cvt_scalef32_pk32_fp6_f16 / v_cvt_scalef32_2xpk16_fp6_f32 (the activations of a two-unit layer)."""
    b = _blocks(v)
    e = e8m0_exponent(np.abs(b).max(-1))[..., None].astype(np.float64)
    ax = np.abs(b) * 2.0 ** -e
    ex = np.maximum(np.floor(np.log2(np.maximum(ax, 2.0 ** -10))), 0.0)
    step = 2.0 ** (ex - 3.0)
    q = np.minimum(np.round(ax / step) * step, 7.5)          # np.round: half to even
    return (np.sign(b) * q * 2.0 ** e).reshape(np.shape(v))


# --------------------------------------------------------------------------------------------- the library's own rules
def bn_fold(weights, scope):
    """s = gamma / sqrt(var + eps), t = beta - mean s, in double as bn_fold of csrc/api_weights.hip."""
    g, b, m, v = (np.asarray(weights[scope + "/" + k], dtype=np.float32).astype(np.float64)
                  for k in ("gamma", "beta", "moving_mean", "moving_variance"))
    s = g / np.sqrt(v + BN_EPS)
    return s, b - m * s


def act_exponent(weights, bn_scope, act="relu"):
    """Power of two the split copy of a layer's output is kept at (fp16 formats): floor(4.5 - log2 rms(gamma, beta)), +-20;
    0 without a normalisation and for tanh."""
    if bn_scope is None or act == "tanh":
        return 0
    g = np.asarray(weights[bn_scope + "/gamma"], dtype=np.float32).astype(np.float64)
    b = np.asarray(weights[bn_scope + "/beta"], dtype=np.float32).astype(np.float64)
    rms = np.sqrt((g * g + b * b).sum() / max(g.size, 1))
    if not (rms > 0 and np.isfinite(rms)):
        return 0
    return int(min(20.0, max(-20.0, np.floor(4.5 - np.log2(rms)))))


def wscale(kernel):
    """2^(14 - e), frexp(max |w|) = m 2^e, exponent clamped to +-24: the largest fp16 weight lands in [8192, 16384)."""
    maxabs = float(np.abs(np.asarray(kernel, dtype=np.float32)).max())
    if not (maxabs > 0 and np.isfinite(maxabs)):
        return 1.0
    return float(np.ldexp(1.0, min(max(14 - int(np.frexp(maxabs)[1]), -24), 24)))


def arithmetic(precision, frame_level, two_unit):
    """Which product a layer runs in: the segment-level layers are fp32 in every precision (choose_kernels: use_split needs a
    frame-level input), a two-unit layer is what Trainer.runs_two_unit says, every other layer of f16f6 is f16x3."""
    if precision == "f32" or not frame_level:
        return "f32"
    if precision == "f16f6":
        return "f16f6" if two_unit else "f16x3"
    return precision


def kernel_matrix(kernel, cin_pad=None):
    """[w, cin(_pad), cout] float64 of a conv ([1, w, cin, cout] / [w, cin, cout]) or dense ([cin, cout]) variable."""
    k = np.asarray(kernel, dtype=np.float32).astype(np.float64)
    if k.ndim == 4:
        k = k[0]
    if k.ndim == 2:
        k = k[None]
    if cin_pad and cin_pad > k.shape[1]:
        k = np.concatenate([k, np.zeros((k.shape[0], cin_pad - k.shape[1], k.shape[2]))], axis=1)
    return k


def split_weights(k3, arith):
    """name -> [w, cin, cout] operand of the kernel: the scaled weights as uploaded; `ws` the layer's power of two."""
    if arith == "f32":
        return {"w": k3, "ws": 1.0}
    if arith == "bf16x3":
        hi = rn_bf16(k3)
        return {"wh": hi, "wl": rn_bf16(k3 - hi), "ws": 1.0}
    ws = wscale(k3)
    s = f32(k3 * ws)
    hi = rn_f16(s)
    if arith == "f16x3":
        return {"wh": hi, "wl": rn_f16(s - hi), "ws": ws}
    lo = s - hi                                   # unrounded; the codes are per (32-channel block, tap, column)
    q = lambda v: np.moveaxis(q6_half_up(np.moveaxis(v, 1, -1)), -1, 1)      # noqa: E731
    return {"wh": hi, "q6wl": q(lo), "q6wh": q(hi), "ws": ws}


def split_acts(x, arith, exponent=0, quantiser=q6_rne):
    """name -> [rows, cin] operand from an fp32 input x (cin a multiple of 32 for the split formats); `exponent` is the producer's
    act_exponent (0 for input features, and unused by f32 / bf16x3)."""
    x = f32(x)
    if arith == "f32":
        return {"x": x}
    if arith == "bf16x3":
        hi = rn_bf16(x)
        return {"ah": hi, "al": rn_bf16(x - hi)}
    s = f32(x * 2.0 ** exponent)
    hi = rn_f16(s)
    if arith == "f16x3":
        return {"ah": hi, "al": rn_f16(s - hi)}
    lo = s - hi
    return {"ah": hi, "q6ah": quantiser(hi), "q6al": quantiser(lo)}


TERMS = {"f32": (("x", "w"),),
         "bf16x3": (("al", "wh"), ("ah", "wl"), ("ah", "wh")),
         "f16x3": (("al", "wh"), ("ah", "wl"), ("ah", "wh")),
         "f16f6": (("q6ah", "q6wl"), ("q6al", "q6wh"), ("ah", "wh"))}


def pad32(x):
    x = np.asarray(x)
    pad = (-x.shape[1]) % 32
    return np.concatenate([x, np.zeros((x.shape[0], pad), dtype=x.dtype)], axis=1) if pad else x


def gather_rows(in_offsets, w):
    """[rows_out, w] input row of every (output row, tap) of a 'valid' convolution over packed utterances, and the output
    offsets: output frame t of an utterance reads its input frames t .. t + w - 1."""
    idx, out_offs = [], [0]
    for b in range(len(in_offsets) - 1):
        n = int(in_offsets[b + 1] - in_offsets[b]) - (w - 1)
        assert n >= 1
        idx.append(int(in_offsets[b]) + np.arange(n)[:, None] + np.arange(w)[None, :])
        out_offs.append(out_offs[-1] + n)
    return np.concatenate(idx), np.asarray(out_offs)


def terms(acts, wts, arith, rows):
    """The term pairs (A [rows_out, w cin], W [w cin, cout]) of `arith`, K tap-major; `rows` from gather_rows."""
    out = []
    for an, wn in TERMS[arith]:
        a, w3 = acts[an], wts[wn]
        A = np.concatenate([a[rows[:, j]] for j in range(rows.shape[1])], axis=1)
        out.append((A, w3.reshape(-1, w3.shape[2])))
    return out


def model_acc(tms):
    return sum(A @ W for A, W in tms)


def sum_sq_partials(tms, block=32, max_elems=1 << 24):
    """sum_i S_i^2 per output element: K blocks of `block` in order, the terms in turn, one step per non-zero product.
    Works on numpy arrays and on torch tensors alike."""
    A0, W0 = tms[0]
    M, K, N = A0.shape[0], A0.shape[1], W0.shape[1]
    step = max(1, max_elems // (block * N))
    parts = []
    for r0 in range(0, M, step):
        S = (A0[r0:r0 + step, :1] @ W0[:1]) * 0.0
        Q = S * 0.0
        for k0 in range(0, K, block):
            for A, W in tms:
                P = A[r0:r0 + step, k0:k0 + block, None] * W[None, k0:k0 + block, :]
                C = P.cumsum(1) + S[:, None, :]
                Q = Q + (C * C * (P != 0)).sum(1)
                S = C[:, -1, :]
        parts.append(Q)
    if isinstance(parts[0], np.ndarray):
        return np.concatenate(parts)
    import torch
    return torch.cat(parts)


def bar_acc(sumsq, lam):
    return lam * U * np.sqrt(np.asarray(sumsq, dtype=np.float64))


# ------------------------------------------------------------------------------------------------------------ epilogue
def epilogue_vectors(weights, kernel_name, bias_name, bn_scope, ws=1.0, in_exp=0):
    """The float vectors of upload_layer: {stage: (scale, shift)} for the '_conv' / '_dense' endpoint (ones, bias), and '_bn'
    (folded normalisation); 1 / ws and 2^-in_exp folded into the multipliers (exact)."""
    bias = np.asarray(weights[bias_name], dtype=np.float32)
    n = bias.shape[0]
    inv = np.float32(np.ldexp(1.0 / ws, -in_exp))
    out = {"affine": (np.ones(n, np.float32) * inv, bias)}
    if bn_scope is not None:
        s, t = bn_fold(weights, bn_scope)
        out["bn"] = (s.astype(np.float32) * inv, (bias.astype(np.float64) * s + t).astype(np.float32))
    else:
        out["bn"] = out["affine"]
    return out


def stage(acc, scale, shift, act=None, alpha=None):
    """v = fmaf(acc, scale, shift) in float64 on the float vectors, then the activation (apply_act)."""
    v = acc * scale.astype(np.float64) + shift.astype(np.float64)
    if act == "relu":
        return np.maximum(v, 0.0), v
    if act == "prelu":
        return np.maximum(v, 0.0) + alpha.astype(np.float64) * (v - np.abs(v)) * 0.5, v
    return v, v


def stage_bar(bacc, scale, pre, act=None):
    """|scale| bar_acc + u |v| on the pre-activation v (the one rounding of the fmaf; ReLU is 1-Lipschitz and rounds nothing);
    PReLU's three rounded operations (alpha d, * 0.5 is exact, the sum, and fmaxf exact: two) add u |v| each."""
    b = np.abs(scale.astype(np.float64)) * bacc + U * np.abs(pre)
    return b + 2 * U * np.abs(pre) if act == "prelu" else b


# ----------------------------------------------------------------------------------------------------- fp32 emulations
def emulate(tms, per_product, reverse=False, block=32):
    """An fp32 accumulator over the same operands: one rounding per (32-block, term) or one per product; K blocks forward or
    backward."""
    A0, W0 = tms[0]
    acc = np.zeros((A0.shape[0], W0.shape[1]), dtype=np.float32)
    starts = list(range(0, A0.shape[1], block))
    for k0 in (reversed(starts) if reverse else starts):
        for A, W in tms:
            if per_product:
                for k in range(k0, min(k0 + block, A.shape[1])):
                    acc = (acc.astype(np.float64) + np.outer(A[:, k], W[k])).astype(np.float32)
            else:
                acc = (acc.astype(np.float64) + A[:, k0:k0 + block] @ W[k0:k0 + block]).astype(np.float32)
    return acc


def emulate_stage(acc32, scale, shift, act=None):
    v = (acc32.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)      # one rounding: fmaf
    return np.maximum(v, np.float32(0)) if act == "relu" else v


# ------------------------------------------------------------------------------------------------------ exact selection
def selection_kernel(w, cin, cout, value, valid_cin=None):
    """[w, cin, cout] with exactly one non-zero entry per output channel: output n reads (tap, block) pair n mod (w nb) at
    position n mod 32 of the block (n mod the valid positions of a partial block)."""
    nb = (cin + 31) // 32
    k = np.zeros((w, cin, cout), dtype=np.float32)
    used = []
    for n in range(cout):
        p = n % (w * nb)
        tap, blk = p % w, p // w
        width = min(32, (valid_cin or cin) - 32 * blk)
        c = 32 * blk + n % width
        k[tap, c, n] = value
        used.append((tap, blk, c % 32))
    return k, used


def selection_predictions(tms, orders=None, exact_products=True):
    """fp32 accumulators of a selection layer: every output has at most one non-zero product per term, so the accumulator is
    those (exactly representable) products added in fp32, one rounding per addition, in the term order of the kernel -- or, for
    `orders` = 'any', the set of results over all orders (a stack [n_orders, rows, cout])."""
    prods = []
    for A, W in tms:
        p = A @ W                                   # one non-zero product per output: exact in float64
        assert not exact_products or np.array_equal(p.astype(np.float32).astype(np.float64), p), "a product is not an fp32 number"
        prods.append(p)
    perms = [tuple(range(len(prods)))] if orders is None else list(itertools.permutations(range(len(prods))))
    out = []
    for perm in perms:
        acc = np.zeros_like(prods[0], dtype=np.float32)
        for i in perm:
            acc = (acc.astype(np.float64) + prods[i]).astype(np.float32)
        out.append(acc)
    return np.stack(out)
