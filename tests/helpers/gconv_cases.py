"""The inputs of tests/test_gpu_gconv.py, shared with the host test that checks the condition put on them
(tests/test_gconv_host.py).

As in tconv_cases.py the ReLU mask is a discontinuity, so that NO element ever has to be left out of a comparison every h of the
float64 oracle is exactly zero by construction (a column with gamma = beta = 0, or a zero of the dyadic family), of certain sign
by exactness (the dyadic family: x, w and b multiples of 1/8), or at least 64 of its own error bounds (ref_gconv.bounds, h) away
from zero.  An input bin takes part in up to nine output bins in two dimensions, so the random family cannot draw its rows in
order as tconv_cases does: it draws all of x, then repairs -- every output bin with an h too close to zero has one of the input
bins it reads redrawn, and the oracle is taken again, until none is left.  precondition() asserts the condition on the oracle
alone.  The seeds are fixed here; they were found on the CPU, with the float64 rule standing in for the device.

The cases cover the six windows the ResNet uses ((3, 3) and (1, 1), strides (1, 1), (1, 2) and (2, 2)); C = 1 (conv0_1), 3, 4
(16-byte rows), 33, 68; N = 1, 31, 33, 68; F_in = 1, 2, 5, 6, 7, 40 (odd and even under a stride: zeros in front 1 / 1 and 0 / 1);
63, 64 and 65 output rows (the edges of a 64-row tile) and `long` with 1120, the smallest kind of size at which the column sums
take a second slice and the chain of gw a second range (both beyond 1024 rows); utterances of 0, 1, 2, odd and even frame counts,
the empty one and the one-frame one in the middle of their batch."""
import numpy as np

import ref_gconv as rg
import ref_seg_grad as rs
import seg_grad_cases as sc

F = np.float32
MARGIN = sc.MARGIN

# (name, (kh, kw, st, sf), C, N, F_in, frames per utterance, bias, batch norm, activation, family, layout: "vec" = 16-byte rows
# where C allows, "odd" = every pitch beyond its width and every base 4 bytes off a 16-byte boundary)
CASES = [
    ("k33_s11_c4", (3, 3, 1, 1), 4, 33, 7, [5, 0, 1, 2, 4], False, True, rs.RELU, "random", "vec"),
    ("k33_s12_c3", (3, 3, 1, 2), 3, 31, 6, [7, 1, 0, 6, 7], True, True, rs.LRELU, "random", "odd"),             # 63 rows
    ("k33_s22_c33", (3, 3, 2, 2), 33, 68, 7, [9, 0, 1, 2, 8, 10], False, False, rs.RELU, "random", "vec"),      # 64 rows
    ("k11_s11_c68", (1, 1, 1, 1), 68, 1, 5, [6, 1, 0, 2, 4], True, True, rs.NONE, "random", "vec"),             # 65 rows
    ("k11_s12_c1", (1, 1, 1, 2), 1, 33, 2, [3, 0, 1, 2], False, True, rs.LRELU, "dyadic", "odd"),
    ("k11_s22_c4", (1, 1, 2, 2), 4, 31, 40, [3, 1, 0, 4], False, True, rs.RELU, "random", "vec"),
    ("k33_s11_c1", (3, 3, 1, 1), 1, 68, 40, [2, 1], False, True, rs.RELU, "random", "vec"),                      # conv0_1
    ("k33_s22_f1", (3, 3, 2, 2), 4, 33, 1, [5, 2], False, False, rs.LRELU, "dyadic", "vec"),
    ("k33_s12_c68", (3, 3, 1, 2), 68, 68, 5, [4, 3], True, False, rs.NONE, "random", "odd"),
    ("k33_s22_c4", (3, 3, 2, 2), 4, 31, 6, [4, 1, 0, 7], False, True, rs.LRELU, "random", "odd"),
    ("long", (3, 3, 1, 1), 4, 31, 40, [14, 0, 14], False, True, rs.LRELU, "random", "vec"),                      # 1120 rows
]
SEEDS = {c[0]: 700 + i for i, c in enumerate(CASES)}
ROUNDS = 400


def _oracle(c):
    return rg.forward(c["x"], c["lens"], c["F_in"], c["window"], c["w"], c["b"], c["bn"], c["act"])


def _near(c, fwd):
    """bool [rows_out]: the output bins with an h within MARGIN bounds of zero (the zero column apart)."""
    near = np.abs(fwd["h"]) < MARGIN * rs.bounds(fwd)["h"]
    if c["zero_col"] is not None:
        near[:, c["zero_col"]] = False
    return near.any(axis=1)


def make(name):
    """-> dict(x [sum(lens) F_in, C], lens, F_in, window, w [N, kh kw C], b or None, bn or None, act, gy [rows_out, N], family,
    layout, zero_col)."""
    _, window, C, N, F_in, lens, has_bias, has_bn, act, family, layout = next(c for c in CASES if c[0] == name)
    r = np.random.RandomState(SEEDS[name])
    kh, kw, st, sf = window
    K = kh * kw * C
    rows = int(sum(lens)) * F_in
    zero_col = None
    if family == "dyadic":
        x = (r.randint(-16, 17, (rows, C)) / 8.0).astype(F)
        w = (r.randint(-16, 17, (N, K)) / 8.0).astype(F)
        b = (r.randint(-16, 17, N) / 8.0).astype(F) if has_bias else None
        bn = None
        if not has_bn:
            x[:2 * F_in] = 0.0                                    # h = 0 exactly in the first bins: the zero of the lower branch
            if b is not None:
                b[0] = 0.0
        else:
            bn = sc._bn_random(r, N)
            bn[1] = np.zeros(N, dtype=F)
            bn[2] = (r.randint(-64, 64, N) / 64.0 + 1.0 / 128.0).astype(F)
    else:
        x = r.standard_normal((rows, C)).astype(F)
        w = (r.standard_normal((N, K)) / np.sqrt(K)).astype(F)
        b = (0.1 * r.standard_normal(N)).astype(F) if has_bias else None
        bn = sc._bn_random(r, N) if has_bn else None
    if has_bn and N > 1:
        zero_col = N // 2
        bn[0][zero_col] = 0.0
        bn[1][zero_col] = 0.0
    c = dict(name=name, x=x, lens=list(lens), F_in=F_in, window=window, w=w, b=b, bn=bn, act=act, family=family, layout=layout,
             zero_col=zero_col)
    if family == "random" and act != rs.NONE:
        for _ in range(ROUNDS):
            fwd = _oracle(c)
            bad = np.nonzero(_near(c, fwd))[0]
            if bad.size == 0:
                break
            for o in bad:
                taps = fwd["idx"][o]
                x[r.choice(taps[taps >= 0])] = r.standard_normal(C).astype(F)
        else:
            raise AssertionError("no clear input found for case %s" % name)
    rows_out = int(sum(rg.out_lens(lens, kh, st))) * rg.rgd.same_pad(F_in, kw, sf)[0]
    c["gy"] = r.standard_normal((rows_out, N)).astype(F)
    return c


def precondition(case, fwd=None):
    """seg_grad_cases.precondition on the gathered form of the case -> the number of elements in each class."""
    return sc.precondition(case, _oracle(case) if fwd is None else fwd)


def offsets(case):
    """The frame offsets [B + 1] of the case."""
    return np.concatenate([[0], np.cumsum(case["lens"])]).astype(np.int64)


def alone(case, b):
    """Utterance b of the case as a batch of its own (the gradient rows that belong to it)."""
    kh, kw, st, sf = case["window"]
    off = offsets(case) * case["F_in"]
    F_out = rg.rgd.same_pad(case["F_in"], kw, sf)[0]
    oo = np.concatenate([[0], np.cumsum(rg.out_lens(case["lens"], kh, st))]) * F_out
    out = dict(case)
    out.update(x=case["x"][off[b]:off[b + 1]], lens=[case["lens"][b]], gy=case["gy"][oo[b]:oo[b + 1]])
    return out
