"""The inputs of tests/test_gpu_tconv.py, shared with the host test that checks the condition put on them
(tests/test_tconv_host.py).

As in seg_grad_cases.py the ReLU mask is a discontinuity, so that NO element ever has to be left out of a comparison every h of
the float64 oracle is exactly zero by construction (a column with gamma = beta = 0, or a zero of the dyadic family), of certain
sign by exactness (the dyadic family: x, w and b multiples of 1/8), or at least 64 of its own error bounds (ref_tconv.bounds, h)
away from zero.  An input row takes part in up to W output rows, so the random family draws the rows of an utterance in order:
input row s completes output row s - (W - 1), and is redrawn until that output row is clear (the later output rows it takes part
in are not complete yet).  precondition() asserts the condition on the oracle alone.  The seeds are fixed here; they were found
on the CPU, with the float64 rule standing in for the device.

Utterance lengths: W, W + 1, W + 62, W + 63, W + 64 input rows give 1, 2, 63, 64 and 65 output rows, so the borders between
utterances fall inside and on the edges of the 64-row tiles; `short` puts an utterance with fewer than W rows in the middle;
`long` has 1100 output rows, the smallest size at which the column sums take a second slice (beyond 1024 rows) and the chain of
gw is cut into row ranges (beyond 256 rows with few tiles)."""
import numpy as np

import ref_seg_grad as rs
import ref_tconv as rt
import seg_grad_cases as sc

F = np.float32
MARGIN = sc.MARGIN


def _lengths(W, kind):
    if kind == "mixed":
        return [W + 63, W, W + 64, W + 1, W + 62]
    if kind == "short":
        return [W + 1, W + 64, max(W - 1, 0), W + 62, W]
    if kind == "one":
        return [W + 64]
    if kind == "long":                       # 1100 output rows: two slices of the column sums, five row ranges of gw
        return [W + 599, W + 499]
    raise ValueError(kind)


# (name, W, C, N, batch norm, activation, family, lengths, layout: "vec" = 16-byte rows where C allows, "odd" = ldx > C and every
# base 4 bytes off a 16-byte boundary)
CASES = [
    ("w1_c30", 1, 30, 8, True, rs.RELU, "random", "mixed", "vec"),
    ("w1_c68", 1, 68, 64, True, rs.LRELU, "random", "short", "vec"),
    ("w5_c30", 5, 30, 8, True, rs.RELU, "random", "mixed", "vec"),
    ("w5_c23", 5, 23, 72, True, rs.LRELU, "random", "short", "vec"),
    ("w5_c68", 5, 68, 64, False, rs.RELU, "random", "mixed", "odd"),
    ("w7_c8", 7, 8, 130, True, rs.RELU, "random", "mixed", "vec"),
    ("w7_c23", 7, 23, 72, False, rs.NONE, "random", "one", "vec"),
    ("w7_c68", 7, 68, 64, True, rs.RELU, "random", "short", "vec"),
    ("w9_c8", 9, 8, 130, True, rs.LRELU, "dyadic", "short", "odd"),
    ("w9_c30", 9, 30, 8, False, rs.LRELU, "dyadic", "one", "vec"),
    ("w9_c68", 9, 68, 64, True, rs.LRELU, "random", "mixed", "vec"),
    ("w9_c23", 9, 23, 72, True, rs.RELU, "random", "mixed", "odd"),
    ("w5_long", 5, 30, 8, True, rs.LRELU, "random", "long", "vec"),
]
SEEDS = {c[0]: 300 + i for i, c in enumerate(CASES)}
TRIES = 4000


def make(name):
    """-> dict(x [rows, C], offsets, taps, w [N, W C], b, bn or None, act, gy [total_out, N], family, layout, zero_col)."""
    _, W, C, N, has_bn, act, family, kind, layout = next(c for c in CASES if c[0] == name)
    r = np.random.RandomState(SEEDS[name])
    K = W * C
    lengths = _lengths(W, kind)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = int(offsets[-1])
    zero_col = None
    if family == "dyadic":
        x = (r.randint(-16, 17, (rows, C)) / 8.0).astype(F)
        w = (r.randint(-16, 17, (N, K)) / 8.0).astype(F)
        b = (r.randint(-16, 17, N) / 8.0).astype(F)
        bn = None
        if not has_bn:
            x[:W], b[0] = 0.0, 0.0                                # h_00 = 0 exactly: the zero of the lower branch is exercised
        else:
            bn = sc._bn_random(r, N)
            bn[1] = np.zeros(N, dtype=F)
            bn[2] = (r.randint(-64, 64, N) / 64.0 + 1.0 / 128.0).astype(F)
    else:
        w = (r.standard_normal((N, K)) / np.sqrt(K)).astype(F)
        b = (0.1 * r.standard_normal(N)).astype(F)
        bn = sc._bn_random(r, N) if has_bn else None
        x = np.zeros((rows, C), dtype=F)
    if has_bn and N > 1:
        zero_col = N // 2
        bn[0][zero_col] = 0.0
        bn[1][zero_col] = 0.0
    if family == "random":
        for bi in range(len(lengths)):
            for s in range(int(offsets[bi]), int(offsets[bi + 1])):
                t = s - (W - 1)
                for _ in range(TRIES):
                    x[s] = r.standard_normal(C).astype(F)
                    if act == rs.NONE or t < offsets[bi] or sc._row_clear(x[t:s + 1].reshape(1, K), w, b, bn, act, zero_col):
                        break
                else:
                    raise AssertionError("no clear row found for case %s" % name)
    total_out = int(rt.out_offsets(offsets, W)[-1])
    gy = r.standard_normal((total_out, N)).astype(F)
    return dict(name=name, x=x, offsets=offsets, taps=W, w=w, b=b, bn=bn, act=act, gy=gy, family=family, layout=layout,
                zero_col=zero_col)


def precondition(case, fwd=None):
    """seg_grad_cases.precondition on the im2col form of the case -> the number of elements in each class."""
    fwd = rt.forward(case["x"], case["offsets"], case["taps"], case["w"], case["b"], case["bn"], case["act"]) if fwd is None else fwd
    return sc.precondition(case, fwd)


def alone(case, b):
    """Utterance b of the case as a batch of its own (the gradient rows that belong to it)."""
    off, oo = case["offsets"], rt.out_offsets(case["offsets"], case["taps"])
    out = dict(case)
    out.update(x=case["x"][off[b]:off[b + 1]], offsets=np.array([0, off[b + 1] - off[b]], dtype=np.int64), gy=case["gy"][oo[b]:oo[b + 1]])
    return out
