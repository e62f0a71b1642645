"""The inputs of tests/test_gpu_seg_grad.py and tests/test_gpu_tail_train.py, shared with the host test that checks the
condition put on them (tests/test_seg_grad_host.py).

The ReLU mask is a discontinuity: an h that the kernel rounds to the other side of zero moves y and every gradient by far more
than any rounding bound.  So that NO element ever has to be left out of a comparison, every h_ij of the float64 oracle is
  * exactly zero by construction: a column with gamma = beta = 0 (s = 0, so the kernel's fma(s, d, 0) is a zero as well; ReLU
    gives gradient 0 there and leaky ReLU takes the 0.2 branch), or a zero of the dyadic family without batch norm; or
  * of certain sign by exactness: the dyadic family, where x, w and b are multiples of 1/8 (so z is a multiple of 1/64 that
    float32 holds exactly along the whole chain), beta = 0 and moving_mean sits half a grid step (1/128) off the grid, so z - mm
    is exact, never zero, and h = s (z - mm) has its sign; or
  * at least 64 times its own error bound (ref_seg_grad.bounds, h) away from zero: the random family redraws a row until all
    of its columns are.
precondition() asserts this on the oracle alone.  The seeds are fixed here."""
import numpy as np

import ref_seg_grad as rs

F = np.float32
MARGIN = 64.0

# (name, n, K, N, batch norm, activation, family, operand pitches: "vec" = 16-byte rows, "odd" = not)
CASES = [
    ("one", 1, 1, 1, True, rs.RELU, "random", "odd"),
    ("n31", 31, 35, 33, True, rs.LRELU, "random", "vec"),
    ("n33", 33, 100, 65, False, rs.RELU, "random", "odd"),
    ("n70", 70, 35, 130, True, rs.RELU, "random", "vec"),
    ("dyadic_bn", 70, 100, 130, True, rs.LRELU, "dyadic", "odd"),
    ("linear", 33, 35, 65, False, rs.NONE, "random", "vec"),
    ("dyadic_k1", 70, 1, 33, False, rs.LRELU, "dyadic", "vec"),
    ("bn_linear", 31, 100, 1, True, rs.NONE, "random", "odd"),
    ("dyadic_relu", 70, 100, 65, False, rs.RELU, "dyadic", "vec"),
]
SEEDS = {c[0]: 100 + i for i, c in enumerate(CASES)}


def _bn_random(r, N):
    gamma = r.uniform(0.5, 1.5, N).astype(F)
    beta = (0.1 * r.standard_normal(N)).astype(F)
    mm = (0.1 * r.standard_normal(N)).astype(F)
    mv = r.uniform(0.5, 1.5, N).astype(F)
    return [gamma, beta, mm, mv]


def make(name):
    """-> dict(x [n, K], w [N, K], b, bn or None, act, gy [n, N], family, pad, zero_col or None), float32."""
    _, n, K, N, has_bn, act, family, pad = next(c for c in CASES if c[0] == name)
    r = np.random.RandomState(SEEDS[name])
    zero_col = None
    if family == "dyadic":
        x = (r.randint(-16, 17, (n, K)) / 8.0).astype(F)
        w = (r.randint(-16, 17, (N, K)) / 8.0).astype(F)
        b = (r.randint(-16, 17, N) / 8.0).astype(F)
        bn = None
        if not has_bn:
            x[0], b[0] = 0.0, 0.0                                 # h_00 = 0 exactly: the zero of the lower branch is exercised
        if has_bn:
            bn = _bn_random(r, N)
            bn[1] = np.zeros(N, dtype=F)
            bn[2] = (r.randint(-64, 64, N) / 64.0 + 1.0 / 128.0).astype(F)
    else:
        w = (r.standard_normal((N, K)) / np.sqrt(K)).astype(F)
        b = (0.1 * r.standard_normal(N)).astype(F)
        bn = _bn_random(r, N) if has_bn else None
        x = np.zeros((n, K), dtype=F)
    if has_bn and N > 1:
        zero_col = N // 2
        bn[0][zero_col] = 0.0
        bn[1][zero_col] = 0.0
    if family == "random":
        for i in range(n):
            for _ in range(1000):
                x[i] = r.standard_normal(K).astype(F)
                if act == rs.NONE or _row_clear(x[i:i + 1], w, b, bn, act, zero_col):
                    break
            else:
                raise AssertionError("no clear row found for case %s" % name)
    gy = r.standard_normal((n, N)).astype(F)
    return dict(name=name, x=x, w=w, b=b, bn=bn, act=act, gy=gy, family=family, pad=pad, zero_col=zero_col)


def _row_clear(x, w, b, bn, act, zero_col):
    fwd = rs.forward(x, w, b, bn, act, rs.SLOPE)
    far = np.abs(fwd["h"]) >= MARGIN * rs.bounds(fwd)["h"]
    if zero_col is not None:
        far[:, zero_col] = True
    return bool(far.all())


def precondition(case, fwd=None, extra_h=None):
    """Assert the condition of the module docstring on the oracle's h (`extra_h`: a further error of h, from an inexact input,
    to add to the bound) -> the number of elements in each class (zero, exact sign, far)."""
    fwd = rs.forward(case["x"], case["w"], case["b"], case["bn"], case["act"], rs.SLOPE) if fwd is None else fwd
    h = fwd["h"]
    bh = rs.bounds(fwd)["h"] + (0.0 if extra_h is None else extra_h)
    zero = np.zeros(h.shape, dtype=bool)
    exact = np.zeros(h.shape, dtype=bool)
    if case.get("zero_col") is not None:
        j = case["zero_col"]
        assert case["bn"][0][j] == 0 and case["bn"][1][j] == 0 and np.all(h[:, j] == 0)
        zero[:, j] = True
    if case.get("family") == "dyadic":
        x, w, b = fwd["x"], fwd["w"], fwd["b"]
        for v in (x, w, b):
            assert np.all(v * 8 == np.round(v * 8))
        assert np.max(np.abs(x) @ np.abs(w).T + np.abs(b)[None, :]) < 2.0 ** 17          # multiples of 1/64 below 2^17: exact
        if fwd["bn"] is None:
            exact[:] = True                                   # h = z exactly, zeros included
        else:
            gamma, beta, mm, _ = fwd["bn"]
            assert np.all(beta == 0) and np.all(mm * 128 == np.round(mm * 128)) and np.all((mm * 128) % 2 == 1)
            assert np.all(fwd["z"] - mm[None, :] != 0)
            exact[:] = True
    far = np.abs(h) >= MARGIN * bh
    ok = zero | exact | far | (case["act"] == rs.NONE)
    assert ok.all(), ("an h of case %s lies within 64 bounds of zero" % case.get("name"), int((~ok).sum()))
    return int(zero.sum()), int((exact & ~zero).sum()), int((far & ~zero & ~exact).sum())


# ---------------------------------------------------------------------------------------------- the tail trainer's toy task
def separable_pooled(seed, speakers=8, segments=4, dim=48):
    """Pooled rows of a separable toy set: `speakers` centres, `segments` rows each -> (x [n, dim] float32, labels int32)."""
    r = np.random.RandomState(seed)
    centres = r.standard_normal((speakers, dim))
    labels = np.repeat(np.arange(speakers), segments)
    return (centres[labels] + 0.2 * r.standard_normal((labels.size, dim))).astype(F), labels.astype(np.int32)
