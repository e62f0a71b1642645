"""The inputs of tests/test_gpu_bn_batch.py, shared with the host test that checks the condition put on them
(tests/test_bn_batch_host.py).

Shapes, the smallest at which the kernels of csrc/bn_batch.hip can still go wrong: n in 1 (every column constant, f = 1), 2, 63,
64, 65 (the edges of the 64-row chunk) and 1025 (the first n with two slices of the column sums); N in 1, 31, 33 (around the
32-column workgroup of the sweeps) and 68 (beyond the 64 columns of a wave of the elementwise kernels); every activation.
Where N >= 3: column 0 is constant (v = 0 exactly, r = 1 / sqrt(eps), h = beta), column 1 has mean 1000 and standard deviation
0.01 (a one-sweep E[z^2] - mu^2 loses it entirely in float32 and most of it in a float32-rounded mean), column N // 2 has gamma
= beta = 0 (h = 0 exactly).  The dyadic family (z multiples of 1/8, |z| <= 2, n a power of two) has an exact mean.

The ReLU / leaky-ReLU mask is a discontinuity and can only be compared where the sign of h is certain.  make() makes it
certain: it draws z, evaluates the float64 rule, and moves every element whose |h| is below MARGIN = 64 of its own bounds
(ref_bn_batch.bounds, h) away from zero, again and again because a move shifts the column's mean, for at most ROUNDS rounds;
then it raises.  The exact zeros of the zero-gamma column are the one exception (h = 0 in the oracle and on the device, both
take the lower branch).  The constant column and n = 1 cannot be moved (h = beta there), so |beta| >= 0.1 everywhere else.  No
element is ever left out of a comparison."""
import itertools

import numpy as np

import ref_bn_batch as rb

F = np.float32
MARGIN = 64.0
ROUNDS = 20

NS = (1, 2, 63, 64, 65, 1025)
WIDTHS = (1, 31, 33, 68)
ACTS = (rb.NONE, rb.RELU, rb.LRELU)
_ACT_NAME = {rb.NONE: "none", rb.RELU: "relu", rb.LRELU: "lrelu"}

# (name, n, N, activation, family)
CASES = [("n%d_N%d_%s" % (n, N, _ACT_NAME[a]), n, N, a, "random") for n, N, a in itertools.product(NS, WIDTHS, ACTS)]
CASES += [("dyadic_n%d_N%d_%s" % (n, N, _ACT_NAME[a]), n, N, a, "dyadic") for (n, N), a in
          itertools.product(((64, 33), (2, 31), (1024, 5)), ACTS)]
NAMES = [c[0] for c in CASES]
SEEDS = {c[0]: 900 + i for i, c in enumerate(CASES)}

# layout -> (columns of padding on every matrix, floats between a 16-byte aligned allocation and the base)
LAYOUTS = {"contiguous": (0, 0), "padded": (3, 0), "offset": (1, 1)}


def make(name):
    """-> dict(name, n, N, z [n, N], gamma, beta, act, gy [n, N], mm, mv, momentum, bessel, family, zero_col, const_col)."""
    idx, (_, n, N, act, family) = next((i, c) for i, c in enumerate(CASES) if c[0] == name)
    r = np.random.RandomState(SEEDS[name])
    gamma = (r.choice([-1.0, 1.0], N) * (0.5 + r.rand(N))).astype(F)
    beta = (r.choice([-1.0, 1.0], N) * (0.1 + np.abs(0.3 * r.standard_normal(N)))).astype(F)
    zero_col = const_col = None
    if family == "dyadic":
        z = (r.randint(-16, 17, (n, N)) / 8.0).astype(F)
    else:
        z = (r.standard_normal((n, N)) * (0.5 + r.rand(N))[None, :] + r.standard_normal(N)[None, :]).astype(F)
        if N >= 3:
            const_col = 0
            z[:, 0] = F(0.75)
            z[:, 1] = (1000.0 + 0.01 * r.standard_normal(n)).astype(F)
            gamma[1], beta[1] = 0.5, 1.0
    if N >= 3:
        zero_col = N // 2
        gamma[zero_col] = beta[zero_col] = 0.0
    fixed = np.zeros(N, dtype=bool)                                   # columns no move can help: h = beta (or 0) there
    for c in (zero_col, const_col):
        if c is not None:
            fixed[c] = True
    for _ in range(ROUNDS):
        fwd = rb.forward(z, gamma, beta, act)
        bh = rb.bounds(fwd)["h"]
        bad = (np.abs(fwd["h"]) < 2.0 * MARGIN * bh) & ~fixed[None, :]
        if not bad.any():
            break
        direction = np.where(fwd["h"] >= 0, 1.0, -1.0) * np.sign(fwd["s"])[None, :]
        if family == "dyadic":
            step = np.full(z.shape, 0.125)
        else:
            slope = np.where(fwd["s"] == 0.0, 1.0, np.abs(fwd["s"]))            # s = 0: the zero-gamma column, never moved
            step = 4.0 * (4.0 * MARGIN * bh - np.abs(fwd["h"])) / slope[None, :]
            step = np.maximum(step, 4.0 * np.spacing(np.abs(z).astype(F)).astype(np.float64))
        z = np.where(bad, (z.astype(np.float64) + direction * step).astype(F), z)
    else:
        raise AssertionError("case %s: elements within %g bounds of the mask's edge after %d rounds" % (name, MARGIN, ROUNDS))
    gy = r.standard_normal((n, N)).astype(F)
    mm = r.standard_normal(N).astype(F)
    mv = (0.5 + r.rand(N)).astype(F)
    return dict(name=name, n=n, N=N, z=z, gamma=gamma, beta=beta, act=act, gy=gy, mm=mm, mv=mv,
                momentum=0.99 if idx % 2 == 0 else 0.9, bessel=bool(idx % 3 != 0), family=family, zero_col=zero_col,
                const_col=const_col)


def precondition(case, fwd=None):
    """Asserts the condition on the float64 oracle alone -> dict(clear, exact_zero): how many elements are in each class."""
    fwd = rb.forward(case["z"], case["gamma"], case["beta"], case["act"]) if fwd is None else fwd
    h, bh = fwd["h"], rb.bounds(fwd)["h"]
    clear = np.abs(h) >= MARGIN * bh
    zero = np.zeros_like(clear)
    if case["zero_col"] is not None:
        zero[:, case["zero_col"]] = h[:, case["zero_col"]] == 0.0
    clear &= ~zero
    left = ~(clear | zero)
    assert not left.any(), "case %s: %d elements neither clear of the mask's edge nor exact zeros" % (case["name"], int(left.sum()))
    assert np.all(np.isfinite(h))
    return dict(clear=int(clear.sum()), exact_zero=int(zero.sum()))
