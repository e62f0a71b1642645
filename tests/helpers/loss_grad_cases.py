"""The inputs of tests/test_gpu_loss_grad.py, shared with the host test that checks the condition the issue puts on them: for
every case the largest element of the error bound stays below 1e-4 (the project's parity gate) of the tensor's largest
|gradient|, so that the bound cannot hide a failure.  That holds for moderate ||x|| and ||w||: the bound grows with
(E + 8) u ||x|| ||w||."""
import numpy as np

import ref_loss_grad

HEAD_ID = {"softmax": 0, "asoftmax": 1, "additive_margin_softmax": 2, "additive_angular_margin_softmax": 3}

# (head, margin, fa, with bias)
HEADS = [("softmax", 0.0, 0.0, True), ("softmax", 0.0, 0.0, False), ("asoftmax", 1, 0.0, False), ("asoftmax", 2, 0.6, False),
         ("asoftmax", 4, 0.3, False), ("additive_margin_softmax", 0.25, 0.8, False),
         ("additive_angular_margin_softmax", 0.3, 0.5, False), ("additive_angular_margin_softmax", 0.2, 1.0, False)]

# (n, C, E): every C in {1, 127, 128, 129, 300}, E in {1, 30, 33, 128}, n in {1, 5, 129, 260}
SHAPES = [(1, 1, 1), (5, 127, 30), (5, 128, 33), (1, 129, 128), (129, 129, 30), (129, 300, 33), (260, 127, 128), (260, 300, 30),
          (129, 1, 33), (260, 128, 1), (5, 300, 128)]

GATE = 1e-4


def f32(a):
    return np.asarray(a, dtype=np.float32)


def edge_labels(rs, n, c, same=False):
    if same:
        return np.full(n, min(127, c - 1), dtype=np.int32)
    want = [0, c - 1, min(127, c - 1), min(128, c - 1)]
    labels = rs.randint(0, c, n)
    if n == 1:
        labels[0] = c - 1
    else:
        labels[:min(n, 4)] = want[:min(n, 4)]
    return labels.astype(np.int32)


def make_case(n, c, e, same=False, seed=0):
    """-> x [n, E], kernel [E, C], bias [C], labels [n], float32 / int32."""
    rs = np.random.RandomState(100000 * seed + 1000 * n + 10 * c + e)
    # a common direction in every row: the sums over the rows then have a coherent part, and the worst-case bound of a chain of
    # n roundings stays well under the gate relative to them
    x = (rs.standard_normal((n, e)) * rs.uniform(0.6, 1.5, (n, 1)) + 2.0 * rs.standard_normal((1, e))) * (0.3 / np.sqrt(e))
    w = rs.standard_normal((e, c)) / np.sqrt(e) * rs.uniform(0.5, 1.5, (1, c))
    b = 0.3 * rs.standard_normal(c)
    return f32(x), f32(w), f32(b), edge_labels(rs, n, c, same)


def reference(x, labels, w, b, head, margin, fa, scale=None):
    """The float64 oracle on the float32 inputs the kernel sees, and its bounds -> (ref, (bx, bk, bb))."""
    ref = ref_loss_grad.classifier_grad(x.astype(np.float64), labels, w.astype(np.float64), None if b is None else b.astype(np.float64),
                                        head, margin, fa, scale)
    return ref, ref_loss_grad.bounds(ref, w.shape[0], w.shape[1])


def gate_ratios(ref, bnd):
    """largest bound / largest |gradient| per tensor (None where the gradient is identically zero, as for C = 1)."""
    out = []
    for g, b in ((ref["grad_x"], bnd[0]), (ref["grad_kernel"], bnd[1]), (ref["grad_bias"], bnd[2])):
        if g is None:
            continue
        top = float(np.abs(g).max())
        out.append(None if top == 0.0 else float(b.max()) / top)
    return out


SPECIAL_HEADS = [("asoftmax", 2, 0.6), ("asoftmax", 4, 0.3), ("additive_margin_softmax", 0.25, 0.8),
                 ("additive_angular_margin_softmax", 0.3, 0.5)]
SPECIAL_K, SPECIAL_COL, SPECIAL_TINY = 7, 100, 50


def make_special():
    """n = 5, C = 129, E = 33 with three special rows: row 1 is zero; column SPECIAL_COL of the kernel is the one-hot e_k and row 2
    is 2.5 e_k with that label (c_raw = 1 exactly: the clipped branch); column SPECIAL_TINY is scaled by 1e-8, under the floor of
    tf.nn.l2_normalize, and is the label of row 3."""
    x, w, b, labels = make_case(5, 129, 33)
    x[1] = 0.0
    w[:, SPECIAL_COL] = 0.0
    w[SPECIAL_K, SPECIAL_COL] = 1.0
    x[2] = 0.0
    x[2, SPECIAL_K] = 2.5
    labels[2] = SPECIAL_COL
    w[:, SPECIAL_TINY] *= np.float32(1e-8)
    labels[3] = SPECIAL_TINY
    return x, w, labels
