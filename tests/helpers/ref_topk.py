"""The rule of identification (include/xvec_hip.h, xv_score_topk) in numpy, over a score matrix that is given: no device.

top_k(scores [n, m], k, labels_a, labels_b) -> (scores [n, k], indices [n, k] int32, count [n] int32): per row the k eligible
columns with the largest scores, by score descending and by column ascending among equal scores (so ties at the selection
boundary go to the lowest columns); column j is eligible for row i unless labels are given and labels_a[i] == labels_b[j];
count = min(k, eligible) and the positions past it hold -inf / -1.  The scores keep their dtype and their bits."""
import numpy as np


def top_k(scores, k, labels_a=None, labels_b=None):
    s = np.asarray(scores)
    n, m = s.shape
    out_s = np.full((n, k), -np.inf, dtype=s.dtype)
    out_i = np.full((n, k), -1, dtype=np.int32)
    count = np.zeros(n, dtype=np.int32)
    cols = np.arange(m)
    for i in range(n):
        ok = np.ones(m, bool) if labels_a is None else np.asarray(labels_b) != np.asarray(labels_a)[i]
        idx, row = cols[ok], s[i, ok]
        order = np.lexsort((idx, -row))[:k]
        count[i] = order.size
        out_s[i, :order.size] = row[order]
        out_i[i, :order.size] = idx[order]
    return out_s, out_i, count


def boundary_ties(scores, k, labels_a=None, labels_b=None):
    """Number of rows in which the selection boundary falls inside a run of equal scores: the k-th and the (k + 1)-th largest
    eligible scores are equal."""
    s = np.asarray(scores)
    rows = 0
    for i in range(s.shape[0]):
        ok = np.ones(s.shape[1], bool) if labels_a is None else np.asarray(labels_b) != np.asarray(labels_a)[i]
        row = np.sort(s[i, ok])[::-1]
        rows += int(row.size > k and row[k - 1] == row[k])
    return rows


def tie_operands():
    """Operands for tie tests -> a [300, 7], b [1000, 7] float32 with entries in {-2..2}: the scores are small integers (exact
    in fp32 whatever the order of summation) and most of them collide; the gallery is four copies of a block of 250 rows, so
    every score of a row comes at least four times and runs of equal scores straddle any selection boundary."""
    rng = np.random.default_rng(2)
    a = rng.integers(-2, 3, (300, 7)).astype(np.float32)
    b = np.tile(rng.integers(-2, 3, (250, 7)).astype(np.float32), (4, 1))
    return a, b
