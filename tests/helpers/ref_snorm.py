"""ORACLE (test infrastructure only) of cohort score normalisation, numpy, float64 throughout.  The reference has no such step
(egs/sre/v1/run.sh:13) and neither has Kaldi: **parity unpinned**; the definitions are those of include/xvec_hip.h.

Scores come as a matrix [n, m] (row i against cohort column j).  Excluded columns are masked out, each row is sorted in
descending order, and mean / np.std(ddof=0) are taken of its first K_eff = min(top_k, eligible) entries (top_k 0: all)."""
import numpy as np


def cohort_stats(scores, top_k=0, labels=None, cohort_labels=None):
    """-> (mean [n], std [n], count [n]) in float64 / int64; K_eff = 0 gives NaN, NaN, 0."""
    s = np.asarray(scores, dtype=np.float64)
    n, m = s.shape
    mean, std, count = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n, np.int64)
    for i in range(n):
        row = s[i]
        if labels is not None:
            row = row[np.asarray(cohort_labels) != np.asarray(labels)[i]]
        k = row.size if top_k == 0 else min(int(top_k), row.size)
        count[i] = k
        if k == 0:
            continue
        top = np.sort(row)[::-1][:k]
        mean[i] = np.mean(top)
        std[i] = np.std(top, ddof=0)
    return mean, std, count


def normalize(scores, ia, ib, enroll, test, mode):
    """enroll / test: (mean, std, ...) per row; mode "z", "t" or "s"."""
    s = np.asarray(scores, dtype=np.float64)
    z = (s - enroll[0][ia]) / enroll[1][ia] if mode in ("z", "s") else None
    t = (s - test[0][ib]) / test[1][ib] if mode in ("t", "s") else None
    return z if mode == "z" else (t if mode == "t" else 0.5 * (z + t))
