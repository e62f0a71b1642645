"""ORACLE (test infrastructure only) of the cosine scoring feature, numpy, float64 throughout: row preparation
(`ivector-subtract-global-mean` | `transform-vec` | `ivector-normalize-length`, and the eps form of misc/utils.py:317),
the cosine score matrix, the exact false-reject / false-accept step functions of a finite set of scores, and the exact
EER from the sorted scores.  Kaldi is absent from the reference tree: the Kaldi steps follow the published algorithms
(**parity unpinned**, as oracle/ref_post.py)."""
import numpy as np


def delta(d):
    """Bound of one fp32 score of two unit rows of length d against the exact value: d * 2^-24 * sum|a_i b_i| <= d * 2^-24
    for the dot product (Cauchy-Schwarz), plus a few ulps from the two normalisations."""
    return (d + 8) * 2.0 ** -24


def prepare(x, mean=None, transform=None, normalize=True, eps=0.0):
    """[n, d_in] -> [n, d_out] float64: x - mean; T y, or T[:, :-1] y + T[:, -1] when T has d_in + 1 columns;
    y / sqrt(sum y^2 + eps), a zero row staying zero when eps == 0."""
    y = np.asarray(x, dtype=np.float64)
    if mean is not None:
        y = y - np.asarray(mean, dtype=np.float64)[None, :]
    if transform is not None:
        t = np.asarray(transform, dtype=np.float64)
        if t.shape[1] == y.shape[1] + 1:
            y = y @ t[:, :-1].T + t[:, -1][None, :]
        elif t.shape[1] == y.shape[1]:
            y = y @ t.T
        else:
            raise ValueError("transform of %d columns for rows of dimension %d" % (t.shape[1], y.shape[1]))
    if normalize:
        s = np.sum(y * y, axis=1) + float(eps)
        inv = np.where(s == 0.0, 1.0, 1.0 / np.sqrt(np.where(s == 0.0, 1.0, s)))
        y = y * inv[:, None]
    return y


def cosine_matrix(a, b):
    return np.asarray(a, dtype=np.float64) @ np.asarray(b, dtype=np.float64).T


class StepRates(object):
    """Exact error rates of finite score sets: FRR(x) = #{same < x} / #same, FAR(x) = #{diff >= x} / #diff."""

    def __init__(self, same_scores, diff_scores):
        self.same = np.sort(np.asarray(same_scores, dtype=np.float64))
        self.diff = np.sort(np.asarray(diff_scores, dtype=np.float64))

    def count_same_below(self, x):
        return np.searchsorted(self.same, x, side="left")

    def count_diff_below(self, x):
        return np.searchsorted(self.diff, x, side="left")

    def frr(self, x):
        return self.count_same_below(x) / float(self.same.size)

    def far(self, x):
        return (self.diff.size - self.count_diff_below(x)) / float(self.diff.size)


def exact_eer(same_scores, diff_scores):
    """min over every threshold x (each score, and one above all of them) of max(FRR(x), FAR(x)): one merged sweep over
    the sorted scores."""
    same = np.sort(np.asarray(same_scores, dtype=np.float64))
    diff = np.sort(np.asarray(diff_scores, dtype=np.float64))
    ns, nd = same.size, diff.size
    best, i, j = 1.0, 0, 0                     # i = #{same < x}, j = #{diff < x}
    points = np.concatenate([same, diff])
    points.sort()
    for x in list(points) + [np.inf]:
        while i < ns and same[i] < x:
            i += 1
        while j < nd and diff[j] < x:
            j += 1
        best = min(best, max(i / float(ns), (nd - j) / float(nd)))
    return best


def self_pairs(scores, labels):
    """Score matrix [n, n] and labels -> (same-label scores, different-label scores) over the pairs i < j."""
    labels = np.asarray(labels)
    iu, ju = np.triu_indices(scores.shape[0], k=1)
    s = scores[iu, ju]
    same = labels[iu] == labels[ju]
    return s[same], s[~same]
