"""The rule of speaker clustering (include/xvec_hip.h, xv_ahc) in numpy, over a score matrix that is given: no device.

ahc(s [n, >= n], threshold, target) -> (labels [n] int32, num_clusters, merge_a [n] int32, merge_b [n] int32, merge_height [n]
float64): average-linkage agglomerative clustering.  Only s[i, j] with i < j < n is read.  Every row starts as a cluster named
by its lowest row; S starts as s and a merge of a < b does S(a, k) <- S(a, k) + S(b, k) in float32 for every other live k; the
linkage is L = float64(S) / float64(|A| * |B|) with the product in int64.  A step takes the largest non-NaN L over the live
pairs a < b, the lowest a and then the lowest b among equal L, and stops without merging when there is no such pair, when
clusters <= target, or when not (L >= threshold).  Labels number the clusters in the order of their lowest rows; the log holds
-1 / -1 / NaN past the merges performed (n slots: n - 1 possible merges and one that is never used).

One O(n^2) numpy expression per merge.  ahc_exact is an independent second statement (float64 mean of the original scores over
the member pairs, brute force) for tie-free data."""
import numpy as np


def _start(s):
    s = np.asarray(s, dtype=np.float32)
    n = s.shape[0]
    S = np.triu(s[:, :n], 1)
    return n, (S + S.T).astype(np.float32)


def _steps(s, threshold=-np.inf, target=1):
    """Generator over the merges -> (a, b, L, number of live pairs that attain the maximum)."""
    n, S = _start(s)
    size = np.ones(n, np.int64)
    live = np.ones(n, bool)
    upper = np.triu(np.ones((n, n), bool), 1)
    clusters = n
    for _ in range(max(n - 1, 0)):
        if clusters <= target:
            return
        with np.errstate(invalid="ignore", divide="ignore"):
            L = S.astype(np.float64) / (size[:, None] * size[None, :]).astype(np.float64)
        ok = upper & live[:, None] & live[None, :] & ~np.isnan(L)
        if not ok.any():
            return
        best = np.where(ok, L, -np.inf).max()
        hits = np.flatnonzero(ok & (L == best))
        a, b = divmod(int(hits[0]), n)
        if not (L[a, b] >= threshold):
            return
        yield a, b, L[a, b], hits.size
        with np.errstate(invalid="ignore"):
            S[a, :] = S[a, :] + S[b, :]
        S[:, a] = S[a, :]
        size[a] += size[b]
        live[b] = False
        clusters -= 1


def labels_from_merges(n, merge_a, merge_b):
    """Labels [n] int32 from a merge log (entries of -1 end it): clusters numbered in the order of their lowest rows."""
    root = np.arange(n)
    for a, b in zip(np.asarray(merge_a).tolist(), np.asarray(merge_b).tolist()):
        if a < 0:
            break
        root[root == b] = a
    return np.unique(root, return_inverse=True)[1].astype(np.int32).reshape(n)


def ahc(s, threshold=-np.inf, target=1):
    n = np.asarray(s).shape[0]
    merge_a = np.full(n, -1, np.int32)
    merge_b = np.full(n, -1, np.int32)
    merge_height = np.full(n, np.nan, np.float64)
    m = 0
    for a, b, L, _ in _steps(s, threshold, target):
        merge_a[m], merge_b[m], merge_height[m] = a, b, L
        m += 1
    return labels_from_merges(n, merge_a, merge_b), n - m, merge_a, merge_b, merge_height


def shared_maximum_steps(s):
    """The number of steps of the full clustering at which more than one live pair attains the maximum."""
    return sum(1 for _, _, _, hits in _steps(s) if hits > 1)


def ahc_exact(s):
    """Brute force in float64: the linkage of two clusters is the mean of the original scores over their member pairs.
    -> list of (a, b, L, gap) per merge; gap = L minus the second-best linkage of that step (inf when there is none)."""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    S = np.triu(s[:, :n], 1)
    S = S + S.T
    members = {i: [i] for i in range(n)}
    merges = []
    while len(members) > 1:
        names = sorted(members)
        cand = sorted(((S[np.ix_(members[a], members[b])].mean(), -a, -b) for i, a in enumerate(names) for b in names[i + 1:]),
                      reverse=True)
        L, a, b = cand[0][0], -cand[0][1], -cand[0][2]
        merges.append((a, b, L, L - cand[1][0] if len(cand) > 1 else np.inf))
        members[a] += members.pop(b)
    return merges


def tie_scores(n, seed=2):
    """Scores [n, n] float32 for tie tests: rows with entries in {-2..2}, d = 5, a block of n // 4 rows in four copies (filled
    up from the front of the block).  The scores are small integers, exact in float32 whatever the order of summation, so the
    cluster sums are exact too and most steps have several pairs at the maximum."""
    block = np.random.default_rng(seed).integers(-2, 3, (max(n // 4, 1), 5)).astype(np.float32)
    x = np.tile(block, (4, 1))[:n]
    if len(x) < n:
        x = np.concatenate([x, x[:n - len(x)]])
    return (x @ x.T).astype(np.float32)
