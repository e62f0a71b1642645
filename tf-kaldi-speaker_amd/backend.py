"""Training the LDA + PLDA back-end: what the reference does with three Kaldi binaries before it scores
(egs/voxceleb/v1/run.sh:384-400, egs/sre/v1/run.sh:399-411):

    ivector-mean scp:xvector.scp mean.vec                                              global_mean
    ivector-compute-lda --total-covariance-factor=0.0 --dim=$lda_dim ... transform.mat   scatter_stats + lda_from_stats
    ivector-compute-plda ark:spk2utt ... plda                                          scatter_stats + plda_from_stats

The heavy part of all three is the second-moment matrix of the training set (about 10^6 rows of dimension 512); it and the
class means come from the GPU in double (csrc/backend.hip through the C ABI: xv_gram_f64 / xv_gram_f64_rows64 /
xv_class_mean_f64).  scatter_stats is the only function here that needs a device (no CPU path, as scoring.py); everything
that takes a `Stats` is numpy float64 on the host and runs without one.

Kaldi is absent from the reference tree: ivector-compute-lda.cc and the PldaStats / PldaEstimator of plda.cc are restated from
the published sources (**parity unpinned**), checked against tests/helpers/ref_backend.py, a transcription of the Kaldi loops
that accumulates speaker by speaker and runs the EM class by class.  `ivector-adapt-plda` (sre only) stays with Kaldi."""

import numpy as np

from . import _lib
from ._lib import ptr
from . import plda as plda_mod
from . import scoring


class Stats(object):
    """Sufficient statistics of a labelled set, float64: `n` rows in S classes with `counts` [S] (all >= 1) and raw class
    means `means` [S, d]; `mean` [d], the mean of all rows; and, about `center` [d],
    total = sum_r (x_r - center)(x_r - center)^T and between = sum_s n_s (m_s - center)(m_s - center)^T."""

    def __init__(self, counts, means, mean, center, total, between):
        self.counts = np.ascontiguousarray(counts, dtype=np.float64).reshape(-1)
        self.means = np.ascontiguousarray(means, dtype=np.float64)
        self.mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        self.center = np.ascontiguousarray(center, dtype=np.float64).reshape(-1)
        self.total = np.ascontiguousarray(total, dtype=np.float64)
        self.between = np.ascontiguousarray(between, dtype=np.float64)
        s = self.counts.shape[0]
        if s < 1:
            raise ValueError("Stats: no class")
        if self.means.ndim != 2 or self.means.shape[0] != s:
            raise ValueError("Stats: %d counts for class means of shape %s" % (s, self.means.shape))
        d = self.means.shape[1]
        if d < 1 or self.mean.shape != (d,) or self.center.shape != (d,) or self.total.shape != (d, d) or self.between.shape != (d, d):
            raise ValueError("Stats: dimension %d, but mean %s, center %s, total %s, between %s"
                             % (d, self.mean.shape, self.center.shape, self.total.shape, self.between.shape))
        if not np.all(self.counts >= 1.0) or not np.all(self.counts == np.floor(self.counts)):
            raise ValueError("Stats: class counts must be whole numbers >= 1")
        self.n = int(self.counts.sum())

    @property
    def dim(self):
        return self.means.shape[1]

    @property
    def num_classes(self):
        return self.counts.shape[0]

    def about_mean(self):
        """(total, between) about the mean of all rows: both lose n (mean - center)(mean - center)^T."""
        delta = self.mean - self.center
        shift = float(self.n) * np.outer(delta, delta)
        return self.total - shift, self.between - shift


def global_mean(x):
    """`ivector-mean` without spk2utt: the mean of the rows of x [n, d], summed in double, as float32 [d] (host)."""
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("global_mean: expected a non-empty [n, d] array, got shape %s" % (x.shape,))
    return (x.sum(axis=0, dtype=np.float64) / float(x.shape[0])).astype(np.float32)


def class_lists(class_index, n):
    """A per-row class id [n] (any array np.unique can sort), or a pair (offsets [S + 1], index) in the convention of
    xv_speaker_mean -> (offsets, index) as int64 arrays with the empty classes removed.  ValueError for an empty class list,
    mismatched lengths or a row number outside [0, n)."""
    if isinstance(class_index, tuple):
        if len(class_index) != 2:
            raise ValueError("class_index: expected per-row ids or (offsets, index)")
        off = np.asarray(class_index[0], dtype=np.int64).reshape(-1)
        idx = np.asarray(class_index[1], dtype=np.int64).reshape(-1)
        if off.size < 1 or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != idx.size:
            raise ValueError("class_index: offsets must start at 0, not decrease and end at len(index) = %d" % idx.size)
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise ValueError("class_index: a row number is outside [0, %d)" % n)
        keep = np.diff(off) > 0
        off = np.concatenate([[0], np.cumsum(np.diff(off)[keep])]).astype(np.int64)
    else:
        ids = np.asarray(class_index).reshape(-1)
        if ids.shape[0] != n:
            raise ValueError("class_index: %d ids for %d rows" % (ids.shape[0], n))
        inverse = np.unique(ids, return_inverse=True)[1].reshape(-1) if n else np.zeros(0, np.int64)
        idx = np.argsort(inverse, kind="stable").astype(np.int64)
        off = np.concatenate([[0], np.cumsum(np.bincount(inverse))]).astype(np.int64)
    if off.size < 2:
        raise ValueError("class_index: no class with at least one row")
    if n >= 2 ** 31 or idx.size >= 2 ** 31:
        raise ValueError("class_index: more than 2^31 - 1 rows")
    return off, idx


def _gram(lib, torch, device, rows, n, d, center, weights, rows64=False):
    """xv_gram_f64 (or its double-row form) with a workspace of its own -> [d, d] float64 tensor on the device."""
    need = _lib.check(lib.xv_gram_f64_workspace(n, d))
    ws = torch.empty((max(need, 8) // 8,), dtype=torch.float64, device=rows.device)
    g = torch.empty((d, d), dtype=torch.float64, device=rows.device)
    stream = _lib.stream(device)
    fn = lib.xv_gram_f64_rows64 if rows64 else lib.xv_gram_f64
    _lib.check(fn(device, ptr(rows), rows.shape[1], n, d, ptr(center),
                  ptr(weights), ptr(g), ptr(ws), need, stream))
    return g


def scatter_stats(x, class_index, center=None, device=0):
    """Rows x [n, d] (numpy, or a float32 torch tensor already on the device) and their classes (class_lists) -> Stats.
    `center` [d] is the point the two scatter matrices are taken about; None: the mean of the rows (the best conditioned
    choice, and the one lda_from_stats needs).  Rows that belong to no class of an (offsets, index) pair do not count; a row
    listed k times counts k times.  1 <= d <= 2048.  GPU: class means (xv_class_mean_f64), the total scatter (xv_gram_f64)
    and the between-class scatter, a second Gram over the class means with the class counts as weights."""
    n, d = scoring._shape2(x, "x")
    if d < 1 or d > 2048:
        raise ValueError("x: rows of dimension %d, expected 1..2048" % d)
    off, idx = class_lists(class_index, n)
    counts = np.diff(off).astype(np.float64)
    if center is not None:
        center = np.asarray(center, dtype=np.float64).reshape(-1)
        if center.shape != (d,):
            raise ValueError("center: shape %s for rows of dimension %d" % (center.shape, d))
    mult = np.bincount(idx, minlength=n).astype(np.float64)
    torch = scoring._need_device()
    lib = _lib.load()
    with torch.cuda.device(device):
        xd = scoring._rows(x, device, "x")
        dev = xd.device
        offd = torch.from_numpy(off.astype(np.int32)).to(dev)
        idxd = torch.from_numpy(idx.astype(np.int32)).to(dev)
        s = counts.shape[0]
        md = torch.empty((s, d), dtype=torch.float64, device=dev)
        stream = _lib.stream(device)
        _lib.check(lib.xv_class_mean_f64(device, ptr(xd), d, n, d, ptr(offd), ptr(idxd), s, None,
                                         ptr(md), d, stream))
        means = md.cpu().numpy()
        mean = counts @ means / counts.sum()
        c = mean if center is None else center
        cd = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
        wd = None if np.all(mult == 1.0) else torch.from_numpy(mult).to(dev)
        total = _gram(lib, torch, device, xd, n, d, cd, wd).cpu().numpy()
        centred = torch.from_numpy(np.ascontiguousarray(means - c[None, :])).to(dev)
        nd = torch.from_numpy(counts).to(dev)
        between = _gram(lib, torch, device, centred, s, d, None, nd, rows64=True).cpu().numpy()
    return Stats(counts, means, mean, c, total, between)


def _eigh_descending(m):
    s, u = np.linalg.eigh(0.5 * (m + m.T))
    order = np.argsort(-s, kind="stable")
    return s[order], u[:, order]


def lda_from_stats(stats, dim=100, total_covariance_factor=0.0, covariance_floor=1e-6):
    """ivector-compute-lda.cc over `stats` -> the [dim, d + 1] float32 matrix `transform-vec` applies ([A | -A mu], the last
    column an offset: scoring.check_transform): lda_float64 rounded to what the Kaldi matrix file holds."""
    return lda_float64(stats, dim, total_covariance_factor, covariance_floor).astype(np.float32)


def lda_float64(stats, dim=100, total_covariance_factor=0.0, covariance_floor=1e-6):
    """[A | -A mu] in float64.  With the scatter matrices about the mean mu of all rows (Kaldi's
    ComputeAndSubtractMean): total = total_scatter / n, within = (total_scatter - between_scatter) / n,
    C = (1 - f) within + f total = U diag(s) U^T with s floored at max(s) covariance_floor, T = diag(s^-1/2) U^T,
    P = the eigenvectors of T (total - within) T^T by descending eigenvalue, A = P[:, :dim]^T T."""
    d = stats.dim
    dim = int(dim)
    if dim < 1 or dim > d:
        raise ValueError("lda_from_stats: dim %d for rows of dimension %d" % (dim, d))
    f = float(total_covariance_factor)
    if not 0.0 <= f <= 1.0:
        raise ValueError("lda_from_stats: total_covariance_factor must be in [0, 1], got %r" % f)
    if not float(covariance_floor) >= 0.0:
        raise ValueError("lda_from_stats: covariance_floor must be >= 0")
    total_scatter, between_scatter = stats.about_mean()
    n = float(stats.n)
    total = total_scatter / n
    within = (total_scatter - between_scatter) / n
    s, u = np.linalg.eigh((1.0 - f) * within + f * total)
    s = np.maximum(s, s.max() * float(covariance_floor))
    if not s.min() > 0.0:
        raise ValueError("lda_from_stats: the covariance to whiten is singular and covariance_floor is 0")
    t = u.T / np.sqrt(s)[:, None]
    _, p = _eigh_descending(t @ (total - within) @ t.T)
    a = p[:, :dim].T @ t
    return np.concatenate([a, -(a @ stats.mean)[:, None]], axis=1)


def plda_from_stats(stats, num_em_iters=10):
    """PldaStats + PldaEstimator of plda.cc over `stats` (every class weight 1) -> plda.Plda, with the last within- and
    between-class covariances of the EM as `within_var` / `between_var` on the result.

    offset_scatter = sum_s (X_s^T X_s - n_s m_s m_s^T) = total - between (about any centre), sum = sum_s m_s, S classes, N rows.
    From W = B = I, each iteration: Wstats = offset_scatter, Wcount = N - S; for each class, with m = m_s - sum / S and n = n_s:
    M = (B^-1 + n W^-1)^-1, w = M (n W^-1 m), Bstats += M + w w^T, Bcount += 1, Wstats += n (M + (m - w)(m - w)^T), Wcount += 1;
    then W = Wstats / Wcount, B = Bstats / Bcount.  Classes are grouped by n here: one inversion per distinct n.
    Output: mean = sum / S; W = L L^T, T1 = L^-1; T1 B T1^T = U diag(psi) U^T by descending psi, floored at 0; transform = U^T T1."""
    num_em_iters = int(num_em_iters)
    if num_em_iters < 0:
        raise ValueError("plda_from_stats: num_em_iters must be >= 0")
    d, s_cls, n_rows = stats.dim, stats.num_classes, stats.n
    offset_scatter = stats.total - stats.between
    offset_scatter = 0.5 * (offset_scatter + offset_scatter.T)
    mean = stats.means.sum(axis=0) / float(s_cls)
    centred = stats.means - mean[None, :]
    groups = [(float(n), centred[stats.counts == n]) for n in np.unique(stats.counts)]
    w_var, b_var = np.eye(d), np.eye(d)
    for _ in range(num_em_iters):
        w_inv, b_inv = np.linalg.inv(w_var), np.linalg.inv(b_var)
        w_stats, w_count = offset_scatter.copy(), float(n_rows - s_cls)
        b_stats, b_count = np.zeros((d, d)), 0.0
        for n, m in groups:
            k = float(m.shape[0])
            mix = np.linalg.inv(b_inv + n * w_inv)
            mix = 0.5 * (mix + mix.T)
            w = (n * m) @ w_inv @ mix                 # rows: M (n W^-1 m), both matrices symmetric
            r = m - w
            b_stats += k * mix + w.T @ w
            b_count += k
            w_stats += n * (k * mix + r.T @ r)
            w_count += k
        w_var = w_stats / w_count
        b_var = b_stats / b_count
        w_var, b_var = 0.5 * (w_var + w_var.T), 0.5 * (b_var + b_var.T)
    t1 = np.linalg.inv(np.linalg.cholesky(w_var))
    psi, u = _eigh_descending(t1 @ b_var @ t1.T)
    model = plda_mod.Plda(mean, u.T @ t1, np.maximum(psi, 0.0))
    model.within_var, model.between_var = w_var, b_var
    return model


# ----------------------------------------------------------------------------- shared by the three commands
def read_utt2spk(path):
    """Kaldi `ark:utt2spk` text table -> {utt: spk}."""
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if len(p) != 2:
                raise ValueError("%s:%d: expected `utt spk`, got %r" % (path, no, line.rstrip("\n")))
            out[p[0]] = p[1]
    return out


def table_path(specifier):
    """`ark:path` / `ark,t:path` / `path` -> path."""
    return specifier.split(":", 1)[1] if ":" in specifier.split("/")[0] else specifier


def front(x, mean, transform, normalize_length, device):
    """The in-pipe steps of the recipe on the device: ivector-subtract-global-mean | transform-vec | ivector-normalize-length
    (scoring.prepare; Kaldi's default --scaleup=true: unit rows times sqrt(dim)) -> float32 tensor on the device."""
    if mean is None and transform is None and not normalize_length:
        return scoring._rows(x, device, "x")
    rows = scoring.prepare(x, mean=mean, transform=transform, normalize=normalize_length, eps=0.0, device=device, as_tensor=True)
    if normalize_length:
        rows *= float(np.sqrt(rows.shape[1]))
    return rows
