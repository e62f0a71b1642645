"""ORACLE (test infrastructure only) of back-end training, numpy, float64 throughout: a literal transcription of the loops of
Kaldi's ivector-compute-lda.cc (CovarianceStats::AccStats one speaker at a time, ComputeAndSubtractMean, ComputeLda) and of
plda.cc (PldaStats::AddSamples one speaker at a time, PldaEstimator with GetStatsFromIntraClass / GetStatsFromClassMeans class
by class, no grouping by n, GetOutput).  tf_kaldi_speaker_amd.backend works from recentred sufficient statistics and groups
the classes by n: same numbers, different order.  Kaldi is absent from the reference tree: the published sources are
restated (**parity unpinned**, as tests/helpers/ref_plda.py)."""
import numpy as np


def groups(x, labels):
    """Rows of x per class, classes in sorted label order, rows in their order in x."""
    x = np.asarray(x, np.float64)
    labels = np.asarray(labels)
    return [x[labels == s] for s in np.unique(labels)]


def numpy_stats(x, labels, center=None):
    """The fields of backend.Stats straight from the rows, vectorised (host tests build their Stats from this)."""
    x = np.asarray(x, np.float64)
    ids, inverse, counts = np.unique(np.asarray(labels), return_inverse=True, return_counts=True)
    sums = np.zeros((ids.shape[0], x.shape[1]))
    np.add.at(sums, inverse.reshape(-1), x)
    means = sums / counts[:, None]
    mean = x.mean(axis=0)
    c = mean if center is None else np.asarray(center, np.float64)
    y, m = x - c[None, :], means - c[None, :]
    return dict(counts=counts.astype(np.float64), means=means, mean=mean, center=c, total=y.T @ y, between=(m * counts[:, None]).T @ m)


def normalizing_transform(covar, floor):
    """ComputeNormalizingTransform of ivector-compute-lda.cc: covar = U diag(s) U^T, s floored at max(s) * floor, rows of U^T
    scaled by s^-1/2."""
    s, u = np.linalg.eigh(covar)
    s = np.maximum(s, s.max() * floor)
    return (u * (s ** -0.5)[None, :]).T


def lda(x, labels, dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """ivector-compute-lda -> [dim, d + 1] float64."""
    spk = groups(x, labels)
    num = sum(g.shape[0] for g in spk)
    mean = np.zeros(spk[0].shape[1])
    for g in spk:                                   # ComputeAndSubtractMean
        for row in g:
            mean += row
    mean /= num
    spk = [g - mean[None, :] for g in spk]
    d = mean.shape[0]
    tot_covar, between_covar, num_utt = np.zeros((d, d)), np.zeros((d, d)), 0
    for g in spk:                                   # CovarianceStats::AccStats
        tot_covar += g.T @ g
        avg = g.sum(axis=0) / g.shape[0]
        between_covar += g.shape[0] * np.outer(avg, avg)
        num_utt += g.shape[0]
    total = tot_covar / num_utt
    within = total - between_covar / num_utt
    t = normalizing_transform(total_covariance_factor * total + (1.0 - total_covariance_factor) * within, covariance_floor)
    proj = t @ (total - within) @ t.T
    s, u = np.linalg.eigh(0.5 * (proj + proj.T))
    u = u[:, np.argsort(-s, kind="stable")]         # SortSvd
    a = u[:, :dim].T @ t
    return np.concatenate([a, -(a @ mean)[:, None]], axis=1)


def plda(x, labels, num_em_iters=10):
    """ivector-compute-plda -> dict(mean, transform, psi, within_var, between_var)."""
    spk = groups(x, labels)
    d = spk[0].shape[1]
    offset_scatter, total_sum = np.zeros((d, d)), np.zeros(d)
    class_info, class_weight, example_weight = [], 0.0, 0.0
    for g in spk:                                   # PldaStats::AddSamples(weight 1)
        n = g.shape[0]
        mean = g.sum(axis=0) / n
        offset_scatter += g.T @ g
        offset_scatter += -float(n) * np.outer(mean, mean)
        class_info.append((1.0, mean, n))
        class_weight += 1.0
        example_weight += n
        total_sum += mean
    within_var, between_var = np.eye(d), np.eye(d)
    for _ in range(num_em_iters):                   # PldaEstimator::EstimateOneIter
        within_stats, within_count = np.zeros((d, d)), 0.0
        between_stats, between_count = np.zeros((d, d)), 0.0
        within_stats += offset_scatter              # GetStatsFromIntraClass
        within_count += example_weight - class_weight
        between_inv, within_inv = np.linalg.inv(between_var), np.linalg.inv(within_var)
        for weight, mean, n in class_info:          # GetStatsFromClassMeans
            m = mean - total_sum / class_weight
            mixed_var = np.linalg.inv(between_inv + n * within_inv)
            w = mixed_var @ (n * (within_inv @ m))
            m_w = m - w
            between_stats += weight * mixed_var
            between_stats += weight * np.outer(w, w)
            between_count += weight
            within_stats += weight * n * mixed_var
            within_stats += weight * n * np.outer(m_w, m_w)
            within_count += weight
        within_var = within_stats / within_count    # EstimateFromStats
        between_var = between_stats / between_count
    mean = total_sum / class_weight                 # GetOutput
    transform1 = np.linalg.inv(np.linalg.cholesky(0.5 * (within_var + within_var.T)))
    proj = transform1 @ between_var @ transform1.T
    s, u = np.linalg.eigh(0.5 * (proj + proj.T))
    order = np.argsort(-s, kind="stable")
    s, u = np.maximum(s[order], 0.0), u[:, order]
    return dict(mean=mean, transform=u.T @ transform1, psi=s, within_var=within_var, between_var=between_var)
