"""The calibration rules of include/xvec_hip.h (xv_logreg_stats, xv_score_fuse) and tf_kaldi_speaker_amd.calibration in
float64 numpy: the oracle of tests/test_calibration_host.py and tests/test_gpu_calibration.py.  Nothing here is shared with
the code under test."""
import math

import numpy as np


def llr(scores, theta):
    """((w_1 s_1 + w_2 s_2) + ...) + b in double, ascending k, bias last, separate multiply and add."""
    s = np.asarray(scores, dtype=np.float32)
    if s.ndim == 1:
        s = s[:, None]
    theta = np.asarray(theta, dtype=np.float64)
    k = s.shape[1]
    acc = theta[0] * s[:, 0].astype(np.float64)
    for j in range(1, k):
        acc = acc + theta[j] * s[:, j].astype(np.float64)
    return acc + theta[k]


def fuse(scores, theta):
    with np.errstate(over="ignore", invalid="ignore"):
        return llr(scores, theta).astype(np.float32)


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigma(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def stats(scores, targets, theta, tau, c_tar, c_non, thresholds=(), exact=True):
    """-> dict: F, g, H and the sums of the absolute values of their terms (aF, ag, aH), the counts n_tar, n_non, bad and
    miss / fa per threshold.  A row with a score that is not finite is counted in bad and left out of everything else.
    The sums are math.fsum (exactly rounded) unless `exact` is off (numpy's pairwise sums: what a Newton iteration needs)."""
    fsum = math.fsum if exact else np.sum
    s = np.asarray(scores, dtype=np.float32)
    if s.ndim == 1:
        s = s[:, None]
    t = np.asarray(targets).reshape(-1) != 0
    ok = np.all(np.isfinite(s), axis=1)
    bad = int(np.count_nonzero(~ok))
    s, t = s[ok], t[ok]
    n, k = s.shape
    l = llr(s, theta) if n else np.zeros(0)
    a = np.concatenate([s.astype(np.float64), np.ones((n, 1))], axis=1)
    z = l + tau
    c = np.where(t, c_tar, c_non)
    tf = c * np.where(t, softplus(-z), softplus(z))
    r = np.where(t, -sigma(-z), sigma(z))
    tg = (c * r)[:, None] * a
    ch = c * sigma(z) * sigma(-z)
    with np.errstate(over="ignore"):
        lf = l.astype(np.float32).astype(np.float64)
    H, aH = np.zeros((k + 1, k + 1)), np.zeros((k + 1, k + 1))
    for i in range(k + 1):
        for j in range(i, k + 1):
            th = ch * a[:, i] * a[:, j]
            H[i, j] = H[j, i] = fsum(th)
            aH[i, j] = aH[j, i] = fsum(np.abs(th))
    out = dict(F=fsum(tf), aF=fsum(np.abs(tf)),
               g=np.array([fsum(tg[:, i]) for i in range(k + 1)]),
               ag=np.array([fsum(np.abs(tg[:, i])) for i in range(k + 1)]), H=H, aH=aH,
               n_tar=int(np.count_nonzero(t)), n_non=int(np.count_nonzero(~t)), bad=bad,
               miss=np.array([np.count_nonzero(t & (lf < eta)) for eta in thresholds], dtype=np.int64),
               fa=np.array([np.count_nonzero(~t & (lf >= eta)) for eta in thresholds], dtype=np.int64))
    return out


def class_weights(targets, prior):
    t = np.asarray(targets).reshape(-1) != 0
    return prior / np.count_nonzero(t), (1.0 - prior) / np.count_nonzero(~t)


def objective(scores, targets, prior):
    """theta -> (F, g, H) at prior `prior`, the callable calibration.newton takes."""
    c_tar, c_non = class_weights(targets, prior)
    tau = math.log(prior / (1.0 - prior))

    def f(theta):
        st = stats(scores, targets, theta, tau, c_tar, c_non, exact=False)
        return st["F"], st["g"], st["H"]
    return f


def decrement(scores, targets, prior, theta):
    F, g, H = objective(scores, targets, prior)(theta)
    return float(g @ np.linalg.solve(H, g)), H


def cllr(l, targets):
    l = np.asarray(l, dtype=np.float32).astype(np.float64)
    t = np.asarray(targets).reshape(-1) != 0
    return (np.mean(softplus(-l[t])) + np.mean(softplus(l[~t]))) / (2.0 * math.log(2.0))


def act_dcf(l, targets, p_target, c_miss=1.0, c_fa=1.0):
    l = np.asarray(l, dtype=np.float32).astype(np.float64)
    t = np.asarray(targets).reshape(-1) != 0
    eta = math.log(c_fa * (1.0 - p_target) / (c_miss * p_target))
    p_miss = np.count_nonzero(l[t] < eta) / float(np.count_nonzero(t))
    p_fa = np.count_nonzero(l[~t] >= eta) / float(np.count_nonzero(~t))
    return (c_miss * p_miss * p_target + c_fa * p_fa * (1.0 - p_target)) / min(c_miss * p_target, c_fa * (1.0 - p_target))


def fixture(k, n, seed, target_rate=0.2):
    """Seeded, overlapping scores: class means at +-6, standard deviation 4 (j + 1) for system j, 20 % targets, at least one
    trial of each class -> (scores [n, k] float32, targets [n] bool)."""
    rs = np.random.RandomState(seed)
    t = rs.rand(n) < target_rate
    t[0], t[1] = True, False
    base = np.where(t, 6.0, -6.0)[:, None]
    s = base + 4.0 * rs.standard_normal((n, k)) * (1.0 + np.arange(k))
    return s.astype(np.float32), t


FIT_SIZES = {1: 2000, 2: 3001, 3: 777, 8: 5000}          # k -> n; the seed is 10 + k
FIT_CASES = [(k, prior) for k in (1, 2, 3, 8) for prior in (0.01, 0.05, 0.5)]
_fits = {}


def fit_case(k, prior, newton):
    """The fixture of (k, prior) and the oracle's own fit of it by `newton` (calibration.newton: host numpy), computed once
    -> (scores, targets, theta, report, lambda_min of the oracle's Hessian at theta)."""
    if (k, prior) not in _fits:
        s, t = fixture(k, FIT_SIZES[k], 10 + k)
        theta, report = newton(objective(s, t, prior), k)
        H = objective(s, t, prior)(theta)[2]
        _fits[(k, prior)] = (s, t, theta, report, float(np.linalg.eigvalsh(H).min()))
    return _fits[(k, prior)]
