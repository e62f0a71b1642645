"""ORACLE (test infrastructure only) of the PLDA scoring feature, numpy, float64 throughout: Kaldi's Plda::TransformIvector
and Plda::LogLikelihoodRatio in the form of plda.cc (not the expansion the GPU evaluates), `ivector-copy-plda --smoothing`,
the minimum DCF of sid/compute_min_dcf.py as a loop over every threshold, and an independent derivation of the log
likelihood ratio from the generative model.  Kaldi is absent from the reference tree: the Kaldi steps follow the published
algorithms (**parity unpinned**, as tests/helpers/ref_score.py)."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def transform_ivector(mean, transform, psi, x, n=1, normalize_length=True, simple_length_norm=False):
    """Rows x [r, D] with utterance counts n (scalar or [r]) -> [r, D]: u = transform (x - mean), then
    u sqrt(D / sum_d u_d^2 / (psi_d + 1 / n)) (normalize_length), or u sqrt(D) / ||u|| (simple).  A zero u stays zero."""
    u = (np.asarray(x, np.float64) - np.asarray(mean, np.float64)[None, :]) @ np.asarray(transform, np.float64).T
    if not normalize_length:
        return u
    d = u.shape[1]
    n = np.broadcast_to(np.asarray(n, np.float64), (u.shape[0],))
    if simple_length_norm:
        ss = np.sum(u * u, axis=1)
    else:
        ss = np.sum(u * u / (np.asarray(psi, np.float64)[None, :] + 1.0 / n[:, None]), axis=1)
    return u * np.where(ss > 0.0, np.sqrt(d / np.where(ss > 0.0, ss, 1.0)), 0.0)[:, None]


def llr(psi, e, n, t):
    """LogLikelihoodRatio of plda.cc for every enrolment row e [r, D] (counts n, scalar or [r]) against every test row
    t [m, D] -> [r, m]: mean = n psi / (n psi + 1) e, variance = 1 + psi / (n psi + 1);
    loglike_given_class = -1/2 (sum log variance + sum (t - mean)^2 / variance), loglike_without_class =
    -1/2 (sum log(1 + psi) + sum t^2 / (1 + psi)); the D log(2 pi) terms cancel."""
    psi = np.asarray(psi, np.float64)
    e, t = np.asarray(e, np.float64), np.asarray(t, np.float64)
    n = np.broadcast_to(np.asarray(n, np.float64), (e.shape[0],))
    out = np.empty((e.shape[0], t.shape[0]))
    without = -0.5 * (np.sum(np.log(1.0 + psi)) + np.sum(t * t / (1.0 + psi)[None, :], axis=1))
    for i in range(e.shape[0]):
        mean = n[i] * psi / (n[i] * psi + 1.0) * e[i]
        var = 1.0 + psi / (n[i] * psi + 1.0)
        given = -0.5 * (np.sum(np.log(var)) + np.sum((t - mean[None, :]) ** 2 / var[None, :], axis=1))
        out[i] = given - without
    return out


def llr_pairs(psi, e, n, t, ia, ib):
    psi = np.asarray(psi, np.float64)
    e, t = np.asarray(e, np.float64)[ia], np.asarray(t, np.float64)[ib]
    n = np.broadcast_to(np.asarray(n, np.float64), (np.max(ia) + 1 if np.ndim(n) == 0 else np.shape(n)[0],))[ia][:, None]
    mean = n * psi / (n * psi + 1.0) * e
    var = 1.0 + psi / (n * psi + 1.0)
    given = -0.5 * (np.sum(np.log(var), axis=1) + np.sum((t - mean) ** 2 / var, axis=1))
    without = -0.5 * (np.sum(np.log(1.0 + psi)) + np.sum(t * t / (1.0 + psi), axis=1))
    return given - without


def llr_gaussian(psi, e, n, t):
    """The same ratio from the generative model, independently: per dimension the enrolment mean (of n utterances) and the
    test vector of one speaker are jointly Gaussian with covariance [[psi + 1/n, psi], [psi, psi + 1]]; of different
    speakers they are independent with the same marginals.  LLR = log N(joint) - log N(e) - log N(t), summed over d."""
    psi = np.asarray(psi, np.float64)
    e, t = np.asarray(e, np.float64), np.asarray(t, np.float64)
    n = np.broadcast_to(np.asarray(n, np.float64), (e.shape[0],))
    out = np.empty((e.shape[0], t.shape[0]))
    for i in range(e.shape[0]):
        a, b, c = psi + 1.0 / n[i], psi, psi + 1.0            # [[a, b], [b, c]]
        det = a * c - b * b
        x, y = e[i][None, :], t
        joint = -0.5 * (np.log(det)[None, :] + (c * x * x - 2.0 * b * x * y + a * y * y) / det[None, :])
        marg = -0.5 * (np.log(a) + x * x / a) - 0.5 * (np.log(c)[None, :] + y * y / c[None, :])
        out[i] = np.sum(joint - marg, axis=1)
    return out


def score_bar(a, b, rho, tau=None):
    """The derived bar of one GPU score s = sum_k a_ik b_jk + rho_i + tau_j (tests/test_gpu_plda.py has the derivation) from
    the packed fp32 operands a [n, K], b [m, K] and the biases rho [n], tau [m] (None: 0) as the device holds them ->
    (K, (K + 8) u sum_k |a_ik b_jk| [n, m], 4 u (|rho_i| + |tau_j|) [n, m]); the caller adds 4 u |s_ref|."""
    a, b = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    k = a.shape[1]
    rho = np.abs(np.asarray(rho, np.float64))
    tau = np.zeros(b.shape[0]) if tau is None else np.abs(np.asarray(tau, np.float64))
    return k, (k + 8) * U * (a @ b.T), 4 * U * (rho[:, None] + tau[None, :])


def smooth(mean, transform, psi, factor):
    """ivector-copy-plda --smoothing: within-class covariance I -> w = 1 + factor psi; psi / w, diag(w^-1/2) transform."""
    w = 1.0 + factor * np.asarray(psi, np.float64)
    return np.array(mean, np.float64), np.asarray(transform, np.float64) * (w ** -0.5)[:, None], np.asarray(psi, np.float64) / w


def min_dcf(scores, targets, p_target, c_miss=1.0, c_fa=1.0):
    """Brute force: every score and +inf as the threshold x; miss = target < x, false alarm = nontarget >= x."""
    s, t = np.asarray(scores, np.float64), np.asarray(targets, bool)
    best = np.inf
    for x in list(s) + [np.inf]:
        p_miss = np.sum(s[t] < x) / float(np.sum(t))
        p_fa = np.sum(s[~t] >= x) / float(np.sum(~t))
        best = min(best, c_miss * p_miss * p_target + c_fa * p_fa * (1.0 - p_target))
    return best / min(c_miss * p_target, c_fa * (1.0 - p_target))


def random_model(rng, d, cond=4.0):
    """mean, a well-conditioned transform (orthogonal x singular values in 1 / cond..1), psi log-uniform in 1e-3..1e2
    sorted descending, as Kaldi leaves it."""
    q1, _ = np.linalg.qr(rng.standard_normal((d, d)))
    q2, _ = np.linalg.qr(rng.standard_normal((d, d)))
    transform = (q1 * np.exp(rng.uniform(-np.log(cond), 0.0, d))[None, :]) @ q2
    psi = np.sort(np.exp(rng.uniform(np.log(1e-3), np.log(1e2), d)))[::-1].copy()
    return 0.5 * rng.standard_normal(d), transform, psi


def draw(rng, mean, transform, psi, speakers, per, noise=1.0):
    """Utterances of the model itself: y ~ N(0, diag(psi)) per speaker, y + noise N(0, I) per utterance, mapped back
    through transform^-1 and mean -> (x [speakers * per, D] float64, labels)."""
    d = psi.shape[0]
    y = rng.standard_normal((speakers, d)) * np.sqrt(psi)[None, :]
    u = np.repeat(y, per, axis=0) + noise * rng.standard_normal((speakers * per, d))
    x = np.linalg.solve(transform, u.T).T + mean[None, :]
    return x, np.repeat(np.arange(speakers), per)
