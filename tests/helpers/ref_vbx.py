"""ORACLE (test infrastructure only) of the VB-HMM resegmentation of x-vector sequences (xv_vbx, csrc/vbx.hip): the rule of
include/xvec_hip.h in numpy, parameterised by dtype.  float64 is the oracle the GPU is compared with; np.longdouble is the
same chain rounded independently, and |float64 - longdouble| is the measure of what rounding alone does to an output.  The
rule follows Landini et al., "Bayesian HMM clustering of x-vector sequences (VBx)", 2022, as the published VB_diarization.py
states it; neither the reference tree nor Kaldi's x-vector recipe has the step: **parity unpinned**."""
import collections

import numpy as np

import ref_plda

Result = collections.namedtuple("Result", ["gamma", "pi", "elbo", "iters", "labels", "max_logp"])

DEFAULTS = dict(fa=0.3, fb=17.0, loop_prob=0.99, max_iters=40, epsilon=1e-6)


def model_affine(mean, transform, psi, lda_dim=None):
    """(A [r, D + 1], psi [r]) of a Plda (mean, transform, psi): A = [transform | -transform mean], the first lda_dim rows."""
    transform = np.asarray(transform, np.float64)
    a = np.concatenate([transform, -(transform @ np.asarray(mean, np.float64))[:, None]], axis=1)
    k = a.shape[0] if lda_dim is None else int(lda_dim)
    return np.ascontiguousarray(a[:k]), np.ascontiguousarray(np.asarray(psi, np.float64)[:k])


def init_gamma(labels, num_spk, smoothing=5.0):
    """Row softmax of smoothing * onehot(label) [T, S] and pi = 1 / S."""
    labels = np.asarray(labels, np.int64)
    z = np.zeros((labels.shape[0], num_spk))
    z[np.arange(labels.shape[0]), labels] = smoothing
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True), np.full(num_spk, 1.0 / num_spk)


def _lse_rows(v, dt):
    """log sum exp over the last axis with the maximum taken out; an all -inf row gives -inf, not NaN."""
    m = np.max(v, axis=-1)
    m0 = np.where(np.isfinite(m), m, dt(0))
    with np.errstate(divide="ignore"):
        return m0 + np.log(np.sum(np.exp(v - m0[..., None]), axis=-1, dtype=dt))


def project(x, a, psi, dtype=np.float64):
    """Step 1: rho [T, r] and G [T]."""
    dt = dtype
    a, psi = np.asarray(a, dt), np.asarray(psi, dt)
    x = np.asarray(x, np.float32).astype(dt)
    u = x @ a[:, :-1].T + a[:, -1][None, :]
    r = a.shape[0]
    two_pi = dt(8) * np.arctan(dt(1))                   # 2 pi in the precision of dt
    g = dt(-0.5) * (np.sum(u * u, axis=1, dtype=dt) + dt(r) * np.log(two_pi))
    return u * np.sqrt(psi)[None, :], g


def vb_hmm(x, a, psi, gamma, pi, fa=0.3, fb=17.0, loop_prob=0.99, max_iters=40, epsilon=1e-6, dtype=np.float64, dense=False):
    """The rule, steps 1-4, on one recording x [T, D] (T >= 1) -> Result.  `dense` runs the forward and backward passes over
    the full [S, S] transition matrix instead of its diagonal-plus-rank-one form (the same sums in another order)."""
    dt = dtype
    rho, g = project(x, a, psi, dt)
    psi = np.asarray(psi, dt)
    gamma, pi = np.array(gamma, dt), np.array(pi, dt)
    t_len, s = gamma.shape
    fa, fb, lp = dt(fa), dt(fb), dt(loop_prob)
    ratio = fa / fb
    elbo, max_logp = [], 0.0
    for it in range(int(max_iters)):
        n = np.sum(gamma, axis=0, dtype=dt)
        inv_l = dt(1) / (dt(1) + ratio * n[:, None] * psi[None, :])
        alpha = ratio * inv_l * (gamma.T @ rho)
        logp = fa * (rho @ alpha.T - dt(0.5) * ((inv_l + alpha * alpha) @ psi)[None, :] + g[:, None])
        max_logp = max(max_logp, float(np.max(np.abs(logp))))
        with np.errstate(divide="ignore"):
            log_pi = np.log(pi)
        lfw = np.empty((t_len, s), dt)
        lbw = np.zeros((t_len, s), dt)
        lse = np.empty(t_len, dt)
        lfw[0] = logp[0] + log_pi
        if dense:
            tr = lp * np.eye(s, dtype=dt) + (dt(1) - lp) * pi[None, :]
        with np.errstate(divide="ignore"):
            for t in range(1, t_len):
                m = np.max(lfw[t - 1])
                m0 = m if np.isfinite(m) else dt(0)
                e = np.exp(lfw[t - 1] - m0)
                tot = np.sum(e, dtype=dt)
                lse[t - 1] = m0 + np.log(tot)
                mix = e @ tr if dense else lp * e + (dt(1) - lp) * pi * tot
                lfw[t] = logp[t] + m0 + np.log(mix)
            lse[t_len - 1] = _lse_rows(lfw[t_len - 1], dt)
            for t in range(t_len - 2, -1, -1):
                v = logp[t + 1] + lbw[t + 1]
                m = np.max(v)
                m0 = m if np.isfinite(m) else dt(0)
                b = np.exp(v - m0)
                mix = tr @ b if dense else lp * b + (dt(1) - lp) * np.sum(pi * b, dtype=dt)
                lbw[t] = m0 + np.log(mix)
        tll = lse[t_len - 1]
        gamma = np.exp(lfw + lbw - tll)
        elbo.append(tll + fb / dt(2) * np.sum(np.log(inv_l) - inv_l - alpha * alpha + dt(1), dtype=dt))
        acc = np.sum(np.exp(lse[:-1, None] + logp[1:] + lbw[1:] - tll), axis=0, dtype=dt) if t_len > 1 else np.zeros(s, dt)
        pi = gamma[0] + (dt(1) - lp) * pi * acc
        pi = pi / np.sum(pi, dtype=dt)
        if it > 0 and elbo[-1] - elbo[-2] < epsilon:
            break
    iters = len(elbo)
    row = np.full(int(max_iters), np.nan, dt)
    row[:iters] = elbo
    return Result(gamma, pi, row, iters, np.argmax(gamma, axis=1).astype(np.int32), max_logp)


def floor(t_len, r, s, max_logp):
    """The floor of an error bar: one rounding per term of the longest chain, (2 T + 2)(r + S + 8) 2^-53 max(1, max|logp|)."""
    return (2 * t_len + 2) * (r + s + 8) * 2.0 ** -53 * max(1.0, max_logp)


def bars(x, a, psi, gamma, pi, **opts):
    """(float64 Result, {output: bar}) with bar = 16 |float64 - longdouble| elementwise + the floor, for gamma, pi and elbo.
    The longdouble run takes as many iterations as the float64 run (epsilon = -inf, max_iters = its count)."""
    ref = vb_hmm(x, a, psi, gamma, pi, dtype=np.float64, **opts)
    wide_opts = dict(opts, epsilon=-np.inf, max_iters=ref.iters)
    wide = vb_hmm(x, a, psi, gamma, pi, dtype=np.longdouble, **wide_opts)
    fl = floor(np.shape(x)[0], np.shape(a)[0], np.shape(gamma)[1], ref.max_logp)
    out = {"gamma": 16.0 * np.abs(ref.gamma - wide.gamma).astype(np.float64) + fl,
           "pi": 16.0 * np.abs(ref.pi - wide.pi).astype(np.float64) + fl,
           "elbo": 16.0 * np.abs(ref.elbo[:ref.iters] - wide.elbo[:ref.iters]).astype(np.float64) + fl}
    return ref, out


def draw_model(rng, r, extra=3):
    """A random model of dimension r behind rows of dimension D = r + extra (D != r on purpose) -> (A [r, D + 1], psi [r])."""
    d = r + extra
    _, _, psi = ref_plda.random_model(rng, r)
    return np.concatenate([rng.standard_normal((r, d)) / np.sqrt(d), 0.1 * rng.standard_normal((r, 1))], axis=1), psi


def draw_rows(rng, a, psi, t_len, s, speakers, scale=1.0, noise_labels=0.2, run=10):
    """Rows of the model (A, psi): speaker means y ~ scale N(0, diag(psi)), unit noise, speaker runs of `run` rows; initial
    labels = the truth with a share `noise_labels` of rows relabelled at random among S -> (x [T, D] float32, init [T], truth [T])."""
    r = a.shape[0]
    y = scale * rng.standard_normal((speakers, r)) * np.sqrt(psi)[None, :]
    runs = (t_len + run - 1) // run
    who = rng.integers(0, speakers, runs)
    truth = np.repeat(who, run)[:t_len]
    u = y[truth] + rng.standard_normal((t_len, r))
    # x with A [x; 1] = u: the least-norm solution of the r equations in D unknowns
    x = np.ascontiguousarray(np.linalg.lstsq(a[:, :-1], (u - a[:, -1][None, :]).T, rcond=None)[0].T, dtype=np.float32)
    init = np.minimum(truth, s - 1).astype(np.int64)
    flip = rng.random(t_len) < noise_labels
    init[flip] = rng.integers(0, s, int(flip.sum()))
    return x, init, truth


def case(t_len, r, s, speakers, scale=1.0, seed=0, extra=3, noise_labels=0.2, run=10):
    """One recording of a model of its own -> (x [T, D] float32, A [r, D + 1], psi [r], init labels [T], truth [T])."""
    rng = np.random.default_rng(1000 * seed + 7 * t_len + 3 * r + s)
    a, psi = draw_model(rng, r, extra)
    x, init, truth = draw_rows(rng, a, psi, t_len, s, speakers, scale, noise_labels, run)
    return x, a, psi, init, truth
