"""Score calibration and fusion on the GPU (csrc/calibrate.hip through the C ABI: xv_logreg_stats / xv_score_fuse): an affine
map from the scores of K systems (1 <= K <= 8) to a log-likelihood ratio, fitted by prior-weighted logistic regression on a
development trial list, and the two metrics that judge it, Cllr and the actual DCF at the Bayes threshold.  The reference's
only answer is misc/utils/average_score.py, the equal-weight mean of two score files, which is Model([0.5, 0.5], 0.0) here;
its recipes leave calibration to outside tools: **parity unpinned**.  include/xvec_hip.h states the rules and
tests/helpers/ref_calibration.py restates them in float64 numpy.

    llr_i = ((w_1 s_i1 + w_2 s_i2) + ...) + b                       double, this order, no fused multiply-add; float32 out
    F(theta) = pi / N_tar sum_tar softplus(-z_i) + (1 - pi) / N_non sum_non softplus(z_i),   z_i = llr_i + log(pi / (1 - pi))
    Cllr = (mean_tar softplus(-llr) + mean_non softplus(llr)) / (2 ln 2)
    actDCF = the cost of scoring.min_dcf at the one threshold eta = log(c_fa (1 - p) / (c_miss p))

The pass over the trials (F, its gradient and Hessian, the error counts) runs on the device, in double, without atomics: a
result is a pure function of its inputs.  The (K + 1) x (K + 1) Newton step is host numpy (newton).  Arrays go in as numpy
or as device tensors, like scoring.py.  No CPU path: without a HIP device everything here except Model, newton,
read_model and write_model raises RuntimeError."""
import collections
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ptr
from .scoring import _need_device

MAX_SYSTEMS = _lib.XV_LOGREG_MAX_SYSTEMS
MAX_THRESHOLDS = _lib.XV_LOGREG_MAX_THRESHOLDS

Stats = collections.namedtuple("Stats", ["F", "g", "H", "n_tar", "n_non", "bad", "miss", "fa"])
Report = collections.namedtuple("Report", ["iterations", "F", "decrement"])


class Model(object):
    """llr = sum_k weights[k] * score_k + bias, fitted at `prior` (kept for the record: applying the model does not use it)."""

    def __init__(self, weights, bias=0.0, prior=0.01):
        self.weights = np.array(weights, dtype=np.float64).reshape(-1)
        self.bias = float(bias)
        self.prior = float(prior)
        if not 1 <= self.weights.size <= MAX_SYSTEMS:
            raise ValueError("a model has 1..%d weights, got %d" % (MAX_SYSTEMS, self.weights.size))
        _check_prior(self.prior)

    @property
    def theta(self):
        return np.concatenate([self.weights, [self.bias]])

    def __repr__(self):
        return "Model(weights=%r, bias=%r, prior=%r)" % (self.weights.tolist(), self.bias, self.prior)


def _check_prior(prior):
    if not 0.0 < prior < 1.0:
        raise ValueError("the prior must lie in (0, 1), got %r" % (prior,))


def write_model(path, model):
    """Text that holds only numbers: `prior`, `bias` and one `weight` line per system, %.17g (a round trip is exact)."""
    with open(path, "w") as f:
        f.write("prior %.17g\nbias %.17g\n" % (model.prior, model.bias))
        f.write("".join("weight %.17g\n" % w for w in model.weights))


def read_model(path):
    prior = bias = None
    weights = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            try:
                if len(p) != 2 or p[0] not in ("prior", "bias", "weight"):
                    raise ValueError
                v = float(p[1])
            except ValueError:
                raise ValueError("%s:%d: expected `prior|bias|weight <number>`, got %r" % (path, no, line.rstrip("\n")))
            if p[0] == "weight":
                weights.append(v)
            elif p[0] == "prior" and prior is None:
                prior = v
            elif p[0] == "bias" and bias is None:
                bias = v
            else:
                raise ValueError("%s:%d: a second `%s` line" % (path, no, p[0]))
    if prior is None or bias is None or not weights:
        raise ValueError("%s: a model needs a prior, a bias and at least one weight" % path)
    return Model(weights, bias, prior)


# --------------------------------------------------------------------------------------------------- device calls
def _scores(x, device):
    """[n, K] float32 on cuda:device (a 1-D array is one system) -> (tensor, n, K, row stride).  A 2-D device tensor whose
    rows are contiguous is taken as it is, padding columns and all."""
    torch = _need_device()
    if isinstance(x, torch.Tensor):
        t = x.to(device="cuda:%d" % device, dtype=torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda:%d" % device)
    if t.dim() == 1:
        t = t.reshape(-1, 1)
    if t.dim() != 2:
        raise ValueError("scores: expected a [n, K] array, got shape %s" % (tuple(t.shape),))
    n, k = int(t.shape[0]), int(t.shape[1])
    if not 1 <= k <= MAX_SYSTEMS:
        raise ValueError("scores of %d systems: 1..%d are supported" % (k, MAX_SYSTEMS))
    if n > 1 and (t.stride(1) != 1 or t.stride(0) < k):
        t = t.contiguous()
    lds = int(t.stride(0)) if n > 1 else k
    if n == 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, n, k, lds


def _targets(t, n, device):
    torch = _need_device()
    if isinstance(t, torch.Tensor):
        d = (t != 0).to(device="cuda:%d" % device, dtype=torch.uint8).reshape(-1).contiguous()
    else:
        d = torch.from_numpy(np.ascontiguousarray(np.asarray(t).reshape(-1) != 0).view(np.uint8)).to("cuda:%d" % device)
    if d.numel() != n:
        raise ValueError("%d targets for %d trials" % (d.numel(), n))
    return d


_ws = {}        # device -> uint8 tensor, kept between calls and grown on demand


def _stats_dev(sd, n, k, lds, td, theta, tau, c_tar, c_non, thresholds, device):
    """xv_logreg_stats on operands that live on cuda:device -> Stats (waits for the result)."""
    torch = _need_device()
    lib = _lib.load()
    theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
    if theta.size != k + 1:
        raise ValueError("theta: %d entries for %d systems" % (theta.size, k))
    thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if thr.size > MAX_THRESHOLDS:
        raise ValueError("at most %d thresholds, got %d" % (MAX_THRESHOLDS, thr.size))
    nd = 1 + (k + 1) + (k + 1) * (k + 2) // 2
    with torch.cuda.device(device):
        need = int(lib.xv_logreg_workspace(n, k))
        if need < 0:
            raise _lib.XvError(need, "xv_logreg_workspace: bad dimensions")
        ws = _ws.get(device)
        if ws is None or ws.numel() < need:
            _ws[device] = ws = torch.empty((max(need, 1 << 16),), dtype=torch.uint8, device=sd.device)
        out = torch.empty((nd,), dtype=torch.float64, device=sd.device)
        cnt = torch.empty((3 + 2 * MAX_THRESHOLDS,), dtype=torch.int64, device=sd.device)
        stream = _lib.stream(device)
        _lib.check(lib.xv_logreg_stats(device, ptr(sd), lds, n, k, ptr(td), C.c_void_p(theta.ctypes.data), float(tau), float(c_tar),
                                       float(c_non), C.c_void_p(thr.ctypes.data) if thr.size else None, thr.size, ptr(out),
                                       ptr(cnt), ptr(ws), ws.numel(), stream))
        o, c = out.cpu().numpy(), cnt.cpu().numpy()
    H = np.zeros((k + 1, k + 1))
    H[np.triu_indices(k + 1)] = o[k + 2:]
    H = H + np.triu(H, 1).T
    return Stats(float(o[0]), o[1:k + 2].copy(), H, int(c[0]), int(c[1]), int(c[2]), c[3:3 + thr.size].copy(),
                 c[3 + MAX_THRESHOLDS:3 + MAX_THRESHOLDS + thr.size].copy())


def _class_weights(targets, prior):
    """(prior / N_tar, (1 - prior) / N_non) from the caller's targets, before anything is sent to the device."""
    if isinstance(targets, np.ndarray) or not hasattr(targets, "is_cuda"):
        t = np.asarray(targets).reshape(-1) != 0
        n_tar, n = int(np.count_nonzero(t)), t.size
    else:
        n_tar, n = int((targets != 0).sum().item()), targets.numel()
    if n_tar == 0 or n_tar == n:
        raise ValueError("calibration needs target and non-target trials (%d, %d)" % (n_tar, n - n_tar))
    return prior / n_tar, (1.0 - prior) / (n - n_tar)


def _no_bad(st):
    if st.bad:
        raise ValueError("%d trials have a score that is not finite" % st.bad)
    return st


def logreg_stats(scores, targets, theta, prior=0.01, thresholds=(), c_tar=None, c_non=None, device=0):
    """One pass of xv_logreg_stats -> Stats(F, g [K + 1], H [K + 1, K + 1] (both triangles), n_tar, n_non, bad, miss, fa).
    `c_tar` / `c_non` default to prior / N_tar and (1 - prior) / N_non with the class counts of `targets` (ValueError when a
    class is empty); tau is log(prior / (1 - prior)).  A row with a score that is not finite is counted in `bad` and left out
    of everything else; nothing is raised for it here (fit, cllr and act_dcf do)."""
    _check_prior(prior)
    if c_tar is None or c_non is None:
        wt, wn = _class_weights(targets, prior)
        c_tar, c_non = wt if c_tar is None else c_tar, wn if c_non is None else c_non
    sd, n, k, lds = _scores(scores, device)
    td = _targets(targets, n, device)
    return _stats_dev(sd, n, k, lds, td, theta, math.log(prior / (1.0 - prior)), c_tar, c_non, thresholds, device)


# --------------------------------------------------------------------------------------------------- the fit
def newton(stats, k, tol=1e-14, max_iter=50):
    """Damped Newton on `stats(theta) -> (F, g, H)` from w = 1 / k, b = 0 -> (theta, Report).  The step is H^-1 g by Cholesky,
    halved until F falls by 1e-4 of step * decrement (Armijo); it stops when the decrement g^T H^-1 g <= tol min(1, F).
    The factor min(1, F) is what makes separable scores fail instead of "converging": on them every step divides F, and
    with it the decrement, by about e, so an absolute 1e-14 would be met after some thirty steps at a weight that means
    nothing, while the decrement never falls below a fixed share of F.  F starts below ln 2 and only falls, so on
    overlapping scores (F of 0.01 .. 0.7 at the optimum) this asks for at most two more digits, which quadratic convergence
    gives within one step.  RuntimeError when the Cholesky factorisation fails, when more than `max_iter` steps are needed
    (both are what linearly separable data produce) or when the line search finds no decrease: it never loops forever and
    never returns a value that is not finite.  Host numpy only: the tests drive it with the numpy oracle, fit binds the
    GPU pass."""
    theta = np.concatenate([np.full(k, 1.0 / k), [0.0]])
    F, g, H = stats(theta)[:3]
    for it in range(max_iter + 1):
        if not (np.isfinite(F) and np.all(np.isfinite(g)) and np.all(np.isfinite(H))):
            raise RuntimeError("calibration: the statistics are not finite at step %d" % it)
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            raise RuntimeError("calibration: the Hessian is not positive definite at step %d (separable or degenerate scores)" % it)
        y = np.linalg.solve(L, g)
        dec = float(y @ y)
        if dec <= tol * min(1.0, F):
            return theta, Report(it, float(F), dec)
        if it == max_iter:
            break
        d = np.linalg.solve(L.T, y)
        step = 1.0
        while True:
            cand = theta - step * d
            Fc, gc, Hc = stats(cand)[:3]
            if np.isfinite(Fc) and Fc <= F - 1e-4 * step * dec:
                break
            step *= 0.5
            if step < 2.0 ** -40:
                raise RuntimeError("calibration: the line search found no decrease at step %d (decrement %g)" % (it, dec))
        theta, F, g, H = cand, Fc, gc, Hc
    raise RuntimeError("calibration: no convergence in %d Newton steps (decrement %g; separable scores?)" % (max_iter, dec))


def fit(scores, targets, prior=0.01, tol=1e-14, max_iter=50, device=0):
    """Fit Model to scores [n, K] (or [n]) and targets [n] (non-zero: target) -> (Model, Report(iterations, F, decrement)).
    ValueError for a prior outside (0, 1), an empty class or a score that is not finite; RuntimeError as newton."""
    _check_prior(prior)
    c_tar, c_non = _class_weights(targets, prior)
    sd, n, k, lds = _scores(scores, device)
    td = _targets(targets, n, device)
    tau = math.log(prior / (1.0 - prior))

    def stats(theta):
        return _no_bad(_stats_dev(sd, n, k, lds, td, theta, tau, c_tar, c_non, (), device))
    theta, report = newton(stats, k, tol=tol, max_iter=max_iter)
    return Model(theta[:k], theta[k], prior), report


def apply(model, scores, device=0, as_tensor=False):
    """scores [n, K] (or [n] for one system) -> llr [n] float32 (xv_score_fuse)."""
    sd, n, k, lds = _scores(scores, device)
    if k != model.weights.size:
        raise ValueError("scores of %d systems for a model of %d" % (k, model.weights.size))
    torch = _need_device()
    lib = _lib.load()
    theta = np.ascontiguousarray(model.theta)
    with torch.cuda.device(device):
        out = torch.empty((n,), dtype=torch.float32, device=sd.device)
        stream = _lib.stream(device)
        _lib.check(lib.xv_score_fuse(device, ptr(sd), lds, n, k, C.c_void_p(theta.ctypes.data), ptr(out), stream))
        return out if as_tensor else out.cpu().numpy()


# --------------------------------------------------------------------------------------------------- the metrics
def bayes_threshold(p_target, c_miss=1.0, c_fa=1.0):
    if not (0.0 < p_target < 1.0) or not c_miss > 0.0 or not c_fa > 0.0:
        raise ValueError("an operating point needs 0 < p_target < 1 and positive costs, got %r, %r, %r" % (p_target, c_miss, c_fa))
    return math.log(c_fa * (1.0 - p_target) / (c_miss * p_target))


def evaluate(llr, targets, points=(), device=0):
    """Cllr and the actual DCF at up to 8 operating points (p_target, c_miss, c_fa) in one pass -> (cllr, [act_dcf ...])."""
    points = [tuple(float(v) for v in p) for p in points]
    thr = [bayes_threshold(*p) for p in points]
    c_tar, c_non = _class_weights(targets, 0.5)
    sd, n, k, lds = _scores(llr, device)
    if k != 1:
        raise ValueError("llr: expected [n] values, got %d columns" % k)
    td = _targets(targets, n, device)
    st = _no_bad(_stats_dev(sd, n, 1, lds, td, [1.0, 0.0], 0.0, c_tar, c_non, thr, device))
    dcf = []
    for (p, c_miss, c_fa), miss, fa in zip(points, st.miss, st.fa):
        p_miss, p_fa = int(miss) / float(st.n_tar), int(fa) / float(st.n_non)
        dcf.append((c_miss * p_miss * p + c_fa * p_fa * (1.0 - p)) / min(c_miss * p, c_fa * (1.0 - p)))
    return st.F / math.log(2.0), dcf


def cllr(llr, targets, device=0):
    """(mean_tar softplus(-llr) + mean_non softplus(llr)) / (2 ln 2): 0 for a perfect system, 1 for llr = 0 everywhere."""
    return evaluate(llr, targets, (), device)[0]


def act_dcf(llr, targets, p_target, c_miss=1.0, c_fa=1.0, device=0):
    """The normalised detection cost of scoring.min_dcf at the Bayes threshold eta = log(c_fa (1 - p) / (c_miss p)):
    P_miss = #{target: llr < eta} / N_tar, P_fa = #{non-target: llr >= eta} / N_non, exact counts, the comparison in double
    on the float32 llr.  It is one of the thresholds min_dcf tries, so act_dcf >= min_dcf on the same scores."""
    return evaluate(llr, targets, [(p_target, c_miss, c_fa)], device)[1][0]
