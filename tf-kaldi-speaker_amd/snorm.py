"""Score normalisation on the GPU: Z-norm, T-norm and S-norm with adaptive top-K cohorts (csrc/score.hip through the C ABI:
xv_cohort_stats).  The reference has no such step (egs/sre/v1/run.sh:13, "In the future, we will add score-normalization")
and neither have Kaldi's binaries: **parity unpinned**, checked against tests/helpers/ref_snorm.py.

Definitions (include/xvec_hip.h states the same):
  e is an enrolment row and t is a test row.  The cohort has rows c_1..c_m.
  score() is either the cosine of prepared rows or the PLDA log likelihood ratio.
  S_e = { score(e, c_j) }: for PLDA the cohort stands on the *test* side.
  S_t = { score(c_j, t) }: for PLDA the cohort stands on the *enrolment* side, num_utts 1.
  top_K(S) is the K largest values of S, with multiplicity.  mu(S) is their mean, sigma(S) their population standard
  deviation (divide by K), computed centred on mu.
  top_k = 0 means K = all eligible columns: plain Z-norm / T-norm.  Otherwise K_eff = min(top_k, eligible): adaptive S-norm
  in its "AS-norm1" form, each side picking its own top-K cohort.
  z: (s - mu(S_e)) / sigma(S_e).  t: (s - mu(S_t)) / sigma(S_t).  s: (z + t) / 2.
  Exclusion labels: a column whose label equals the row's label is not eligible.
  K_eff = 0 gives NaN, NaN; K_eff = 1 or equal selected values give std exactly 0.
  AS-norm2 (cohort chosen by the other side of the trial) is not offered.

No CPU path: cohort_stats and plda_cohort_stats raise RuntimeError without a HIP device; normalize is host arithmetic."""
import collections

import numpy as np

from . import _lib
from ._lib import ptr
from . import scoring

CohortStats = collections.namedtuple("CohortStats", ["mean", "std", "count"])

DEFAULT_WORKSPACE_BYTES = 64 << 20


def workspace_min_bytes(n, m, top_k=0):
    """The least `workspace_bytes` for n rows against a cohort of m: one 128-row panel of m scores."""
    return scoring._workspace_min_bytes("xv_cohort_stats_workspace", n, m, top_k)


def _label_ids(labels, cohort_labels, n, m):
    return scoring._label_ids(labels, cohort_labels, n, m, "labels", "cohort_labels")


def _stats(ad, lda, n, row_bias, bd, ldb, m, col_bias, k, top_k, ids_a, ids_b, workspace_bytes, device, as_tensor):
    """The call itself, on operands that already live on cuda:device."""
    top_k = int(top_k)
    if top_k < 0:
        raise ValueError("top_k must be >= 0, got %d" % top_k)
    top_k = min(top_k, m)                                # K_eff = min(top_k, eligible) anyway
    torch = scoring._need_device()
    lib = _lib.load()
    with torch.cuda.device(device):
        dev = ad.device
        mean = torch.empty((n,), dtype=torch.float32, device=dev)
        std = torch.empty((n,), dtype=torch.float32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        if n:
            need = workspace_min_bytes(n, m, top_k)
            if workspace_bytes is None:                  # whole panels up to the default, never more than the rows ask for
                per_row = need // 128
                workspace_bytes = max(need, min((n + 127) // 128 * 128 * per_row, DEFAULT_WORKSPACE_BYTES // need * need))
            workspace_bytes = int(workspace_bytes)
            ws = torch.empty((max(workspace_bytes, 1),), dtype=torch.uint8, device=dev)
            rb, la, cb, lb, stream, held = scoring._panel_args(torch, device, dev, row_bias, ids_a, col_bias, ids_b)
            _lib.check(lib.xv_cohort_stats(device, ptr(ad), lda, n, rb, la, ptr(bd), ldb, m, cb, lb, k, top_k,
                                           ptr(mean), ptr(std), ptr(count), ptr(ws), workspace_bytes, stream))
        if as_tensor:
            return CohortStats(mean, std, count)
        return CohortStats(mean.cpu().numpy(), std.cpu().numpy(), count.cpu().numpy())


def cohort_stats(x, cohort, top_k=0, labels=None, cohort_labels=None, device=0, workspace_bytes=None, as_tensor=False):
    """Prepared rows x [n, d] against prepared cohort rows [m, d] (scoring.prepare) -> CohortStats(mean, std, count), each
    [n]: mean and population std (float32) of the top_k largest cosines of every row of x against the cohort (top_k 0: all)
    and K_eff (int32).  `labels` [n] / `cohort_labels` [m] (anything np.unique sorts) exclude the columns that carry the
    row's label.  `workspace_bytes` None picks a size; any value from workspace_min_bytes(n, m) up gives the same bits."""
    (n, d), (m, db) = scoring._shape2(x, "x"), scoring._shape2(cohort, "cohort")
    if d != db:
        raise ValueError("x and cohort have different dimensions: %d, %d" % (d, db))
    ids_a, ids_b = _label_ids(labels, cohort_labels, n, m)
    torch = scoring._need_device()
    with torch.cuda.device(device):
        ad, bd = scoring._rows(x, device, "x"), scoring._rows(cohort, device, "cohort")
        return _stats(ad, d, n, None, bd, d, m, None, d, top_k, ids_a, ids_b, workspace_bytes, device, as_tensor)


def plda_cohort_stats(enroll, test, per, top_k=0, labels=None, cohort_labels=None, workspace_bytes=None, as_tensor=False):
    """PLDA form, on what plda.prepare_enroll / plda.prepare_test return.  per="enroll": statistics per enrolment row over the
    test-side rows (the cohort through prepare_test); per="test": per test row over the enrolment-side rows (the cohort
    through prepare_enroll, num_utts 1).  `labels` belong to the rows the statistics are for, `cohort_labels` to the other side.

    The score is llr_matrix(enroll, test)[i, j] = (a_i . b_j + rho_i) + tau_j.  per="enroll" takes exactly these bits;
    per="test" is the same call with the operands swapped and adds the two biases in the other order, (a . b + tau_j) + rho_i,
    which can differ from the matrix entry in the last place."""
    from . import plda
    if per not in ("enroll", "test"):
        raise ValueError('per must be "enroll" or "test", got %r' % (per,))
    k, tau = plda._operands(enroll, test, "plda_cohort_stats")
    n, m, dev = len(enroll), len(test), enroll.device
    if per == "enroll":
        ids_a, ids_b = _label_ids(labels, cohort_labels, n, m)
        return _stats(enroll.packed, enroll.packed.shape[1], n, enroll.bias, test.packed, test.packed.shape[1], m, tau, k, top_k,
                      ids_a, ids_b, workspace_bytes, dev, as_tensor)
    ids_a, ids_b = _label_ids(labels, cohort_labels, m, n)
    return _stats(test.packed, test.packed.shape[1], m, tau, enroll.packed, enroll.packed.shape[1], n, enroll.bias, k, top_k,
                  ids_a, ids_b, workspace_bytes, dev, as_tensor)


def _first_bad(std, used, side):
    std = np.asarray(std.detach().cpu().numpy() if hasattr(std, "detach") else std)
    rows = np.unique(np.asarray(used, dtype=np.int64))
    s = std[rows]
    bad = rows[~(np.isfinite(s) & (s != 0))]
    if bad.size:
        r = int(bad[0])
        raise ValueError("normalize: %s row %d is used by a trial and has a cohort std of %r (no eligible cohort row, or equal "
                         "cohort scores)" % (side, r, float(std[r])))


def normalize(scores, ia, ib, enroll_stats, test_stats, mode="s"):
    """Trial scores [npairs] of enrolment rows ia against test rows ib -> normalised scores, numpy in numpy out, torch in
    torch out: "z" (s - mean_e[ia]) / std_e[ia], "t" (s - mean_t[ib]) / std_t[ib], "s" their mean.  The side a mode does not
    use may be None.  ValueError names the first row used by a trial whose std is 0 or not finite; never a silent inf."""
    if mode not in ("z", "t", "s"):
        raise ValueError('mode must be "z", "t" or "s", got %r' % (mode,))
    ia = np.asarray(ia, dtype=np.int64).reshape(-1)
    ib = np.asarray(ib, dtype=np.int64).reshape(-1)
    is_torch = hasattr(scores, "detach")
    if tuple(scores.shape) != ia.shape or ia.shape != ib.shape:
        raise ValueError("scores, ia and ib have different lengths")

    def side(stats, idx, name):
        if stats is None:
            raise ValueError('mode "%s" needs the %s statistics' % (mode, name))
        if idx.size and (idx.min() < 0 or idx.max() >= stats.mean.shape[0]):
            raise ValueError("normalize: a trial index is outside the %s statistics" % name)
        _first_bad(stats.std, idx, name)
        if is_torch:
            import torch
            sel = torch.from_numpy(idx).to(scores.device)
            mu, sd = torch.as_tensor(stats.mean).to(scores.device)[sel], torch.as_tensor(stats.std).to(scores.device)[sel]
        else:
            mu, sd = np.asarray(_host(stats.mean))[idx], np.asarray(_host(stats.std))[idx]
        return (scores - mu) / sd

    if mode == "z":
        return side(enroll_stats, ia, "enrolment")
    if mode == "t":
        return side(test_stats, ib, "test")
    return (side(enroll_stats, ia, "enrolment") + side(test_stats, ib, "test")) * 0.5


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x
