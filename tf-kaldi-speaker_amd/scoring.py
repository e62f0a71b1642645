"""Cosine scoring of x-vectors on the GPU (csrc/score.hip through the C ABI: xv_score_prepare / xv_score_matrix /
xv_score_pairs / xv_score_histogram): what the reference does with Kaldi binaries in its cosine back-end
(egs/voxceleb/v1/run.sh:362-365 plain cosine, :404-408 mean-subtract + transform-vec + length-norm +
ivector-compute-dot-products) and with a numpy double loop in its model-selection metric (compute_cos_pairwise_eer,
misc/utils.py:307-346).  PLDA scoring with a trained model is in plda.py, on the same kernels; PLDA / LDA training is in
backend.py.

Everything is fp32 with exact products: a score of two prepared rows of length d is within (d + 8) * 2^-24 of the exact
value.  Arrays go in and come out as numpy; a float32 torch tensor that already lives on the device is taken as it is,
and `as_tensor=True` keeps a result there.  No CPU path: without a HIP device every function here except
eer_from_histograms, exact_eer, min_dcf, read_trials and identification_rate raises RuntimeError.

Identification (top_k, identification_rate; plda.llr_top_k is the PLDA form) answers "which gallery rows score highest for
this query" through xv_score_topk, without the [n, m] score matrix.  The reference has no identification step: **parity
unpinned**; include/xvec_hip.h states the rule and tests/helpers/ref_topk.py restates it in numpy."""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr


def _need_device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device visible: scoring has no CPU fallback")
    return torch


def _rows(x, device, what):
    """[n, d] float32 on cuda:device, contiguous (numpy array or torch tensor)."""
    torch = _need_device()
    if isinstance(x, torch.Tensor):
        t = x.to(device="cuda:%d" % device, dtype=torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda:%d" % device)
    if t.dim() != 2:
        raise ValueError("%s: expected a [n, d] array, got shape %s" % (what, tuple(t.shape)))
    return t.contiguous()


def _shape2(x, what):
    shape = tuple(x.shape)
    if len(shape) != 2:
        raise ValueError("%s: expected a [n, d] array, got shape %s" % (what, shape))
    return shape


def check_transform(d_in, transform_shape):
    """The `transform-vec` rule: a transform for d_in-dimensional rows is [d_out, d_in] or [d_out, d_in + 1] (the last
    column is an offset: the input is extended by a constant 1).  -> (d_out, t_cols); ValueError otherwise."""
    if len(transform_shape) != 2 or transform_shape[0] < 1:
        raise ValueError("transform: expected a [d_out, d_in] or [d_out, d_in + 1] matrix, got shape %s" % (tuple(transform_shape),))
    d_out, t_cols = int(transform_shape[0]), int(transform_shape[1])
    if t_cols not in (d_in, d_in + 1):
        raise ValueError("transform: %d columns for rows of dimension %d (expected %d, or %d with an offset column)"
                         % (t_cols, d_in, d_in, d_in + 1))
    return d_out, t_cols


def prepare(x, mean=None, transform=None, normalize=True, eps=0.0, device=0, as_tensor=False):
    """Rows [n, d_in] -> [n, d_out], in this order, each step optional: subtract `mean` [d_in]
    (`ivector-subtract-global-mean`); apply `transform` [d_out, d_in] or [d_out, d_in + 1] (`transform-vec`); divide by
    sqrt(sum x^2 + eps) (`ivector-normalize-length`: eps 0, a zero row stays zero; misc/utils.py:317: eps 1e-12)."""
    n, d_in = _shape2(x, "x")
    if d_in < 1:
        raise ValueError("x: rows of dimension 0")
    d_out, t_cols = d_in, 0
    if transform is not None:
        d_out, t_cols = check_transform(d_in, tuple(transform.shape))
    if mean is not None and tuple(mean.shape) != (d_in,):
        raise ValueError("mean: shape %s for rows of dimension %d" % (tuple(mean.shape), d_in))
    if not eps >= 0.0:
        raise ValueError("eps must be >= 0")
    torch = _need_device()
    lib = _lib.load()
    with torch.cuda.device(device):
        xd = _rows(x, device, "x")
        md = None if mean is None else _rows(np.asarray(mean).reshape(1, -1) if not isinstance(mean, torch.Tensor)
                                             else mean.reshape(1, -1), device, "mean")
        td = None if transform is None else _rows(transform, device, "transform")
        out = torch.empty((n, d_out), dtype=torch.float32, device=xd.device)
        if n:
            stream = _lib.stream(device)
            _lib.check(lib.xv_score_prepare(device, ptr(xd), d_in, n, d_in, ptr(md),
                                            ptr(td), t_cols, d_out, t_cols, int(bool(normalize)),
                                            float(eps), ptr(out), d_out, stream))
        return out if as_tensor else out.cpu().numpy()


def cosine_matrix(a, b, device=0, as_tensor=False):
    """Prepared rows a [n, d], b [m, d] -> [n, m] float32 scores a[i] . b[j] (1 <= d <= 2048)."""
    (n, d), (m, db) = _shape2(a, "a"), _shape2(b, "b")
    if d != db:
        raise ValueError("a and b have different dimensions: %d, %d" % (d, db))
    torch = _need_device()
    lib = _lib.load()
    with torch.cuda.device(device):
        ad, bd = _rows(a, device, "a"), _rows(b, device, "b")
        out = torch.empty((n, m), dtype=torch.float32, device=ad.device)
        stream = _lib.stream(device)
        _lib.check(lib.xv_score_matrix(device, ptr(ad), d, n, ptr(bd), d, m, d, ptr(out), max(m, 1), stream))
        return out if as_tensor else out.cpu().numpy()


def cosine_pairs(a, b, ia, ib, device=0, as_tensor=False):
    """Trial scores a[ia[k]] . b[ib[k]] of prepared rows (`ivector-compute-dot-products`) -> [npairs] float32.
    An index out of range raises XvError(XV_ERR_INVALID) here, on the host; repeated calls are bit-identical."""
    (n, d), (m, db) = _shape2(a, "a"), _shape2(b, "b")
    if d != db:
        raise ValueError("a and b have different dimensions: %d, %d" % (d, db))
    ia = np.ascontiguousarray(ia, dtype=np.int64).reshape(-1)
    ib = np.ascontiguousarray(ib, dtype=np.int64).reshape(-1)
    if ia.shape != ib.shape:
        raise ValueError("ia and ib have different lengths")
    if ia.size and (ia.min() < 0 or ia.max() >= n or ib.min() < 0 or ib.max() >= m):
        raise _lib.XvError(_lib.XV_ERR_INVALID, "cosine_pairs: a trial index is out of range")
    torch = _need_device()
    lib = _lib.load()
    with torch.cuda.device(device):
        ad, bd = _rows(a, device, "a"), _rows(b, device, "b")
        iad = torch.from_numpy(ia.astype(np.int32)).to(ad.device)
        ibd = torch.from_numpy(ib.astype(np.int32)).to(ad.device)
        out = torch.empty((ia.size,), dtype=torch.float32, device=ad.device)
        stream = _lib.stream(device)
        _lib.check(lib.xv_score_pairs(device, ptr(ad), d, n, ptr(bd), d, m, d, ptr(iad), ptr(ibd), ia.size, ptr(out),
                                      stream))
        return out if as_tensor else out.cpu().numpy()


TopK = collections.namedtuple("TopK", ["scores", "indices", "count"])

TOPK_WORKSPACE_BYTES = 256 << 20        # what top_k lets its workspace grow to on its own: whole 128-row panels up to this,
TOPK_WORKSPACE_PANELS = 4               # or this many panels when they are larger (a long gallery: 512 rows per launch)
_topk_ws = {}                           # device -> uint8 tensor, kept between calls and grown on demand


def _workspace_min_bytes(entry, n, m, top_k):
    """The panel entry points' workspace query (`entry`: xv_cohort_stats_workspace or xv_score_topk_workspace)."""
    need = int(getattr(_lib.load(), entry)(int(n), int(m), int(top_k)))
    if need < 0:
        raise _lib.XvError(need, "%s: bad dimensions" % entry)
    return need


def topk_workspace_min_bytes(n, m, top_k=1):
    """The least workspace for n rows against a gallery of m: one 128-row panel of m scores."""
    return _workspace_min_bytes("xv_score_topk_workspace", n, m, top_k)


def _label_ids(labels_a, labels_b, n, m, name_a="labels_a", name_b="labels_b"):
    """Exclusion labels of both sides (anything np.unique sorts) -> two int32 id arrays, or None, None."""
    if (labels_a is None) != (labels_b is None):
        raise ValueError("%s and %s are given together or not at all" % (name_a, name_b))
    if labels_a is None:
        return None, None
    la, lb = np.asarray(labels_a).reshape(-1), np.asarray(labels_b).reshape(-1)
    if la.shape[0] != n or lb.shape[0] != m:
        raise ValueError("%s: %d for %d rows, %s: %d for %d rows" % (name_a, la.shape[0], n, name_b, lb.shape[0], m))
    ids = np.unique(np.concatenate([la, lb]), return_inverse=True)[1].astype(np.int32)
    return np.ascontiguousarray(ids[:n]), np.ascontiguousarray(ids[n:])


def _panel_args(torch, device, dev, row_bias, ids_a, col_bias, ids_b):
    """What xv_cohort_stats and xv_score_topk take beside their operands: the id arrays uploaded to `dev` -> (row_bias,
    labels_a, col_bias, labels_b), each a pointer or None, the current stream, and the uploads (to keep until the call)."""
    held = [None if ids is None else torch.from_numpy(ids).to(dev) for ids in (ids_a, ids_b)]
    rb, la, cb, lb = (ptr(t) for t in (row_bias, held[0], col_bias, held[1]))
    return rb, la, cb, lb, _lib.stream(device), held


def _top_k(ad, lda, n, row_bias, bd, ldb, m, col_bias, d, k, ids_a, ids_b, device, as_tensor):
    """xv_score_topk on operands that already live on cuda:device -> TopK."""
    k = int(k)
    if not 1 <= k <= 1024:
        raise ValueError("k must be in 1..1024, got %d" % k)
    torch = _need_device()
    lib = _lib.load()
    with torch.cuda.device(device):
        dev = ad.device
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        indices = torch.empty((n, k), dtype=torch.int32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        if n:
            need = topk_workspace_min_bytes(n, m, k)
            want = min((n + 127) // 128 * need, max(TOPK_WORKSPACE_PANELS * need, TOPK_WORKSPACE_BYTES // need * need))
            ws = _topk_ws.get(device)
            if ws is None or ws.numel() < want:
                _topk_ws[device] = ws = torch.empty((want,), dtype=torch.uint8, device=dev)
            rb, la, cb, lb, stream, held = _panel_args(torch, device, dev, row_bias, ids_a, col_bias, ids_b)
            _lib.check(lib.xv_score_topk(device, ptr(ad), lda, n, rb, la, ptr(bd), ldb, m, cb, lb, d, k,
                                         ptr(scores), ptr(indices), k, ptr(count), ptr(ws), ws.numel(), stream))
        if as_tensor:
            return TopK(scores, indices, count)
        return TopK(scores.cpu().numpy(), indices.cpu().numpy(), count.cpu().numpy())


def top_k(a, b, k, labels_a=None, labels_b=None, device=0, as_tensor=False):
    """Prepared rows a [n, d] (queries) against prepared rows b [m, d] (the gallery) -> TopK(scores [n, k] float32,
    indices [n, k] int32, count [n] int32): for every row of a the k rows of b with the largest cosine, by score descending
    and by row number ascending among equal scores; count is min(k, eligible rows) and the positions past it hold -inf / -1.
    `labels_a` [n] / `labels_b` [m] (anything np.unique sorts) make the rows of b that carry a query's label ineligible for
    it: labels_a = labels_b = arange searches a set against itself without a row finding itself.  1 <= k <= 1024; k may
    exceed m.  The scores are the bits cosine_matrix(a, b) holds; the [n, m] matrix is never written: the scores pass through
    a workspace of whole 128-row panels that is kept between calls and grows on demand (up to TOPK_WORKSPACE_BYTES, or
    TOPK_WORKSPACE_PANELS panels if that is more: a row is selected by one workgroup, so a long gallery wants several hundred
    rows per launch); its size does not change the result."""
    (n, d), (m, db) = _shape2(a, "a"), _shape2(b, "b")
    if d != db:
        raise ValueError("a and b have different dimensions: %d, %d" % (d, db))
    ids_a, ids_b = _label_ids(labels_a, labels_b, n, m)
    torch = _need_device()
    with torch.cuda.device(device):
        ad, bd = _rows(a, device, "a"), _rows(b, device, "b")
        return _top_k(ad, d, n, None, bd, d, m, None, d, k, ids_a, ids_b, device, as_tensor)


def identification_rate(indices, query_labels, gallery_labels, ranks=(1, 5, 10)):
    """Closed-set identification rates from the indices of top_k (host numpy) -> (rates, absent): rates[r] is the fraction of
    all queries whose own label is carried by one of their first r hits, for every r of `ranks` (r beyond the width of
    `indices` raises ValueError); padding (-1) never matches.  A query whose label no gallery row carries counts as a miss,
    and `absent` is the number of such queries.  No queries: every rate is 0.0."""
    idx = np.asarray(indices)
    if idx.ndim != 2:
        raise ValueError("indices: expected a [n, k] array, got shape %s" % (tuple(idx.shape),))
    ql, gl = np.asarray(query_labels).reshape(-1), np.asarray(gallery_labels).reshape(-1)
    n, width = idx.shape
    if ql.shape[0] != n:
        raise ValueError("query_labels: %d labels for %d queries" % (ql.shape[0], n))
    if idx.size and (idx.min() < -1 or idx.max() >= gl.shape[0]):
        raise ValueError("indices: an entry is outside the gallery of %d rows" % gl.shape[0])
    ranks = [int(r) for r in ranks]
    if any(r < 1 or r > width for r in ranks):
        raise ValueError("ranks %r for hits %d wide" % (tuple(ranks), width))
    valid = idx >= 0
    hit = np.zeros((n, width), dtype=bool)
    if gl.size:
        hit = valid & (gl[np.where(valid, idx, 0)] == ql[:, None])
    first = np.where(hit.any(axis=1), hit.argmax(axis=1), width)        # position of the first correct hit, or `width`
    rates = collections.OrderedDict((r, float(np.count_nonzero(first < r)) / n if n else 0.0) for r in ranks)
    absent = int(np.count_nonzero(~np.isin(ql, gl)))
    return rates, absent


def _check_nbins(nbins):
    nbins = int(nbins)
    if nbins < 256 or nbins > 65536 or nbins & (nbins - 1):
        raise ValueError("nbins must be a power of two in 256..65536, got %d" % nbins)
    return nbins


def score_histograms(a, labels_a, b=None, labels_b=None, nbins=65536, device=0):
    """Histograms of the scores of prepared rows, never materialising the score matrix -> (h_same, h_diff), two uint64
    arrays [nbins]; bin = clamp(floor((s + 1) * nbins / 2), 0, nbins - 1).  With b None: all pairs i < j of a (labels
    compared within a); otherwise all pairs (i, j) of a x b.  Labels are any array np.unique can sort."""
    nbins = _check_nbins(nbins)
    n, d = _shape2(a, "a")
    self_mode = b is None
    if self_mode and labels_b is not None:
        raise ValueError("labels_b without b")
    la = np.asarray(labels_a).reshape(-1)
    if la.shape[0] != n:
        raise ValueError("labels_a: %d labels for %d rows" % (la.shape[0], n))
    if self_mode:
        m = n
        ids = np.unique(la, return_inverse=True)[1].astype(np.int32)
        ida = idb = ids
    else:
        m, db = _shape2(b, "b")
        if d != db:
            raise ValueError("a and b have different dimensions: %d, %d" % (d, db))
        lb = np.asarray(labels_b).reshape(-1)
        if lb.shape[0] != m:
            raise ValueError("labels_b: %d labels for %d rows" % (lb.shape[0], m))
        ids = np.unique(np.concatenate([la, lb]), return_inverse=True)[1].astype(np.int32)
        ida, idb = ids[:n], ids[n:]
    torch = _need_device()
    lib = _lib.load()
    with torch.cuda.device(device):
        ad = _rows(a, device, "a")
        lad = torch.from_numpy(np.ascontiguousarray(ida)).to(ad.device)
        bd, lbd = (ad, lad) if self_mode else (_rows(b, device, "b"), torch.from_numpy(np.ascontiguousarray(idb)).to(ad.device))
        hist = torch.zeros((2, nbins), dtype=torch.int64, device=ad.device)      # uint64 counts (torch has no uint64 arithmetic)
        stream = _lib.stream(device)
        _lib.check(lib.xv_score_histogram(device, ptr(ad), d, n, ptr(lad), ptr(bd), d, m, ptr(lbd), d, int(self_mode), nbins,
                                          ptr(hist), C.c_void_p(hist.data_ptr() + 8 * nbins),
                                          stream))
        h = hist.cpu().numpy().view(np.uint64)
    return h[0].copy(), h[1].copy()


def eer_from_histograms(h_same, h_diff, lo=-1.0, hi=1.0):
    """Equal error rate of two score histograms over [lo, hi), by default the cosine range [-1, 1] (bin k = [e_k, e_k+1),
    e_k = lo + (hi - lo) k / nbins; the end bins of plda.llr_histograms also hold what falls outside) -> (eer, threshold).

    At a bin edge k (0..nbins) the false-reject rate is FRR(k) = sum(h_same[:k]) / sum(h_same) (same-label mass below the
    edge) and the false-accept rate is FAR(k) = sum(h_diff[k:]) / sum(h_diff) (different-label mass at or above it).
    FRR - FAR runs from -1 at k = 0 to +1 at k = nbins without decreasing; the crossing bin is the first k with
    FRR(k+1) >= FAR(k+1).  Inside it both rates are taken as linear; with g = FRR - FAR and t = -g(k) / (g(k+1) - g(k))
    the result is eer = FRR(k) + t (FRR(k+1) - FRR(k)) (= the interpolated FAR) at threshold e_k + t (e_k+1 - e_k).
    Pure numpy in float64 over exact integer counts: deterministic."""
    hs = np.asarray(h_same).astype(np.uint64).reshape(-1)
    hd = np.asarray(h_diff).astype(np.uint64).reshape(-1)
    if hs.shape != hd.shape or hs.size < 1:
        raise ValueError("histograms of different or zero length")
    nbins = hs.size
    cs = np.concatenate([[0], np.cumsum(hs, dtype=np.uint64)])
    cd = np.concatenate([[0], np.cumsum(hd, dtype=np.uint64)])
    ns, nd = int(cs[-1]), int(cd[-1])
    if ns == 0 or nd == 0:
        raise ValueError("EER needs at least one same-label and one different-label score (%d, %d)" % (ns, nd))
    frr = cs.astype(np.float64) / ns
    far = (nd - cd.astype(np.float64)) / nd
    g = frr - far
    k = int(np.argmax(g[1:] >= 0.0))
    t = -g[k] / (g[k + 1] - g[k])
    lo, hi = float(lo), float(hi)
    if not lo < hi:
        raise ValueError("empty score range [%r, %r)" % (lo, hi))
    w = (hi - lo) / nbins
    return float(frr[k] + t * (frr[k + 1] - frr[k])), float(lo + w * (k + t))


def select_rows(n, max_num_embeddings):
    """Row numbers compute_cos_pairwise_eer keeps (misc/utils.py:319-323): all of them, or every (n // max)-th."""
    if max_num_embeddings is None or n <= max_num_embeddings:
        return np.arange(n)
    if max_num_embeddings < 1:
        raise ValueError("max_num_embeddings must be positive")
    return np.arange(0, n, n // max_num_embeddings)


def pairwise_eer(embeddings, labels, max_num_embeddings=None, nbins=65536, device=0):
    """compute_cos_pairwise_eer (misc/utils.py:307-346) on the GPU -> (eer, threshold).

    Rows are divided by sqrt(sum x^2 + 1e-12) and every pair i < j is scored; the scores are counted in two histograms of
    `nbins` bins (score_histograms) and the EER is read from them (eer_from_histograms), so it is exact up to the bin width
    2 / nbins instead of up to the reference's interp1d / brentq.  There is no need to down-sample; with
    `max_num_embeddings` set and exceeded the reference's selection range(0, n, n // max_num_embeddings) is applied.
    Unlike the reference this does not write a `test.txt` into the working directory and does not normalise the
    caller's `embeddings` in place."""
    nbins = _check_nbins(nbins)
    n, _ = _shape2(embeddings, "embeddings")
    labels = np.asarray(labels).reshape(-1)
    if labels.shape[0] != n:
        raise ValueError("labels: %d labels for %d rows" % (labels.shape[0], n))
    keep = select_rows(n, max_num_embeddings)
    if len(keep) != n:
        embeddings, labels = embeddings[keep], labels[keep]
    x = prepare(embeddings, normalize=True, eps=1e-12, device=device, as_tensor=True)
    h_same, h_diff = score_histograms(x, labels, nbins=nbins, device=device)
    return eer_from_histograms(h_same, h_diff)


def read_trials(path):
    """Trial list: lines `key1 key2 [target|nontarget]` -> (keys1, keys2, targets); targets is a bool list, or None when
    no line has a third column.  Blank lines are skipped; anything else raises ValueError with the line number."""
    k1, k2, tg = [], [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if len(p) not in (2, 3) or (len(p) == 3 and p[2] not in ("target", "nontarget")):
                raise ValueError("%s:%d: expected `key1 key2 [target|nontarget]`, got %r" % (path, no, line.rstrip("\n")))
            if tg and (len(p) == 3) != (tg[-1] is not None):
                raise ValueError("%s:%d: trials with and without a label in one list" % (path, no))
            k1.append(p[0])
            k2.append(p[1])
            tg.append(p[2] == "target" if len(p) == 3 else None)
    if not tg or tg[0] is None:
        return k1, k2, None
    return k1, k2, tg


def exact_eer(scores, targets):
    """EER of a finite trial list, exactly, from the sorted scores (host, float64): with FRR(x) = #{target < x} / #target
    and FAR(x) = #{nontarget >= x} / #nontarget, the minimum over every threshold x (each distinct score, and one above
    the largest) of max(FRR(x), FAR(x)).  FRR - FAR does not decrease in x, so this is the value at the crossing."""
    s = np.asarray(scores, dtype=np.float64)
    t = np.asarray(targets, dtype=bool)
    nt, nn = int(t.sum()), int((~t).sum())
    if nt == 0 or nn == 0:
        raise ValueError("EER needs target and nontarget trials (%d, %d)" % (nt, nn))
    xs = np.unique(s)
    tgt, non = np.sort(s[t]), np.sort(s[~t])
    frr = np.concatenate([np.searchsorted(tgt, xs, side="left"), [nt]]) / float(nt)
    far = np.concatenate([nn - np.searchsorted(non, xs, side="left"), [0]]) / float(nn)
    return float(np.min(np.maximum(frr, far)))


def min_dcf(scores, targets, p_target=0.01, c_miss=1.0, c_fa=1.0):
    """Minimum normalised detection cost of a finite trial list (host, float64), the statement of Kaldi's
    sid/compute_min_dcf.py (egs/voxceleb/v1/run.sh:418-421: --p-target 0.01 and 0.001) -> (minDCF, threshold).

    With P_miss(x) = #{target < x} / #target and P_fa(x) = #{nontarget >= x} / #nontarget (the rates of exact_eer), the
    minimum over every threshold x (each distinct score, and one above the largest: reported as +inf) of
    c_miss P_miss(x) p_target + c_fa P_fa(x) (1 - p_target), divided by min(c_miss p_target, c_fa (1 - p_target)), the cost
    of the better of the two constant decisions.  Of equal minima the lowest threshold is returned."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    t = np.asarray(targets, dtype=bool).reshape(-1)
    if s.shape != t.shape:
        raise ValueError("scores and targets have different lengths")
    if not (0.0 < p_target < 1.0) or not c_miss > 0.0 or not c_fa > 0.0:
        raise ValueError("min_dcf needs 0 < p_target < 1 and positive costs, got %r, %r, %r" % (p_target, c_miss, c_fa))
    nt, nn = int(t.sum()), int((~t).sum())
    if nt == 0 or nn == 0:
        raise ValueError("minDCF needs target and nontarget trials (%d, %d)" % (nt, nn))
    xs = np.unique(s)
    tgt, non = np.sort(s[t]), np.sort(s[~t])
    p_miss = np.concatenate([np.searchsorted(tgt, xs, side="left"), [nt]]) / float(nt)
    p_fa = np.concatenate([nn - np.searchsorted(non, xs, side="left"), [0]]) / float(nn)
    cost = c_miss * p_miss * p_target + c_fa * p_fa * (1.0 - p_target)
    k = int(np.argmin(cost))
    return float(cost[k] / min(c_miss * p_target, c_fa * (1.0 - p_target))), float(xs[k]) if k < xs.size else float("inf")
