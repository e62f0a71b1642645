"""PLDA scoring with a trained Kaldi `Plda` on the GPU (csrc/score.hip through the C ABI: xv_plda_prepare / xv_plda_matrix /
xv_plda_pairs / xv_plda_histogram): the last line of every recipe of the reference, `ivector-plda-scoring
--normalize-length=true [--num-utts=ark:num_utts.ark] "ivector-copy-plda --smoothing=0.0 plda - |" enroll test trials scores`
(egs/voxceleb/v1/run.sh:410-426, egs/voxceleb/v2|v3/run.sh:188-190, egs/sre/v1/run.sh:415-491, egs/fisher/v1/eval_plda.sh).
Training (`ivector-compute-lda`, `ivector-compute-plda`) is in backend.py; `ivector-adapt-plda` stays with Kaldi.  Kaldi is absent from the
reference tree: model file, TransformIvector and LogLikelihoodRatio restate plda.cc as published (**parity unpinned**),
checked against tests/helpers/ref_plda.py.

A `Plda` holds mean [D], transform [D, D] and psi [D] (float64): after u = transform (x - mean) the within-class covariance
is I and the between-class covariance is diag(psi).

  TransformIvector(x, n)   u = transform (x - mean); with normalize_length  u <- u sqrt(D / sum_d u_d^2 / (psi_d + 1 / n)),
                           with simple_length_norm  u <- u sqrt(D) / ||u||.  n = num_utts on the enrolment side, 1 on the test side.
  LogLikelihoodRatio(e, n, t)   with c = n psi / (n psi + 1) and v = 1 + psi / (n psi + 1):
                           s = -1/2 [sum log v + sum (t - c e)^2 / v] + 1/2 [sum log(1 + psi) + sum t^2 / (1 + psi)]

Expanded, s(i, j) = sum_d A_id t_jd + sum_d W_id t_jd^2 + rho_i with A = e c / v, W = (1 / (1 + psi) - 1 / v) / 2 and
rho = sum_d [log(1 + psi) - log v] / 2 - sum_d e^2 c^2 / v / 2.  When every enrolment row has the same n, W does not depend on
the row and the middle term is a per-column constant tau_j = sum_d W_d t_jd^2: the score matrix is a rank-D product with a row
and a column term added in the epilogue.  With mixed n the product is [A | W] . [t | t^2] (K = 2 D).  The per-n vectors are
built here in float64, one table per distinct n, and stay float64 on the device; products are exact fp32 with fp32
accumulation, rho and tau are accumulated in double and rounded once.

Model files are read and written on the host (numpy); everything else needs a HIP device (no CPU path, as scoring.py)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr
from . import kaldi_io
from . import scoring


class Plda(object):
    """mean [D], transform [D, D], psi [D], float64.  Shape errors raise kaldi_io.BadInputFormat."""

    def __init__(self, mean, transform, psi):
        self.mean = np.ascontiguousarray(mean, dtype=np.float64)
        self.transform = np.ascontiguousarray(transform, dtype=np.float64)
        self.psi = np.ascontiguousarray(psi, dtype=np.float64)
        m, t, p = self.mean.shape, self.transform.shape, self.psi.shape
        if len(m) != 1 or len(p) != 1 or len(t) != 2:
            raise kaldi_io.BadInputFormat("Plda: mean, transform, psi of shapes %s, %s, %s" % (m, t, p))
        if t[0] != t[1]:
            raise kaldi_io.BadInputFormat("Plda: transform is not square: %d x %d" % t)
        if m[0] != t[1] or p[0] != t[0] or m[0] < 1:
            raise kaldi_io.BadInputFormat("Plda: mean of dimension %d, transform %d x %d, psi of dimension %d" % (m[0], t[0], t[1], p[0]))
        if not np.all(self.psi >= 0.0):                 # also refuses NaN
            bad = int(np.argmax(~(self.psi >= 0.0)))
            raise kaldi_io.BadInputFormat("Plda: psi[%d] = %r of %d is negative" % (bad, float(self.psi[bad]), p[0]))
        self._device = {}

    @property
    def dim(self):
        return self.psi.shape[0]


class AdaptedPlda(object):
    """A Plda adapted to one recording (adapt_groups): `pca` [r, D] (the kept principal directions as rows), `affine`
    [r, D + 1] (u = affine [x; 1] has within-class covariance I and between-class covariance diag(psi)), `psi` [r],
    `eigenvalues` [D] (all of the recording's PCA spectrum, descending), float64; `dim` = r, `in_dim` = D.  prepare_enroll /
    prepare_test take it in place of a Plda, with rows of length in_dim."""

    def __init__(self, pca, affine, psi, eigenvalues):
        self.pca = None if pca is None else np.ascontiguousarray(pca, dtype=np.float64)
        self.affine = np.ascontiguousarray(affine, dtype=np.float64)
        self.psi = np.ascontiguousarray(psi, dtype=np.float64)
        self.eigenvalues = None if eigenvalues is None else np.ascontiguousarray(eigenvalues, dtype=np.float64)
        if self.affine.ndim != 2 or self.psi.shape != (self.affine.shape[0],) or self.affine.shape[0] < 1 or self.affine.shape[1] < 2:
            raise ValueError("AdaptedPlda: affine of shape %s, psi of shape %s" % (self.affine.shape, self.psi.shape))
        if self.pca is not None and self.pca.shape != (self.affine.shape[0], self.affine.shape[1] - 1):
            raise ValueError("AdaptedPlda: pca of shape %s for an affine of shape %s" % (self.pca.shape, self.affine.shape))
        self._device = {}

    @property
    def dim(self):
        return self.psi.shape[0]

    @property
    def in_dim(self):
        return self.affine.shape[1] - 1


# ----------------------------------------------------------------------------- model file
def _text_tokens(data):
    """Whitespace-separated tokens of a text-mode object; a line end is the token '\\n' (it separates matrix rows)."""
    out = []
    for line in data.decode("latin1").split("\n"):
        out += line.split()
        out.append("\n")
    return out


def _text_numbers(tok, pos, what):
    """`[ ... ]` from tok[pos] -> (rows: list of lists of float, next position)."""
    while pos < len(tok) and tok[pos] == "\n":
        pos += 1
    if pos >= len(tok) or tok[pos] != "[":
        raise kaldi_io.BadInputFormat("Plda: expected '[' at the start of %s, got %r" % (what, tok[pos] if pos < len(tok) else "end of file"))
    pos += 1
    rows, cur = [], []
    while True:
        if pos >= len(tok):
            raise kaldi_io.BadInputFormat("Plda: end of file inside %s (%d rows read)" % (what, len(rows)))
        t = tok[pos]
        pos += 1
        if t == "\n" or t == "]":
            if cur:
                rows.append(cur)
                cur = []
            if t == "]":
                return rows, pos
            continue
        try:
            cur.append(float(t))
        except ValueError:
            raise kaldi_io.BadInputFormat("Plda: %r inside %s" % (t, what))


def read_plda(path_or_pipe):
    """A Kaldi `Plda` file (what ivector-compute-plda / ivector-copy-plda write), binary or text; `cmd |` reads a pipe.
    Binary: '\\0B' '<Plda> ' mean ('DV ' vector) transform ('DM ' matrix) psi ('DV ') '</Plda> '; float payloads ('FV ', 'FM ')
    are accepted too.  Text: `<Plda>  [ mean ]`, ` [` rows `]`, ` [ psi ]`, `</Plda>`."""
    fd = kaldi_io.open_or_fd(path_or_pipe)
    try:
        s = kaldi_io._Stream(fd)
        flag = s.read(2)
        if flag == b"\0B":
            kaldi_io.expect_token(s, "<Plda>")
            mean = kaldi_io._read_vec_binary(s)
            transform = kaldi_io._read_mat_binary(s)
            psi = kaldi_io._read_vec_binary(s)
            end = s.read_token()
            if end != b"</Plda>":
                raise kaldi_io.BadInputFormat("Plda: end token </Plda> missing after psi of dimension %d (got %r)" % (psi.shape[0], end[:40]))
        else:
            data = flag
            while True:
                chunk = s.read(1 << 20)
                if not chunk:
                    break
                data += chunk
            tok = _text_tokens(data)
            pos = 0
            while pos < len(tok) and tok[pos] == "\n":
                pos += 1
            if pos >= len(tok) or tok[pos] != "<Plda>":
                raise kaldi_io.BadInputFormat("Plda: expected token <Plda>, got %r" % (tok[pos] if pos < len(tok) else "end of file"))
            rows, pos = _text_numbers(tok, pos + 1, "mean")
            mean = np.array([v for r in rows for v in r], dtype=np.float64)
            rows, pos = _text_numbers(tok, pos, "transform")
            if len(set(len(r) for r in rows)) > 1:
                raise kaldi_io.BadInputFormat("Plda: transform rows of lengths %s" % sorted(set(len(r) for r in rows)))
            transform = np.array(rows, dtype=np.float64).reshape(len(rows), len(rows[0]) if rows else 0)
            rows, pos = _text_numbers(tok, pos, "psi")
            psi = np.array([v for r in rows for v in r], dtype=np.float64)
            while pos < len(tok) and tok[pos] == "\n":
                pos += 1
            if pos >= len(tok) or tok[pos] != "</Plda>":
                raise kaldi_io.BadInputFormat("Plda: end token </Plda> missing after psi of dimension %d" % psi.shape[0])
    finally:
        if fd is not path_or_pipe:
            fd.close()
    return Plda(mean, transform, psi)


def write_plda(path, plda, binary=True):
    """The file read_plda reads, in Kaldi's layout (doubles; text mode prints 17 significant digits: exact)."""
    if binary:
        data = (b"\0B<Plda> " + kaldi_io.vec_payload(plda.mean) + kaldi_io.mat_payload(plda.transform)
                + kaldi_io.vec_payload(plda.psi) + b"</Plda> ")
    else:
        vec = lambda v: " [ " + " ".join(repr(float(a)) for a in v) + " ]\n"       # noqa: E731
        rows = ["  " + " ".join(repr(float(a)) for a in r) for r in plda.transform]
        data = ("<Plda> " + vec(plda.mean) + " [\n" + "\n".join(rows) + " ]\n" + vec(plda.psi) + "</Plda> ").encode("latin1")
    fd = kaldi_io.open_or_fd(path, mode="wb")
    try:
        fd.write(data)
    finally:
        if fd is not path:
            fd.close()


def smooth(plda, factor):
    """`ivector-copy-plda --smoothing=factor` (Plda::SmoothWithinClassCovariance): the within-class covariance I becomes
    w = 1 + factor psi per dimension and the model is re-whitened: psi <- psi / w, transform <- diag(w^-1/2) transform.
    Float64 on the host; factor 0 returns the same numbers."""
    factor = float(factor)
    if not 0.0 <= factor <= 1.0:
        raise ValueError("smoothing factor must be in [0, 1], got %r" % factor)
    w = 1.0 + factor * plda.psi
    return Plda(plda.mean.copy(), plda.transform / np.sqrt(w)[:, None], plda.psi / w)


# ----------------------------------------------------------------------------- per-n tables (host, float64)
def tables(psi, n):
    """The vectors of one n -> dict of float64 [D] arrays: inv = 1 / (psi + 1 / n) (TransformIvector), c, v, a = c / v,
    q = -c^2 / (2 v), w = (1 / (1 + psi) - 1 / v) / 2, and the scalar logdet = sum [log(1 + psi) - log v] / 2."""
    psi = np.asarray(psi, dtype=np.float64)
    n = float(n)
    c = n * psi / (n * psi + 1.0)
    v = 1.0 + psi / (n * psi + 1.0)
    return dict(inv=1.0 / (psi + 1.0 / n), c=c, v=v, a=c / v, q=-0.5 * c * c / v, w=0.5 * (1.0 / (1.0 + psi) - 1.0 / v),
                logdet=0.5 * float(np.sum(np.log1p(psi) - np.log(v))))


_NORM_NONE, _NORM_PLDA, _NORM_SIMPLE = 0, 1, 2


def _norm_mode(normalize_length, simple_length_norm):
    return _NORM_NONE if not normalize_length else (_NORM_SIMPLE if simple_length_norm else _NORM_PLDA)


def _affine(model, device, torch):
    """[transform | -transform mean] as float32 on the device (the offset in float64 first; the affine of an AdaptedPlda,
    rounded once), cached on the model."""
    key = ("affine", device)
    if key not in model._device:
        if isinstance(model, AdaptedPlda):
            t = model.affine.astype(np.float32)
        else:
            t = np.concatenate([model.transform, -(model.transform @ model.mean)[:, None]], axis=1).astype(np.float32)
        model._device[key] = torch.from_numpy(np.ascontiguousarray(t)).to("cuda:%d" % device)
    return model._device[key]


def _pad4(k):
    return (k + 3) // 4 * 4


class PldaRows(object):
    """Prepared rows of one side, on the device: `rows` [n, D] float32 (TransformIvector), `packed` [n, ld] (the scoring
    operand: A, or [A | W] for an enrolment set of mixed n; [t | t^2] on the test side), `bias` [n] (rho; on the test side
    tau(n) is made on demand, per n, and kept), `num_utts` (enrolment; numpy int64) and `uniform_n` (their common value,
    or None)."""

    def __init__(self, model, side, device, rows, packed, bias, num_utts):
        self.model, self.side, self.device = model, side, device
        self.rows, self.packed, self.bias = rows, packed, bias
        self.num_utts = num_utts
        self.uniform_n = None
        if side == "enroll":
            self.uniform_n = int(num_utts[0]) if num_utts.size and np.all(num_utts == num_utts[0]) else (1 if not num_utts.size else None)
        self._tau = {}

    def __len__(self):
        return int(self.rows.shape[0])

    @property
    def k(self):
        """Length of the product an enrolment set asks for: D, or 2 D with mixed n."""
        return self.model.dim if self.uniform_n is not None else 2 * self.model.dim

    def tau(self, n):
        """Test side: tau_j = sum_d W_d(n) t_jd^2 for an enrolment set of uniform n -> [m] float32 on the device."""
        if self.side != "test":
            raise ValueError("tau belongs to the test side")
        n = int(n)
        if n not in self._tau:
            torch = scoring._need_device()
            d = self.model.dim
            with torch.cuda.device(self.device):
                tab = np.zeros((1, 4, d))
                tab[0, 2] = tables(self.model.psi, n)["w"]
                tabd = torch.from_numpy(tab).to(self.rows.device)
                out = torch.empty((len(self),), dtype=torch.float32, device=self.rows.device)
                if len(self):
                    stream = _lib.stream(self.device)
                    _lib.check(_lib.load().xv_plda_prepare(self.device, ptr(self.rows), d, len(self), d, None, 0, d, _NORM_NONE, 1, 0,
                                                           ptr(tabd), None, 1, None, None, 0, None, 0, ptr(out),
                                                           stream))
            self._tau[n] = out
        return self._tau[n]


def _prepare(model, x, side, num_utts, normalize_length, simple_length_norm, device):
    n, d_in = scoring._shape2(x, "x")
    d = model.dim
    d_model = model.in_dim if isinstance(model, AdaptedPlda) else d
    if d_in != d_model:
        raise ValueError("x: rows of dimension %d for a Plda of dimension %d" % (d_in, d_model))
    if d > 2048:
        raise ValueError("Plda of dimension %d: at most 2048" % d)
    if side == "enroll":
        counts = np.ones(n, np.int64) if num_utts is None else np.ascontiguousarray(num_utts, dtype=np.int64).reshape(-1)
        if counts.shape[0] != n:
            raise ValueError("num_utts: %d counts for %d rows" % (counts.shape[0], n))
        if counts.size and counts.min() < 1:
            raise ValueError("num_utts: counts must be >= 1, got %d" % counts.min())
        distinct, index = np.unique(counts, return_inverse=True)
        if not distinct.size:
            distinct = np.array([1], np.int64)
        mixed = distinct.size > 1
        if mixed and 2 * d > 2048:
            raise ValueError("an enrolment set of mixed num_utts needs 2 D <= 2048, D = %d" % d)
        tab, logdet = np.zeros((distinct.size, 4, d)), np.zeros(distinct.size)
        for k, nu in enumerate(distinct):
            t = tables(model.psi, int(nu))
            tab[k, 0], tab[k, 1], tab[k, 2], tab[k, 3], logdet[k] = t["inv"], t["a"], t["q"], t["w"], t["logdet"]
        ldp = _pad4(2 * d if mixed else d)
    else:
        counts, index, mixed = None, None, True                  # the test side always carries [t | t^2]
        tab, logdet = np.zeros((1, 4, d)), None
        tab[0, 0], tab[0, 1] = tables(model.psi, 1)["inv"], 1.0
        ldp = _pad4(2 * d)
    torch = scoring._need_device()
    lib = _lib.load()
    with torch.cuda.device(device):
        xd = scoring._rows(x, device, "x")
        aff = _affine(model, device, torch)
        tabd = torch.from_numpy(tab).to(xd.device)
        logd = None if logdet is None else torch.from_numpy(logdet).to(xd.device)
        idx = None if index is None or not mixed else torch.from_numpy(index.astype(np.int32)).to(xd.device)
        rows = torch.empty((n, d), dtype=torch.float32, device=xd.device)
        packed = torch.zeros((n, ldp), dtype=torch.float32, device=xd.device)
        bias = torch.empty((n,), dtype=torch.float32, device=xd.device) if side == "enroll" else None
        if n:
            stream = _lib.stream(device)
            _lib.check(lib.xv_plda_prepare(device, ptr(xd), d_in, n, d_in, ptr(aff), d_in + 1, d,
                                           _norm_mode(normalize_length, simple_length_norm), 0 if side == "enroll" else 1,
                                           int(mixed), ptr(tabd), ptr(logd), tab.shape[0],
                                           ptr(idx), ptr(rows), d, ptr(packed), ldp,
                                           ptr(bias), stream))
    return PldaRows(model, side, device, rows, packed, bias, counts)


def prepare_enroll(model, x, num_utts=None, normalize_length=True, simple_length_norm=False, device=0):
    """Enrolment rows [n, D] (x-vectors or speaker means behind the `ivector-subtract-global-mean | transform-vec |
    ivector-normalize-length` front, e.g. scoring.prepare(..., as_tensor=True)) -> PldaRows: TransformIvector(x_i, num_utts_i)
    and the packed operands A (W) and rho.  `num_utts` [n] is what --num-utts reads (None: 1 everywhere); the two switches
    are Kaldi's --normalize-length / --simple-length-normalization with ivector-plda-scoring's use of them in the recipes."""
    return _prepare(model, x, "enroll", num_utts, normalize_length, simple_length_norm, device)


def prepare_test(model, x, normalize_length=True, simple_length_norm=False, device=0):
    """Test rows [m, D] -> PldaRows: TransformIvector(x_j, 1) and the packed operand [t | t^2]."""
    return _prepare(model, x, "test", None, normalize_length, simple_length_norm, device)


def _same_model(a, b):
    """Two models by their arrays: a Plda by psi, transform and mean, an AdaptedPlda by psi and affine."""
    if isinstance(a, AdaptedPlda) != isinstance(b, AdaptedPlda):
        return False
    if isinstance(a, AdaptedPlda):
        return np.array_equal(a.psi, b.psi) and np.array_equal(a.affine, b.affine)
    return np.array_equal(a.psi, b.psi) and np.array_equal(a.transform, b.transform) and np.array_equal(a.mean, b.mean)


def _operands(enroll, test, who):
    if not isinstance(enroll, PldaRows) or not isinstance(test, PldaRows) or enroll.side != "enroll" or test.side != "test":
        raise ValueError("%s: expected prepare_enroll(...) and prepare_test(...) results, in this order" % who)
    if enroll.model is not test.model and not _same_model(enroll.model, test.model):
        raise ValueError("%s: the two sides were prepared with different models" % who)
    if enroll.device != test.device:
        raise ValueError("%s: the two sides live on different devices (%d, %d)" % (who, enroll.device, test.device))
    tau = test.tau(enroll.uniform_n) if enroll.uniform_n is not None else None
    return enroll.k, tau


def llr_matrix(enroll, test, as_tensor=False):
    """Log likelihood ratios of every enrolment row against every test row -> [n, m] float32."""
    k, tau = _operands(enroll, test, "llr_matrix")
    torch = scoring._need_device()
    lib = _lib.load()
    n, m, dev = len(enroll), len(test), enroll.device
    with torch.cuda.device(dev):
        out = torch.empty((n, m), dtype=torch.float32, device=enroll.rows.device)
        stream = _lib.stream(dev)
        _lib.check(lib.xv_plda_matrix(dev, ptr(enroll.packed), enroll.packed.shape[1], n, ptr(enroll.bias),
                                      ptr(test.packed), test.packed.shape[1], m, ptr(tau), k,
                                      ptr(out), max(m, 1), stream))
        return out if as_tensor else out.cpu().numpy()


def llr_top_k(enroll, test, k, per="test", labels_enroll=None, labels_test=None, as_tensor=False):
    """Identification with PLDA, on what prepare_enroll / prepare_test return -> scoring.TopK(scores, indices, count).
    per="test": for every test row the k enrolment rows with the largest LLR (who is this?); per="enroll": for every
    enrolment row the k best test rows.  Order, ties, padding and the exclusion labels (`labels_enroll` [n] and `labels_test`
    [m], given together) are those of scoring.top_k; the [n, m] matrix is never written.

    The score is llr_matrix(enroll, test)[i, j] = (a_i . b_j + rho_i) + tau_j.  per="enroll" takes exactly these bits: it is
    xv_plda_matrix's operand order.  per="test" is the same call with the operands swapped and adds the two biases in the
    other order, (b_j . a_i + tau_j) + rho_i: the bits of xv_plda_matrix called with the test side first, which can differ
    from the entry of llr_matrix in the last place."""
    if per not in ("enroll", "test"):
        raise ValueError('per must be "enroll" or "test", got %r' % (per,))
    kk, tau = _operands(enroll, test, "llr_top_k")
    n, m, dev = len(enroll), len(test), enroll.device
    ids_e, ids_t = scoring._label_ids(labels_enroll, labels_test, n, m)
    if per == "enroll":
        return scoring._top_k(enroll.packed, enroll.packed.shape[1], n, enroll.bias, test.packed, test.packed.shape[1], m, tau,
                              kk, k, ids_e, ids_t, dev, as_tensor)
    return scoring._top_k(test.packed, test.packed.shape[1], m, tau, enroll.packed, enroll.packed.shape[1], n, enroll.bias, kk, k,
                          ids_t, ids_e, dev, as_tensor)


def llr_pairs(enroll, test, ia, ib, as_tensor=False):
    """`ivector-plda-scoring` over a trial list: LLR of enrolment row ia[k] against test row ib[k] -> [npairs] float32.
    An index out of range raises XvError(XV_ERR_INVALID) here, on the host; repeated calls are bit-identical."""
    k, tau = _operands(enroll, test, "llr_pairs")
    n, m, dev = len(enroll), len(test), enroll.device
    ia = np.ascontiguousarray(ia, dtype=np.int64).reshape(-1)
    ib = np.ascontiguousarray(ib, dtype=np.int64).reshape(-1)
    if ia.shape != ib.shape:
        raise ValueError("ia and ib have different lengths")
    if ia.size and (ia.min() < 0 or ia.max() >= n or ib.min() < 0 or ib.max() >= m):
        raise _lib.XvError(_lib.XV_ERR_INVALID, "llr_pairs: a trial index is out of range")
    torch = scoring._need_device()
    lib = _lib.load()
    with torch.cuda.device(dev):
        iad = torch.from_numpy(ia.astype(np.int32)).to(enroll.rows.device)
        ibd = torch.from_numpy(ib.astype(np.int32)).to(enroll.rows.device)
        out = torch.empty((ia.size,), dtype=torch.float32, device=enroll.rows.device)
        stream = _lib.stream(dev)
        _lib.check(lib.xv_plda_pairs(dev, ptr(enroll.packed), enroll.packed.shape[1], n, ptr(enroll.bias),
                                     ptr(test.packed), test.packed.shape[1], m, ptr(tau), k,
                                     ptr(iad), ptr(ibd), ia.size, ptr(out), stream))
        return out if as_tensor else out.cpu().numpy()


def llr_histograms(enroll, labels_e, test, labels_t, lo, hi, nbins=8192):
    """Histograms of the LLRs of every (enrolment, test) pair without the matrix -> (h_same, h_diff), uint64 [nbins];
    bin = clamp(floor((s - lo) nbins / (hi - lo)), 0, nbins - 1): the end bins also hold what falls outside [lo, hi).
    scoring.eer_from_histograms(h_same, h_diff, lo, hi) reads the EER from them."""
    nbins = scoring._check_nbins(nbins)
    lo, hi = float(lo), float(hi)
    if not (lo < hi) or not np.isfinite(hi - lo):
        raise ValueError("the range [lo, hi) is empty or not finite: %r, %r" % (lo, hi))
    k, tau = _operands(enroll, test, "llr_histograms")
    n, m, dev = len(enroll), len(test), enroll.device
    la, lb = np.asarray(labels_e).reshape(-1), np.asarray(labels_t).reshape(-1)
    if la.shape[0] != n or lb.shape[0] != m:
        raise ValueError("labels: %d, %d labels for %d, %d rows" % (la.shape[0], lb.shape[0], n, m))
    ids = np.unique(np.concatenate([la, lb]), return_inverse=True)[1].astype(np.int32)
    torch = scoring._need_device()
    lib = _lib.load()
    with torch.cuda.device(dev):
        lad = torch.from_numpy(np.ascontiguousarray(ids[:n])).to(enroll.rows.device)
        lbd = torch.from_numpy(np.ascontiguousarray(ids[n:])).to(enroll.rows.device)
        hist = torch.zeros((2, nbins), dtype=torch.int64, device=enroll.rows.device)
        stream = _lib.stream(dev)
        _lib.check(lib.xv_plda_histogram(dev, ptr(enroll.packed), enroll.packed.shape[1], n, ptr(enroll.bias),
                                         ptr(lad), ptr(test.packed), test.packed.shape[1], m,
                                         ptr(tau), ptr(lbd), k, lo, hi, nbins,
                                         ptr(hist), C.c_void_p(hist.data_ptr() + 8 * nbins), stream))
        h = hist.cpu().numpy().view(np.uint64)
    return h[0].copy(), h[1].copy()


# ----------------------------------------------------------------------------- per-recording adaptation (csrc/plda_adapt.hip)
ADAPT_MAX_DIM = 256
ADAPT_BUDGET_BYTES = 1 << 30            # what the outputs and the workspace of one xv_plda_adapt call may take together


def _check_target_energy(target_energy):
    te = float(target_energy)
    if not 0.0 < te <= 1.0:             # also refuses NaN
        raise ValueError("target_energy must be in (0, 1], got %r" % (target_energy,))
    return te


def _adapt_device(model, device, torch):
    """mean, transform^-1 (inverted once, float64, on the host) and psi as doubles on the device, cached on the model."""
    key = ("adapt", device)
    if key not in model._device:
        dev = "cuda:%d" % device
        model._device[key] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
                                   for a in (model.mean, np.linalg.inv(model.transform), model.psi))
    return model._device[key]


def _adapt_raw(model, xs, offsets, target_energy, device=0, want_pca=True, budget=None, ws_bytes=None):
    """xv_plda_adapt over the groups of `xs` (a [N, D] float32 device tensor whose rows are sorted by group; group g owns
    the rows offsets[g] .. offsets[g + 1]) -> (dim [G] int32, eigval [G, D], pca [G, D, D] or None, affine [G, D, D + 1],
    psi [G, D], sweeps [G, 2] int32), numpy.  The groups go in runs whose outputs fit `budget` bytes (a run holds at least one
    group), each with a workspace of one slot per group (xv_plda_adapt_slot_bytes) inside the same budget, or of exactly `ws_bytes`; by
    the rule the result does not depend on either.  One device-to-host copy per run and output."""
    te = _check_target_energy(target_energy)
    d = model.dim
    if not 1 <= d <= ADAPT_MAX_DIM:
        raise ValueError("a Plda of dimension %d cannot be adapted: at most %d" % (d, ADAPT_MAX_DIM))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    groups = offsets.shape[0] - 1
    if int(xs.shape[1]) != d:
        raise ValueError("x: rows of dimension %d for a Plda of dimension %d" % (int(xs.shape[1]), d))
    torch = scoring._need_device()
    lib = _lib.load()
    budget = ADAPT_BUDGET_BYTES if budget is None else int(budget)
    per_group = 8 * (d * d + d * (d + 1) + 2 * d) + 4
    slot = int(lib.xv_plda_adapt_slot_bytes(d))
    run = max(1, (budget // 2) // per_group)
    dims, eig, pcas, affs, psis, sweeps = [], [], [], [], [], []
    with torch.cuda.device(device):
        dev = torch.device("cuda:%d" % device)
        stream = _lib.stream(device)
        mean, ainv, psi = _adapt_device(model, device, torch)
        for g0 in range(0, groups, run):
            g1 = min(groups, g0 + run)
            cnt = g1 - g0
            off = np.ascontiguousarray(offsets[g0:g1 + 1])
            dim = torch.empty((cnt,), dtype=torch.int32, device=dev)
            eigval = torch.zeros((cnt, d), dtype=torch.float64, device=dev)
            pca = torch.zeros((cnt, d, d), dtype=torch.float64, device=dev)
            affine = torch.zeros((cnt, d, d + 1), dtype=torch.float64, device=dev)
            psi_out = torch.zeros((cnt, d), dtype=torch.float64, device=dev)
            least = int(lib.xv_plda_adapt_workspace(cnt, d))
            if least < 0:
                raise _lib.XvError(least, "xv_plda_adapt_workspace: bad arguments")
            if ws_bytes is None:
                slots = max(1, min(cnt, (budget // 2) // slot))
                size = least + (slots - 1) * slot
            else:
                size = int(ws_bytes)
            ws = torch.empty((max(size, 8),), dtype=torch.uint8, device=dev)
            _lib.check(lib.xv_plda_adapt(device, ptr(xs), d, off.ctypes.data_as(C.c_void_p), cnt, d, ptr(mean),
                                         ptr(ainv), ptr(psi), te, ptr(dim), ptr(eigval), ptr(pca),
                                         ptr(affine), ptr(psi_out), ptr(ws), size, stream))
            dims.append(dim.cpu().numpy())
            eig.append(eigval.cpu().numpy())
            if want_pca:
                pcas.append(pca.cpu().numpy())
            affs.append(affine.cpu().numpy())
            psis.append(psi_out.cpu().numpy())
            sweeps.append(ws[8 * (cnt + 1):16 * cnt + 8].cpu().numpy().view(np.int32).reshape(cnt, 2).copy())
    if not groups:
        return (np.zeros(0, np.int32), np.zeros((0, d)), np.zeros((0, d, d)) if want_pca else None, np.zeros((0, d, d + 1)),
                np.zeros((0, d)), np.zeros((0, 2), np.int32))
    return (np.concatenate(dims), np.concatenate(eig), np.concatenate(pcas) if want_pca else None, np.concatenate(affs),
            np.concatenate(psis), np.concatenate(sweeps))


def _warn_fallback(dims, who):
    bad = int(np.sum(np.asarray(dims) == 0))
    if bad:
        import warnings
        warnings.warn("%s: %d of %d groups could not be adapted (fewer than 2 rows, no variance, or an iteration that did not "
                      "converge) and are scored with the global model" % (who, bad, len(dims)), RuntimeWarning, stacklevel=3)


def adapt_groups(model, x, groups, target_energy, device=0):
    """Kaldi's `ivector-plda-scoring-dense --target-energy` adaptation for every group (recording) of the rows x [N, D]
    (the rows behind the mean / transform / normalize front, numpy or a device tensor): the PCA of the group's own rows keeps
    the leading directions that hold `target_energy` of the variance plus one, the global model is projected there and
    diagonalised again (include/xvec_hip.h, xv_plda_adapt, states the rule).  -> OrderedDict group -> AdaptedPlda in sorted
    group order, None for a group that falls back to the global model (fewer than 2 rows, no variance, a projected
    within-class covariance that is not positive definite, an iteration that did not converge); one warning per call counts
    them.  `groups` [N] holds one id per row (anything np.unique sorts)."""
    import collections
    n, _ = scoring._shape2(x, "x")
    ids = np.asarray(groups).reshape(-1)
    if ids.shape[0] != n:
        raise ValueError("groups: %d ids for %d rows" % (ids.shape[0], n))
    _check_target_energy(target_energy)
    names, inverse = np.unique(ids, return_inverse=True)
    order = np.argsort(inverse, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(names)))]).astype(np.int64)
    torch = scoring._need_device()
    with torch.cuda.device(device):
        xd = scoring._rows(x, device, "x")
        xs = xd[torch.from_numpy(order).to(xd.device)].contiguous()
    dim, eigval, pca, affine, psi, _ = _adapt_raw(model, xs, offsets, target_energy, device)
    _warn_fallback(dim, "adapt_groups")
    out = collections.OrderedDict()
    for g, name in enumerate(names):
        r = int(dim[g])
        key = name.item() if hasattr(name, "item") else name
        out[key] = AdaptedPlda(pca[g, :r], affine[g, :r], psi[g, :r], eigval[g]) if r else None
    return out
