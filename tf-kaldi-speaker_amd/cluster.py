"""Speaker clustering on the GPU: average-linkage agglomerative clustering of the sub-segment x-vectors of every recording
(xv_ahc, csrc/cluster.hip), the step Kaldi's diarization/cluster.sh runs with agglomerative-cluster over a dense cosine or PLDA
score matrix per recording.  The reference has no clustering step: **parity unpinned**; include/xvec_hip.h states the rule and
tests/helpers/ref_cluster.py restates it in numpy.

    python -m tf_kaldi_speaker_amd.cluster [--gpu 0] [--threshold T | --reco2num-spk FILE] [--mean mean.vec]
           [--transform transform.mat] [--normalize true] [--plda plda [--smoothing 0.0] [--normalize-length true]
           [--simple-length-normalization false] [--target-energy E]] [--segments FILE --rttm-out FILE]
           <utt2reco> <xvector-rspecifier> <labels-out>

<utt2reco> holds lines `key recording`; every key of the x-vector table needs one (a key without a recording is an error).
The table goes through the front of score_cos (--mean, --transform, --normalize).  Without --plda the score of two rows is their
cosine; with --plda it is the log likelihood ratio of ivector-plda-scoring with both sides counted as one utterance (the
model options are score_plda's).  With --target-energy E (Kaldi's diarization/score_plda.sh uses 0.1) every recording is
scored as ivector-plda-scoring-dense scores it: with the model projected onto the leading principal directions of the
recording's own x-vectors (xv_plda_adapt, csrc/plda_adapt.hip; plda.adapt_groups states the rule); without it the scores are
those of the global model.  Rows of one recording are merged by average linkage while the best linkage is at
least --threshold (a score: larger = more similar; default 0.0, Kaldi's default), or, with --reco2num-spk (lines
`recording N`), down to N clusters; a recording with fewer rows than N gets one cluster per row and a warning.
<labels-out> ('-': stdout) gets `key label` lines in input order, labels from 1 per recording as agglomerative-cluster writes
them; stdout gets one summary line, `R recordings, N segments, C clusters`.  With --segments (lines `key recording start end`
in seconds) and --rttm-out the labels are also written as RTTM (rttm_lines below, what diarization/make_rttm.py does)."""
import argparse
import collections
import ctypes as C
import sys

import numpy as np

from . import _lib
from ._lib import ptr
from . import scoring

Clustering = collections.namedtuple("Clustering", ["labels", "num_clusters", "merge_a", "merge_b", "merge_height"])

MAX_ROWS = 8192                         # the row-best cache of one group lives in the LDS of one CU
MATRIX_BUDGET_BYTES = 1 << 30           # what the score matrices of one xv_ahc call may take together (at least one group)


def matrix_ld(n):
    """Row stride of a group's matrix inside the packed buffer: n rounded up to 4, at least 4."""
    return max(4, (int(n) + 3) // 4 * 4)


def _targets(num_clusters, count, names=None):
    if num_clusters is None:
        return None
    if isinstance(num_clusters, dict):
        t = [num_clusters[k] for k in names]
    elif np.ndim(num_clusters) == 0:
        t = [num_clusters] * count
    else:
        t = list(num_clusters)
        if len(t) != count:
            raise ValueError("num_clusters: %d entries for %d groups" % (len(t), count))
    t = np.asarray(t, dtype=np.int64)
    if t.size and t.min() < 1:
        raise ValueError("num_clusters must be >= 1, got %d" % t.min())
    return np.minimum(t, 2 ** 31 - 1).astype(np.int32)


def _threshold(threshold):
    t = -np.inf if threshold is None else float(threshold)
    if t != t:
        raise ValueError("threshold is NaN (None means no threshold)")
    return t


def _chunks(sizes, budget):
    """The groups, largest first, in runs whose matrices fit `budget` bytes together (a run holds at least one group) and
    whose smallest group has at least half the rows of its largest.  A call keeps 16 bytes of LDS per row of its largest group
    for EVERY workgroup, so one long recording in a call of short ones would leave them one workgroup per CU; sorted runs keep
    the groups of a call alike (at most 14 extra calls from 8192 rows down)."""
    runs, cur, used = [], [], 0
    for g in sorted(range(len(sizes)), key=lambda g: -sizes[g]):
        n = sizes[g]
        need = 4 * n * matrix_ld(n) if n else 0
        if cur and (used + need > budget or 2 * n < sizes[cur[0]]):
            runs.append(cur)
            cur, used = [], 0
        cur.append(g)
        used += need
    if cur:
        runs.append(cur)
    return runs


def _run(sizes, fill, threshold, targets, device, budget=None):
    """xv_ahc over groups of `sizes` rows -> list of Clustering (numpy).  fill(g, view) writes the scores of group g into
    `view`, its [n, ld] slice of the packed device buffer (only the upper triangle of the first n columns matters).  The groups
    are sent in chunks of similar size whose matrices fit `budget` bytes (_chunks); by the rule the result does not depend on the chunking."""
    for n in sizes:
        if n > MAX_ROWS:
            raise ValueError("a group of %d rows: at most %d can be clustered at once; split the recording" % (n, MAX_ROWS))
    torch = scoring._need_device()
    lib = _lib.load()
    out = [None] * len(sizes)
    with torch.cuda.device(device):
        dev = torch.device("cuda:%d" % device)
        stream = _lib.stream(device)
        for run in _chunks(sizes, MATRIX_BUDGET_BYTES if budget is None else budget):
            rows = np.ascontiguousarray([sizes[g] for g in run], dtype=np.int32)
            tg = None if targets is None else np.ascontiguousarray(targets[run], dtype=np.int32)
            floats = [n * matrix_ld(n) if n else 0 for n in rows.tolist()]
            s = torch.empty((max(sum(floats), 1),), dtype=torch.float32, device=dev)
            off = 0
            for g, n, f in zip(run, rows.tolist(), floats):
                if n:
                    fill(g, s[off:off + f].view(n, matrix_ld(n)))
                off += f
            total = int(rows.sum())
            labels = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)
            merge_a, merge_b = torch.empty_like(labels), torch.empty_like(labels)
            height = torch.empty((max(total, 1),), dtype=torch.float64, device=dev)
            count = torch.empty((len(run),), dtype=torch.int32, device=dev)
            need = int(lib.xv_ahc_workspace(len(run), rows.ctypes.data_as(C.c_void_p)))
            if need < 0:
                raise _lib.XvError(need, "xv_ahc_workspace: bad group sizes")
            ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
            _lib.check(lib.xv_ahc(device, ptr(s), rows.ctypes.data_as(C.c_void_p), None if tg is None else tg.ctypes.data_as(C.c_void_p),
                                  len(run), threshold, ptr(labels), ptr(count), ptr(merge_a), ptr(merge_b), ptr(height), ptr(ws), ws.numel(),
                                  stream))
            labels, merge_a, merge_b, height, count = (t.cpu().numpy() for t in (labels, merge_a, merge_b, height, count))
            off = 0
            for i, (g, n) in enumerate(zip(run, rows.tolist())):
                out[g] = Clustering(labels[off:off + n].copy(), int(count[i]), merge_a[off:off + n].copy(), merge_b[off:off + n].copy(),
                                    height[off:off + n].copy())
                off += n
    return out


def ahc(matrices, threshold=None, num_clusters=None, device=0, budget=None):
    """Cluster every matrix of `matrices` (square [n, n] score matrices, numpy or torch, larger = more similar; only the upper
    triangle is read) -> list of Clustering(labels [n] int32, num_clusters, merge_a, merge_b [n] int32, merge_height [n] float64).
    `threshold` (None: none) stops the merging when the best average linkage falls below it, `num_clusters` (an int, or one per
    matrix; None: 1) when that many clusters are left, whichever comes first.  Labels number the clusters by their lowest row; the
    merge log holds -1 / -1 / NaN past the merges performed and allows the dendrogram to be cut again on the host.
    A non-finite entry in an upper triangle raises ValueError; so does a matrix of more than 8192 rows (split the recording)."""
    torch = scoring._need_device()
    mats = []
    for g, m in enumerate(matrices):
        t = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))
        if t.dim() != 2 or t.shape[0] != t.shape[1]:
            raise ValueError("matrix %d: expected a square [n, n] array, got shape %s" % (g, tuple(t.shape)))
        t = t.to(dtype=torch.float32)
        if t.shape[0] > 1 and not bool(torch.isfinite(torch.triu(t, 1)).all()):
            raise ValueError("matrix %d: a score above the diagonal is not finite" % g)
        mats.append(t)
    sizes = [int(t.shape[0]) for t in mats]

    def fill(g, view):
        view[:, :sizes[g]].copy_(mats[g])

    return _run(sizes, fill, _threshold(threshold), _targets(num_clusters, len(mats)), device, budget)


def _group_rows(groups, n):
    ids = np.asarray(groups).reshape(-1)
    if ids.shape[0] != n:
        raise ValueError("groups: %d ids for %d rows" % (ids.shape[0], n))
    names, inverse = np.unique(ids, return_inverse=True)
    order = np.argsort(inverse, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(names)))])
    return [k.item() if hasattr(k, "item") else k for k in names], [order[bounds[i]:bounds[i + 1]] for i in range(len(names))]


def _by_group(x_rows, groups, fill_rows, threshold, num_clusters, device):
    names, members = _group_rows(groups, x_rows)
    res = _run([len(m) for m in members], lambda g, view: fill_rows(members[g], view), _threshold(threshold),
               _targets(num_clusters, len(names), names), device)
    labels = np.zeros(x_rows, np.int32)
    for m, r in zip(members, res):
        labels[m] = r.labels
    return labels, collections.OrderedDict(zip(names, res))


def cosine(x, groups, threshold=None, num_clusters=None, mean=None, transform=None, normalize=True, device=0):
    """Cluster the rows x [N, d] within every group (recording) by the cosine of the prepared rows (scoring.prepare: mean,
    transform, normalize) -> (labels [N] int32 in input order, OrderedDict group -> Clustering in sorted group order).
    `groups` [N] holds one id per row (anything np.unique sorts); a group's rows keep their input order, so row i of its
    Clustering is the i-th row of x that carries the id.  Every group's matrix is written by xv_score_matrix: its scores are
    bit for bit those of scoring.cosine_matrix over the group's rows.  `num_clusters` may also be a dict by group id."""
    n, _ = scoring._shape2(x, "x")
    torch = scoring._need_device()
    lib = _lib.load()
    rows = scoring.prepare(x, mean=mean, transform=transform, normalize=normalize, device=device, as_tensor=True)
    d = int(rows.shape[1])

    def fill(members, view):
        a = rows[torch.from_numpy(members).to(rows.device)].contiguous()
        stream = _lib.stream(device)
        _lib.check(lib.xv_score_matrix(device, ptr(a), d, len(members), ptr(a), d, len(members), d, ptr(view), view.shape[1],
                                       stream))

    return _by_group(n, groups, fill, threshold, num_clusters, device)


def _plda_fill(model, x, names, members, mean, transform, normalize, normalize_length, simple_length_norm, target_energy, device):
    """The front, the global operands and, with `target_energy`, one xv_plda_adapt over all groups -> fill(g, view), which
    writes the score matrix of group g into `view` [n, ld] with xv_plda_matrix."""
    from . import plda as plda_mod
    torch = scoring._need_device()
    lib = _lib.load()
    front = mean is not None or transform is not None or normalize
    rows = scoring.prepare(x, mean=mean, transform=transform, normalize=normalize, device=device, as_tensor=True) if front else x
    norm = dict(normalize_length=normalize_length, simple_length_norm=simple_length_norm, device=device)
    whole = []

    def global_operands():                # the global model over all rows, as without target_energy; made on first use
        if not whole:
            enroll, test = plda_mod.prepare_enroll(model, rows, **norm), plda_mod.prepare_test(model, rows, **norm)
            whole.append((enroll, test) + plda_mod._operands(enroll, test, "cluster.plda"))
        return whole[0]

    def matrix(a, rho, b, tau, k, count, view):
        stream = _lib.stream(device)
        _lib.check(lib.xv_plda_matrix(device, ptr(a), a.shape[1], count, ptr(rho), ptr(b), b.shape[1], count, ptr(tau), k,
                                      ptr(view), view.shape[1], stream))

    def fill_global(g, view):
        enroll, test, k, tau = global_operands()
        idx = torch.from_numpy(members[g]).to(enroll.packed.device)
        matrix(enroll.packed[idx].contiguous(), enroll.bias[idx].contiguous(), test.packed[idx].contiguous(), tau[idx].contiguous(),
               k, len(members[g]), view)

    if target_energy is None:
        global_operands()
        return fill_global

    with torch.cuda.device(device):
        rows = scoring._rows(rows, device, "x")
        order = np.concatenate(members) if members else np.zeros(0, np.int64)
        xs = rows[torch.from_numpy(order).to(rows.device)].contiguous()
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
    dim, _, _, affine, psi, _ = plda_mod._adapt_raw(model, xs, offsets, target_energy, device, want_pca=False)
    plda_mod._warn_fallback(dim, "cluster.plda")

    def fill(g, view):
        r = int(dim[g])
        if r == 0:
            return fill_global(g, view)
        adapted = plda_mod.AdaptedPlda(None, affine[g, :r], psi[g, :r], None)
        xg = xs[int(offsets[g]):int(offsets[g + 1])]
        enroll, test = plda_mod.prepare_enroll(adapted, xg, **norm), plda_mod.prepare_test(adapted, xg, **norm)
        k, tau = plda_mod._operands(enroll, test, "cluster.plda")
        matrix(enroll.packed, enroll.bias, test.packed, tau, k, len(members[g]), view)

    return fill


def plda(model, x, groups, threshold=None, num_clusters=None, mean=None, transform=None, normalize=True, normalize_length=True,
         simple_length_norm=False, device=0, target_energy=None):
    """cosine() with the PLDA front: the score of rows i and j is the log likelihood ratio of plda.llr_matrix with row i on the
    enrolment side (plda.prepare_enroll, one utterance) and row j on the test side (plda.prepare_test), written by
    xv_plda_matrix.  `model` is a plda.Plda (plda.read_plda, plda.smooth); mean / transform / normalize are the front before it.
    `target_energy` None scores every recording with the one global model.  A value in (0, 1] is Kaldi's
    `ivector-plda-scoring-dense --target-energy`: one xv_plda_adapt call over all recordings (plda.adapt_groups has the rule)
    gives every recording its own PCA-projected model, and its matrix is bit for bit plda.llr_matrix of the recording's rows
    prepared with that model; a recording that cannot be adapted is scored with the global model, and one warning counts
    such recordings."""
    n, _ = scoring._shape2(x, "x")
    names, members = _group_rows(groups, n)
    fill = _plda_fill(model, x, names, members, mean, transform, normalize, normalize_length, simple_length_norm, target_energy, device)
    res = _run([len(m) for m in members], fill, _threshold(threshold), _targets(num_clusters, len(names), names), device)
    labels = np.zeros(n, np.int32)
    for m, r in zip(members, res):
        labels[m] = r.labels
    return labels, collections.OrderedDict(zip(names, res))


def plda_matrices(model, x, groups, mean=None, transform=None, normalize=True, normalize_length=True, simple_length_norm=False,
                  device=0, target_energy=None):
    """The score matrices plda() clusters, one [n, n] float32 numpy array per group -> OrderedDict in sorted group order."""
    n, _ = scoring._shape2(x, "x")
    torch = scoring._need_device()
    names, members = _group_rows(groups, n)
    fill = _plda_fill(model, x, names, members, mean, transform, normalize, normalize_length, simple_length_norm, target_energy, device)
    out = collections.OrderedDict()
    with torch.cuda.device(device):
        for g, (name, m) in enumerate(zip(names, members)):
            buf = torch.empty((len(m), matrix_ld(len(m))), dtype=torch.float32, device="cuda:%d" % device)
            fill(g, buf)
            out[name] = buf[:, :len(m)].cpu().numpy()
    return out


# ---------------------------------------------------------------------------------------------------- host: RTTM

def read_segments(path):
    """Lines `key recording start end` (seconds) -> list of (key, recording, start, end)."""
    out = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            try:
                if len(p) != 4:
                    raise ValueError
                start, end = float(p[2]), float(p[3])
            except ValueError:
                raise ValueError("%s:%d: expected `key recording start end`, got %r" % (path, no, line.rstrip("\n")))
            if not start <= end:
                raise ValueError("%s:%d: the segment ends before it starts" % (path, no))
            out.append((p[0], p[1], start, end))
    return out


def rttm_lines(segments, labels):
    """RTTM text of labelled segments, the restatement of diarization/make_rttm.py (**parity unpinned**).  `segments` is a list
    of (key, recording, start, end); `labels` maps a key to its label (segments whose key has none are left out).  Per
    recording, in sorted order of the recordings: the segments are sorted by start (then end, then key); a segment that touches
    or overlaps its predecessor and carries the same label is merged into it; where neighbours with different labels overlap
    both are cut at the midpoint of the overlap; what is left with a positive duration is written as
    `SPEAKER <recording> 1 <start %.3f> <duration %.3f> <NA> <NA> <label> <NA> <NA>`."""
    per = collections.OrderedDict()
    for key, reco, start, end in segments:
        if key in labels:
            per.setdefault(reco, []).append((float(start), float(end), key, labels[key]))
    lines = []
    for reco in sorted(per):
        turns = []
        for start, end, _, lab in sorted(per[reco], key=lambda t: t[:3]):
            if turns and turns[-1][2] == lab and start <= turns[-1][1]:
                turns[-1][1] = max(turns[-1][1], end)
                continue
            if turns and start < turns[-1][1]:
                mid = 0.5 * (turns[-1][1] + start)
                turns[-1][1] = mid
                start = mid
            turns.append([start, end, lab])
        for start, end, lab in turns:
            if end > start:
                lines.append("SPEAKER %s 1 %.3f %.3f <NA> <NA> %s <NA> <NA>\n" % (reco, start, end - start, lab))
    return "".join(lines)


# ---------------------------------------------------------------------------------------------------- command line

def read_reco2num_spk(path):
    """Lines `recording N`, N >= 1 -> dict."""
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if len(p) != 2 or not p[1].isdigit() or int(p[1]) < 1:
                raise ValueError("%s:%d: expected `recording N` with N >= 1, got %r" % (path, no, line.rstrip("\n")))
            out[p[0]] = int(p[1])
    return out


def format_labels(keys, labels):
    """`key label` lines, labels from 1."""
    return "".join("%s %d\n" % (k, int(l) + 1) for k, l in zip(keys, labels))


def parse_args(argv=None):
    from .score_cos import _bool
    ap = argparse.ArgumentParser(prog="cluster", description=__doc__.split("\n\n")[0])
    ap.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--threshold", type=float, default=None,
                    help="stop merging when the best average linkage is below this score; default 0.0 (without --reco2num-spk)")
    ap.add_argument("--reco2num-spk", default="", help="`recording N` lines: merge every recording down to N clusters instead")
    ap.add_argument("--mean", default="", help="Kaldi vector subtracted from every x-vector (ivector-subtract-global-mean)")
    ap.add_argument("--transform", default="", help="Kaldi matrix applied after the mean (transform-vec; [d_out, d] or [d_out, d + 1])")
    ap.add_argument("--normalize", type=_bool, default=True, help="length-normalise last (ivector-normalize-length); default true")
    ap.add_argument("--plda", default="", help="Kaldi Plda: score by log likelihood ratio instead of cosine")
    ap.add_argument("--smoothing", type=float, default=None, help="ivector-copy-plda --smoothing; default 0.0; needs --plda")
    ap.add_argument("--normalize-length", type=_bool, default=None, help="ivector-plda-scoring --normalize-length; default true; needs --plda")
    ap.add_argument("--simple-length-normalization", type=_bool, default=None,
                    help="ivector-plda-scoring --simple-length-normalization; default false; needs --plda")
    ap.add_argument("--target-energy", type=float, default=None,
                    help="ivector-plda-scoring-dense --target-energy, in (0, 1]: score every recording in the PCA subspace of its own "
                         "x-vectors that holds this share of their variance; default: the global model; needs --plda")
    ap.add_argument("--segments", default="", help="`key recording start end` lines; with --rttm-out: write the labels as RTTM")
    ap.add_argument("--rttm-out", default="", help="RTTM file to write; needs --segments")
    ap.add_argument("utt2reco")
    ap.add_argument("xvector_rspecifier")
    ap.add_argument("labels_out")
    args = ap.parse_args(argv)
    if args.threshold is not None and args.reco2num_spk:
        ap.error("--threshold and --reco2num-spk exclude each other")
    if args.threshold is not None and args.threshold != args.threshold:
        ap.error("--threshold is NaN")
    if args.threshold is None and not args.reco2num_spk:
        args.threshold = 0.0
    if not args.plda:
        for name, value in (("--smoothing", args.smoothing), ("--normalize-length", args.normalize_length),
                            ("--simple-length-normalization", args.simple_length_normalization),
                            ("--target-energy", args.target_energy)):
            if value is not None:
                ap.error("%s needs --plda" % name)
    args.smoothing = 0.0 if args.smoothing is None else args.smoothing
    args.normalize_length = True if args.normalize_length is None else args.normalize_length
    args.simple_length_normalization = bool(args.simple_length_normalization)
    if not 0.0 <= args.smoothing <= 1.0:
        ap.error("--smoothing must be in [0, 1]")
    if args.target_energy is not None and not 0.0 < args.target_energy <= 1.0:
        ap.error("--target-energy must be in (0, 1]")
    if bool(args.segments) != bool(args.rttm_out):
        ap.error("--segments and --rttm-out are given together")
    return args


def main(argv=None):
    args = parse_args(argv)
    from . import kaldi_io
    from . import postprocess
    from .score_cos import _rspec, read_utt2spk
    utt2reco = read_utt2spk(args.utt2reco)
    keys, x = postprocess.read_vectors(_rspec(args.xvector_rspecifier))
    if not keys:
        sys.stderr.write("cluster: the x-vector table is empty\n")
        return 1
    missing = [k for k in keys if k not in utt2reco]
    if missing:
        sys.stderr.write("cluster: %d keys have no recording in %s (first: %s)\n" % (len(missing), args.utt2reco, missing[0]))
        return 1
    recos = np.array([utt2reco[k] for k in keys], dtype=object).astype(str)
    targets = None
    if args.reco2num_spk:
        num_spk = read_reco2num_spk(args.reco2num_spk)
        names, counts = np.unique(recos, return_counts=True)
        absent = [r for r in names.tolist() if r not in num_spk]
        if absent:
            sys.stderr.write("cluster: %d recordings have no entry in %s (first: %s)\n" % (len(absent), args.reco2num_spk, absent[0]))
            return 1
        for r, c in zip(names.tolist(), counts.tolist()):
            if c < num_spk[r]:
                sys.stderr.write("cluster: warning: recording %s has %d segments for %d speakers: one cluster per segment\n" % (r, c, num_spk[r]))
        targets = {r: num_spk[r] for r in names.tolist()}
    mean = np.asarray(kaldi_io.read_vec_flt(args.mean), dtype=np.float32) if args.mean else None
    transform = np.asarray(kaldi_io.read_mat(args.transform), dtype=np.float32) if args.transform else None
    front = dict(threshold=args.threshold, num_clusters=targets, mean=mean, transform=transform, normalize=args.normalize, device=args.gpu)
    try:
        if args.plda:
            from . import plda as plda_mod
            model = plda_mod.smooth(plda_mod.read_plda(args.plda), args.smoothing)
            labels, per = plda(model, x, recos, normalize_length=args.normalize_length, simple_length_norm=args.simple_length_normalization,
                               target_energy=args.target_energy, **front)
        else:
            labels, per = cosine(x, recos, **front)
    except ValueError as e:
        sys.stderr.write("cluster: %s\n" % e)
        return 1
    if args.labels_out == "-":
        sys.stdout.write(format_labels(keys, labels))
    else:
        with open(args.labels_out, "w") as f:
            f.write(format_labels(keys, labels))
    if args.rttm_out:
        text = rttm_lines(read_segments(args.segments), {k: int(l) + 1 for k, l in zip(keys, labels)})
        with open(args.rttm_out, "w") as f:
            f.write(text)
    print("%d recordings, %d segments, %d clusters" % (len(per), len(keys), sum(r.num_clusters for r in per.values())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
