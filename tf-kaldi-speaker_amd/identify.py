"""Closed-set speaker identification on the GPU: for every query x-vector the K best entries of a gallery, by cosine or by
PLDA log likelihood ratio, without the [queries, gallery] score matrix (xv_score_topk through scoring.top_k / plda.llr_top_k).

    python -m tf_kaldi_speaker_amd.identify [--gpu 0] [--top-k 10] [--mean mean.vec] [--transform transform.mat]
           [--normalize true] [--plda plda [--num-utts ark:num_utts.ark] [--smoothing 0.0] [--normalize-length true]
           [--simple-length-normalization false]] [--exclude-utt2spk utt2spk]
           [--gallery-utt2spk FILE --query-utt2spk FILE [--ranks 1,5,10]]
           <gallery-rspecifier> <query-rspecifier> <out>

Both tables go through the front of score_cos (--mean, --transform, --normalize: ivector-subtract-global-mean | transform-vec |
ivector-normalize-length).  Without --plda the score is the cosine of the prepared rows.  With --plda the gallery stands on the
enrolment side and the queries on the test side of ivector-plda-scoring, and --num-utts (counts of the gallery keys),
--smoothing, --normalize-length and --simple-length-normalization are score_plda's options with score_plda's meaning.
--exclude-utt2spk (lines `key label`, as in score_cos) keeps a query from finding gallery entries of its own label: give the
same table twice and an utt2spk that labels every key by itself to search a set against itself.

<out> ('-': stdout) gets one line per hit, `query_id gallery_id score`, grouped by query in input order and in rank order
within a query: score descending, gallery order among equal scores.  A query with fewer than --top-k eligible gallery entries
gets fewer lines.  With --gallery-utt2spk and --query-utt2spk the identification rates are printed on stdout as one line,
`rank-1 0.9731 rank-5 0.9912 rank-10 0.9950 (N queries, M without a gallery entry)`: the fraction of all queries whose label
is carried by one of their first r hits; a query whose label no gallery entry carries counts as a miss.  --ranks defaults to
those of 1,5,10 that --top-k allows.  The reference has no identification step: **parity unpinned**."""
import argparse
import sys

import numpy as np

from . import kaldi_io
from . import scoring
from .score_cos import _bool, _table, exclusion_labels, read_utt2spk


def _ranks(s):
    try:
        v = [int(p) for p in s.split(",")]
    except ValueError:
        v = []
    if not v or any(r < 1 for r in v):
        raise argparse.ArgumentTypeError("expected positive ranks such as 1,5,10, got %r" % s)
    return v


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="identify", description=__doc__.split("\n\n")[0])
    ap.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--top-k", type=int, default=10, help="hits per query, 1..1024; default 10")
    ap.add_argument("--mean", default="", help="Kaldi vector subtracted from every x-vector (ivector-subtract-global-mean)")
    ap.add_argument("--transform", default="", help="Kaldi matrix applied after the mean (transform-vec; [d_out, d] or [d_out, d + 1])")
    ap.add_argument("--normalize", type=_bool, default=True, help="length-normalise last (ivector-normalize-length); default true")
    ap.add_argument("--plda", default="", help="Kaldi Plda: score by log likelihood ratio (gallery = enrolment side) instead of cosine")
    ap.add_argument("--num-utts", default=None, help="ark,t: int table of utterance counts per gallery key (default: 1); needs --plda")
    ap.add_argument("--smoothing", type=float, default=None, help="ivector-copy-plda --smoothing; default 0.0; needs --plda")
    ap.add_argument("--normalize-length", type=_bool, default=None, help="ivector-plda-scoring --normalize-length; default true; needs --plda")
    ap.add_argument("--simple-length-normalization", type=_bool, default=None,
                    help="ivector-plda-scoring --simple-length-normalization; default false; needs --plda")
    ap.add_argument("--exclude-utt2spk", default="", help="`key label` lines: gallery entries of a query's own label are left out")
    ap.add_argument("--gallery-utt2spk", default="", help="`key label` lines for the gallery; with --query-utt2spk: print identification rates")
    ap.add_argument("--query-utt2spk", default="", help="`key label` lines for the queries")
    ap.add_argument("--ranks", type=_ranks, default=None, help="ranks of the identification rates; default 1,5,10 as far as --top-k allows")
    ap.add_argument("gallery_rspecifier")
    ap.add_argument("query_rspecifier")
    ap.add_argument("out")
    args = ap.parse_args(argv)
    if not 1 <= args.top_k <= 1024:
        ap.error("--top-k must be in 1..1024")
    if not args.plda:
        for name, value in (("--num-utts", args.num_utts), ("--smoothing", args.smoothing), ("--normalize-length", args.normalize_length),
                            ("--simple-length-normalization", args.simple_length_normalization)):
            if value is not None:
                ap.error("%s needs --plda" % name)
    args.smoothing = 0.0 if args.smoothing is None else args.smoothing
    args.normalize_length = True if args.normalize_length is None else args.normalize_length
    args.simple_length_normalization = bool(args.simple_length_normalization)
    if not 0.0 <= args.smoothing <= 1.0:
        ap.error("--smoothing must be in [0, 1]")
    if bool(args.gallery_utt2spk) != bool(args.query_utt2spk):
        ap.error("--gallery-utt2spk and --query-utt2spk are given together")
    if args.ranks is not None and not args.gallery_utt2spk:
        ap.error("--ranks needs --gallery-utt2spk and --query-utt2spk")
    if args.ranks is None:
        args.ranks = [r for r in (1, 5, 10) if r <= args.top_k]
    elif max(args.ranks) > args.top_k:
        ap.error("--ranks %s with --top-k %d" % (",".join(str(r) for r in args.ranks), args.top_k))
    return args


def format_hits(query_keys, gallery_keys, hits):
    """scoring.TopK on the host -> the text of <out>: `query_id gallery_id score` (%g), padded positions left out."""
    lines = []
    for q, key in enumerate(query_keys):
        for r in range(int(hits.count[q])):
            lines.append("%s %s %g\n" % (key, gallery_keys[int(hits.indices[q, r])], hits.scores[q, r]))
    return "".join(lines)


def format_rates(rates, queries, absent):
    return "%s (%d queries, %d without a gallery entry)" % (" ".join("rank-%d %.4f" % (r, v) for r, v in rates.items()), queries, absent)


def _labels(tool, path, row, what):
    spk = read_utt2spk(path)
    missing = [k for k in row if k not in spk]
    if missing:
        sys.stderr.write("%s: %d %s keys have no label in %s (first: %s)\n" % (tool, len(missing), what, path, missing[0]))
        return None
    lab = [None] * len(row)
    for k, i in row.items():
        lab[i] = spk[k]
    return np.array(lab, dtype=object).astype(str)


def main(argv=None):
    args = parse_args(argv)
    mean = np.asarray(kaldi_io.read_vec_flt(args.mean), dtype=np.float32) if args.mean else None
    transform = np.asarray(kaldi_io.read_mat(args.transform), dtype=np.float32) if args.transform else None
    rowg, xg = _table(args.gallery_rspecifier, mean, transform, args.normalize, args.gpu)
    rowq, xq = (rowg, xg) if args.query_rspecifier == args.gallery_rspecifier else _table(args.query_rspecifier, mean, transform,
                                                                                         args.normalize, args.gpu)
    if not rowg or not rowq:
        sys.stderr.write("identify: the %s table is empty\n" % ("gallery" if not rowg else "query"))
        return 1
    lq = lg = None
    if args.exclude_utt2spk:
        lq, lg = exclusion_labels(read_utt2spk(args.exclude_utt2spk), rowq, rowg)
    if args.plda:
        from . import plda
        from .score_plda import read_num_utts
        model = plda.smooth(plda.read_plda(args.plda), args.smoothing)
        num_utts = None
        if args.num_utts:
            counts = read_num_utts(args.num_utts)
            num_utts = np.ones(len(rowg), np.int64)
            for k, i in rowg.items():
                num_utts[i] = counts.get(k, 1)
            absent = sum(1 for k in rowg if k not in counts)
            if absent:
                sys.stderr.write("identify: %d of %d gallery keys have no --num-utts entry (counted as 1)\n" % (absent, len(rowg)))
        norm = dict(normalize_length=args.normalize_length, simple_length_norm=args.simple_length_normalization, device=args.gpu)
        hits = plda.llr_top_k(plda.prepare_enroll(model, xg, num_utts=num_utts, **norm), plda.prepare_test(model, xq, **norm),
                              args.top_k, per="test", labels_enroll=lg, labels_test=lq)
    else:
        hits = scoring.top_k(xq, xg, args.top_k, labels_a=lq, labels_b=lg, device=args.gpu)
    gallery_keys, query_keys = sorted(rowg, key=rowg.get), sorted(rowq, key=rowq.get)
    text = format_hits(query_keys, gallery_keys, hits)
    with (sys.stdout if args.out == "-" else open(args.out, "w")) as f:
        f.write(text)
    sys.stderr.write("identify: %d queries against %d gallery entries, %d hits\n" % (len(rowq), len(rowg), int(np.sum(hits.count))))
    if args.gallery_utt2spk:
        gl = _labels("identify", args.gallery_utt2spk, rowg, "gallery")
        ql = _labels("identify", args.query_utt2spk, rowq, "query")
        if gl is None or ql is None:
            return 1
        rates, absent = scoring.identification_rate(hits.indices, ql, gl, ranks=args.ranks)
        print(format_rates(rates, len(rowq), absent))
    return 0


if __name__ == "__main__":
    sys.exit(main())
