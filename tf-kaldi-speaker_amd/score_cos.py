"""Cosine scoring of a trial list on the GPU: the reference's cosine back-end without the Kaldi binaries
(egs/voxceleb/v1/run.sh:362-365: `ivector-normalize-length` x 2 | `ivector-compute-dot-products`; :404-408: the same
behind `ivector-subtract-global-mean mean.vec` | `transform-vec transform.mat`).

    python -m tf_kaldi_speaker_amd.score_cos [--gpu 0] [--mean mean.vec] [--transform transform.mat]
           [--normalize true] [--eer] [--cohort <rspecifier> [--norm z|t|s] [--top-k N] [--exclude-utt2spk FILE]]
           <trials> <rspecifier1> <rspecifier2> <scores-out>

Trials are lines `key1 key2 [target|nontarget]`; key1 is looked up in table 1 and key2 in table 2, and the output lines
are `key1 key2 score` in trial order, as ivector-compute-dot-products writes them.  A trial whose key is missing from
its table is skipped and counted (reported on stderr); the exit status is non-zero only if no trial was scored.  That is
Kaldi's behaviour as published; Kaldi is absent from the reference tree, so this is **parity unpinned**.  `--eer` needs
the third column and prints `EER: x%`, the exact EER of the scores as written (from the sorted scores, on the host,
what `compute-eer` would be given).  PLDA scoring is score_plda.py, which shares the helpers below.

`--cohort` turns on score normalisation (snorm.py; the reference has none: **parity unpinned**): the cohort table goes through
the same --mean / --transform / --normalize front, `--norm` is z, t or s (default s), `--top-k N` keeps the N largest cohort
scores per row (default 0: all of them) and `--exclude-utt2spk FILE` (lines `key label`) keeps a row from being normalised
by cohort rows of its own label; keys of any of the three tables found in the file get that label, keys not in it are never
excluded.  The scores written, and --eer, are then the normalised ones.  Without --cohort nothing changes."""
import argparse
import sys

import numpy as np

from . import kaldi_io
from . import postprocess
from . import scoring


def _bool(s):
    if s.lower() in ("true", "1", "yes"):
        return True
    if s.lower() in ("false", "0", "no"):
        return False
    raise argparse.ArgumentTypeError("expected true or false, got %r" % s)


def _rspec(s):
    return s if ":" in s.split("/")[0] else "ark:" + s


def _table(rspecifier, mean, transform, normalize, device):
    keys, x = postprocess.read_vectors(_rspec(rspecifier))
    if not keys:
        return {}, None
    rows = scoring.prepare(x, mean=mean, transform=transform, normalize=normalize, eps=0.0, device=device, as_tensor=True)
    return {k: i for i, k in enumerate(keys)}, rows


def select_trials(tool, keys1, keys2, row1, row2):
    """Numbers of the trials whose keys are both in their tables (the others are skipped and counted on stderr), or None
    when there is none."""
    kept = [t for t in range(len(keys1)) if keys1[t] in row1 and keys2[t] in row2]
    skipped = len(keys1) - len(kept)
    if skipped:
        sys.stderr.write("%s: skipped %d of %d trials (key not in its table)\n" % (tool, skipped, len(keys1)))
    if not kept:
        sys.stderr.write("%s: no trial was scored\n" % tool)
        return None
    return kept


def write_scores(tool, path, keys1, keys2, kept, scores):
    """Lines `key1 key2 score` (%g) in trial order to `path` ('-': stdout) -> the scores as printed."""
    text = ["%g" % s for s in scores]
    with (sys.stdout if path == "-" else open(path, "w")) as f:
        f.write("".join("%s %s %s\n" % (keys1[t], keys2[t], s) for t, s in zip(kept, text)))
    sys.stderr.write("%s: scored %d trials\n" % (tool, len(kept)))
    return [float(s) for s in text]


def add_snorm_options(ap):
    ap.add_argument("--cohort", default="", help="cohort table for score normalisation (same front as the other two tables)")
    ap.add_argument("--norm", choices=("z", "t", "s"), default=None, help="z-norm, t-norm or s-norm; default s when a cohort is given")
    ap.add_argument("--top-k", type=int, default=None, help="adaptive cohort: the N largest cohort scores per row; default 0 (all)")
    ap.add_argument("--exclude-utt2spk", default="", help="`key label` lines: cohort rows of a row's own label are left out")


def check_snorm_options(ap, args):
    """--norm, --top-k and --exclude-utt2spk belong to --cohort; fills in their defaults."""
    if not args.cohort:
        for name, value in (("--norm", args.norm), ("--top-k", args.top_k), ("--exclude-utt2spk", args.exclude_utt2spk or None)):
            if value is not None:
                ap.error("%s needs --cohort" % name)
        return
    args.norm = args.norm or "s"
    args.top_k = 0 if args.top_k is None else args.top_k
    if args.top_k < 0:
        ap.error("--top-k must be >= 0")


def read_utt2spk(path):
    """Lines `key label` -> dict."""
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if len(p) != 2:
                raise ValueError("%s:%d: expected `key label`, got %r" % (path, no, line.rstrip("\n")))
            out[p[0]] = p[1]
    return out


def exclusion_labels(spk, *tables):
    """One label array per table (dict key -> row): the label of the key in `spk`, or one no other row carries."""
    out = []
    for no, row in enumerate(tables):
        lab = [None] * len(row)
        for k, i in row.items():
            lab[i] = "s " + spk[k] if k in spk else "u%d %s" % (no, k)      # a label holds no blank: the two kinds never meet
        out.append(np.array(lab, dtype=object).astype(str))
    return out


def normalise_scores(tool, args, scores, ia, ib, row1, row2, rowc, stats):
    """The --cohort step behind both tools: `stats(side, labels, cohort_labels)` -> snorm.CohortStats of side "enroll" / "test".
    -> normalised scores, or None (reported on stderr) when a row used by a trial has no usable cohort statistics."""
    from . import snorm
    l1 = l2 = lc = None
    if args.exclude_utt2spk:
        l1, l2, lc = exclusion_labels(read_utt2spk(args.exclude_utt2spk), row1, row2, rowc)
    ze = stats("enroll", l1, lc) if args.norm in ("z", "s") else None
    zt = stats("test", l2, lc) if args.norm in ("t", "s") else None
    try:
        return snorm.normalize(scores, ia, ib, ze, zt, mode=args.norm)
    except ValueError as e:
        sys.stderr.write("%s: %s\n" % (tool, e))
        return None


def main(argv=None):
    ap = argparse.ArgumentParser(prog="score_cos", description=__doc__.split("\n\n")[0])
    ap.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--mean", default="", help="Kaldi vector subtracted from every x-vector (ivector-subtract-global-mean)")
    ap.add_argument("--transform", default="", help="Kaldi matrix applied after the mean (transform-vec; [d_out, d] or [d_out, d + 1])")
    ap.add_argument("--normalize", type=_bool, default=True, help="length-normalise last (ivector-normalize-length); default true")
    ap.add_argument("--eer", action="store_true", help="print the exact EER of the scored trials (needs labelled trials)")
    add_snorm_options(ap)
    ap.add_argument("trials")
    ap.add_argument("rspecifier1")
    ap.add_argument("rspecifier2")
    ap.add_argument("scores_out")
    args = ap.parse_args(argv)
    check_snorm_options(ap, args)

    keys1, keys2, targets = scoring.read_trials(args.trials)
    if args.eer and targets is None:
        sys.stderr.write("score_cos: --eer needs trials with a target / nontarget column\n")
        return 2
    mean = np.asarray(kaldi_io.read_vec_flt(args.mean), dtype=np.float32) if args.mean else None
    transform = np.asarray(kaldi_io.read_mat(args.transform), dtype=np.float32) if args.transform else None
    row1, x1 = _table(args.rspecifier1, mean, transform, args.normalize, args.gpu)
    row2, x2 = (row1, x1) if args.rspecifier2 == args.rspecifier1 else _table(args.rspecifier2, mean, transform,
                                                                             args.normalize, args.gpu)
    kept = select_trials("score_cos", keys1, keys2, row1, row2)
    if kept is None:
        return 1
    ia = np.fromiter((row1[keys1[t]] for t in kept), dtype=np.int64, count=len(kept))
    ib = np.fromiter((row2[keys2[t]] for t in kept), dtype=np.int64, count=len(kept))
    scores = scoring.cosine_pairs(x1, x2, ia, ib, device=args.gpu)
    if args.cohort:
        from . import snorm
        rowc, xc = _table(args.cohort, mean, transform, args.normalize, args.gpu)
        if not rowc:
            sys.stderr.write("score_cos: the cohort table is empty\n")
            return 1

        def stats(side, labels, cohort_labels):
            return snorm.cohort_stats(x1 if side == "enroll" else x2, xc, top_k=args.top_k, labels=labels,
                                      cohort_labels=cohort_labels, device=args.gpu)
        scores = normalise_scores("score_cos", args, scores, ia, ib, row1, row2, rowc, stats)
        if scores is None:
            return 1
    printed = write_scores("score_cos", args.scores_out, keys1, keys2, kept, scores)
    if args.eer:
        eer = scoring.exact_eer(printed, [targets[t] for t in kept])
        print("EER: %.4g%%" % (100.0 * eer))
    return 0


if __name__ == "__main__":
    sys.exit(main())
