"""Cosine scoring of a trial list on the GPU: the reference's cosine back-end without the Kaldi binaries
(egs/voxceleb/v1/run.sh:362-365: `ivector-normalize-length` x 2 | `ivector-compute-dot-products`; :404-408: the same
behind `ivector-subtract-global-mean mean.vec` | `transform-vec transform.mat`).

    python -m tf_kaldi_speaker_amd.score_cos [--gpu 0] [--mean mean.vec] [--transform transform.mat]
           [--normalize true] [--eer] <trials> <rspecifier1> <rspecifier2> <scores-out>

Trials are lines `key1 key2 [target|nontarget]`; key1 is looked up in table 1 and key2 in table 2, and the output lines
are `key1 key2 score` in trial order, as ivector-compute-dot-products writes them.  A trial whose key is missing from
its table is skipped and counted (reported on stderr); the exit status is non-zero only if no trial was scored.  That is
Kaldi's behaviour as published; Kaldi is absent from the reference tree, so this is **parity unpinned**.  `--eer` needs
the third column and prints `EER: x%`, the exact EER of the scores as written (from the sorted scores, on the host,
what `compute-eer` would be given).  PLDA scoring is score_plda.py, which shares the helpers below."""
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


def main(argv=None):
    ap = argparse.ArgumentParser(prog="score_cos", description=__doc__.split("\n\n")[0])
    ap.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--mean", default="", help="Kaldi vector subtracted from every x-vector (ivector-subtract-global-mean)")
    ap.add_argument("--transform", default="", help="Kaldi matrix applied after the mean (transform-vec; [d_out, d] or [d_out, d + 1])")
    ap.add_argument("--normalize", type=_bool, default=True, help="length-normalise last (ivector-normalize-length); default true")
    ap.add_argument("--eer", action="store_true", help="print the exact EER of the scored trials (needs labelled trials)")
    ap.add_argument("trials")
    ap.add_argument("rspecifier1")
    ap.add_argument("rspecifier2")
    ap.add_argument("scores_out")
    args = ap.parse_args(argv)

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
    printed = write_scores("score_cos", args.scores_out, keys1, keys2, kept, scores)
    if args.eer:
        eer = scoring.exact_eer(printed, [targets[t] for t in kept])
        print("EER: %.4g%%" % (100.0 * eer))
    return 0


if __name__ == "__main__":
    sys.exit(main())
