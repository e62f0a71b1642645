"""Score calibration and fusion of Kaldi-style score files on the GPU (calibration.py): what the reference leaves to outside
tools, and the weighted form of its misc/utils/average_score.py.  **Parity unpinned**, as calibration.py.

    python -m tf_kaldi_speaker_amd.calibrate train [--prior 0.01] [--gpu 0] <trials> <model-out> <scores1> [<scores2> ...]
    python -m tf_kaldi_speaker_amd.calibrate apply [--gpu 0] <model> <llr-out> <scores1> [<scores2> ...]
    python -m tf_kaldi_speaker_amd.calibrate eval  [--gpu 0] [--p-target P[,C_MISS[,C_FA]]]... <trials> <scores>

Score files hold `key1 key2 score` lines, trials `key1 key2 target|nontarget` lines.  `train` fits one weight per score file
and a bias to the labelled trials and writes the model (text, numbers only).  `apply` writes `key1 key2 llr` (%g) in the order
of the first score file.  `eval` prints one line: EER, then minDCF and actDCF per operating point (default 0.01), then Cllr.
A trial (for `apply`: a line of the first score file) that a score file lacks is skipped and counted on stderr; the exit
status is non-zero only when nothing is left, as score_cos does."""
import argparse
import sys

import numpy as np

from . import calibration
from . import scoring


def read_scores(path):
    """Lines `key1 key2 score` -> (pairs in file order, dict pair -> score); of a repeated pair the last line counts."""
    pairs, table = [], {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            try:
                if len(p) != 3:
                    raise ValueError
                v = float(p[2])
            except ValueError:
                raise ValueError("%s:%d: expected `key1 key2 score`, got %r" % (path, no, line.rstrip("\n")))
            if (p[0], p[1]) not in table:
                pairs.append((p[0], p[1]))
            table[(p[0], p[1])] = v
    return pairs, table


def join_scores(tool, pairs, tables):
    """The pairs that every table holds, in order -> (kept numbers, scores [len(kept), len(tables)] float32), or (None, None)
    when none is left; the others are skipped and counted on stderr."""
    kept = [i for i, p in enumerate(pairs) if all(p in t for t in tables)]
    skipped = len(pairs) - len(kept)
    if skipped:
        sys.stderr.write("%s: skipped %d of %d trials (not in every score file)\n" % (tool, skipped, len(pairs)))
    if not kept:
        sys.stderr.write("%s: no trial is left\n" % tool)
        return None, None
    return kept, np.array([[t[pairs[i]] for t in tables] for i in kept], dtype=np.float32)


def _labelled_trials(tool, path):
    k1, k2, targets = scoring.read_trials(path)
    if targets is None:
        sys.stderr.write("%s: the trials need a target / nontarget column\n" % tool)
        return None, None
    return list(zip(k1, k2)), targets


def _point(s):
    try:
        v = [float(x) for x in s.split(",")]
        if not 1 <= len(v) <= 3:
            raise ValueError
        v += [1.0] * (3 - len(v))
        calibration.bayes_threshold(*v)
    except ValueError:
        raise argparse.ArgumentTypeError("expected P[,C_MISS[,C_FA]] with 0 < P < 1 and positive costs, got %r" % s)
    return tuple(v)


def train(args):
    pairs, targets = _labelled_trials("calibrate train", args.trials)
    if pairs is None:
        return 2
    kept, scores = join_scores("calibrate train", pairs, [read_scores(p)[1] for p in args.scores])
    if kept is None:
        return 1
    model, report = calibration.fit(scores, [targets[i] for i in kept], prior=args.prior, device=args.gpu)
    calibration.write_model(args.model, model)
    sys.stderr.write("calibrate train: %d trials, %d systems, %d Newton steps, objective %.6g, decrement %.3g\n"
                     % (len(kept), scores.shape[1], report.iterations, report.F, report.decrement))
    return 0


def apply(args):
    model = calibration.read_model(args.model)
    if len(args.scores) != model.weights.size:
        sys.stderr.write("calibrate apply: %d score files for a model of %d systems\n" % (len(args.scores), model.weights.size))
        return 2
    first = read_scores(args.scores[0])
    tables = [first[1]] + [read_scores(p)[1] for p in args.scores[1:]]
    kept, scores = join_scores("calibrate apply", first[0], tables)
    if kept is None:
        return 1
    llr = calibration.apply(model, scores, device=args.gpu)
    with (sys.stdout if args.out == "-" else open(args.out, "w")) as f:
        f.write("".join("%s %s %g\n" % (first[0][i][0], first[0][i][1], v) for i, v in zip(kept, llr)))
    sys.stderr.write("calibrate apply: wrote %d trials\n" % len(kept))
    return 0


def evaluate(args):
    pairs, targets = _labelled_trials("calibrate eval", args.trials)
    if pairs is None:
        return 2
    kept, scores = join_scores("calibrate eval", pairs, [read_scores(args.scores)[1]])
    if kept is None:
        return 1
    llr, t = scores[:, 0], np.array([targets[i] for i in kept], dtype=bool)
    points = args.p_target or [(0.01, 1.0, 1.0)]
    if len(points) > calibration.MAX_THRESHOLDS:
        sys.stderr.write("calibrate eval: at most %d operating points\n" % calibration.MAX_THRESHOLDS)
        return 2
    cllr, act = calibration.evaluate(llr, t, points, device=args.gpu)
    out = ["EER: %.4g%%" % (100.0 * scoring.exact_eer(llr, t))]
    for (p, c_miss, c_fa), a in zip(points, act):
        name = "p=%g" % p if (c_miss, c_fa) == (1.0, 1.0) else "p=%g,%g,%g" % (p, c_miss, c_fa)
        out.append("minDCF(%s): %.4f actDCF(%s): %.4f" % (name, scoring.min_dcf(llr, t, p, c_miss, c_fa)[0], name, a))
    out.append("Cllr: %.4f" % cllr)
    print(" ".join(out))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="calibrate", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command")
    sub.required = True
    p = sub.add_parser("train", help="fit weights and a bias to labelled trials")
    p.add_argument("--prior", type=float, default=0.01, help="target prior of the objective; default 0.01")
    p.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    p.add_argument("trials")
    p.add_argument("model")
    p.add_argument("scores", nargs="+")
    p.set_defaults(run=train)
    p = sub.add_parser("apply", help="scores -> calibrated, fused llr")
    p.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    p.add_argument("model")
    p.add_argument("out")
    p.add_argument("scores", nargs="+")
    p.set_defaults(run=apply)
    p = sub.add_parser("eval", help="EER, minDCF, actDCF and Cllr of one score file")
    p.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    p.add_argument("--p-target", type=_point, action="append", help="operating point P[,C_MISS[,C_FA]]; repeatable; default 0.01")
    p.add_argument("trials")
    p.add_argument("scores")
    p.set_defaults(run=evaluate)
    args = ap.parse_args(argv)
    if args.command == "train" and not 0.0 < args.prior < 1.0:
        ap.error("--prior must lie in (0, 1)")
    if len(getattr(args, "scores", [])) > calibration.MAX_SYSTEMS and args.command != "eval":
        ap.error("at most %d score files" % calibration.MAX_SYSTEMS)
    try:
        return args.run(args)
    except (ValueError, RuntimeError) as e:
        sys.stderr.write("calibrate %s: %s\n" % (args.command, e))
        return 1


if __name__ == "__main__":
    sys.exit(main())
