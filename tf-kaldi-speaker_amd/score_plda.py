"""PLDA scoring of a trial list on the GPU with a trained Kaldi `Plda`: the reference's PLDA back-end without the Kaldi
binaries (egs/voxceleb/v1/run.sh:410-426, egs/sre/v1/run.sh:415-491, egs/fisher/v1/eval_plda.sh):

    ivector-plda-scoring --normalize-length=true [--num-utts=ark:num_utts.ark] "ivector-copy-plda --smoothing=0.0 plda - |"
        "ark:ivector-subtract-global-mean mean.vec scp:enroll.scp ark:- | transform-vec transform.mat ark:- ark:- | ivector-normalize-length ark:- ark:- |"
        "ark:ivector-subtract-global-mean mean.vec scp:test.scp ark:- | transform-vec transform.mat ark:- ark:- | ivector-normalize-length ark:- ark:- |"
        trials scores

    python -m tf_kaldi_speaker_amd.score_plda [--gpu 0] [--normalize-length true] [--simple-length-normalization false]
           [--num-utts ark:num_utts.ark] [--smoothing 0.0] [--mean mean.vec] [--transform transform.mat]
           [--front-normalize true] [--eer] [--min-dcf P_TARGET[,C_MISS[,C_FA]] ...]
           [--cohort <rspecifier> [--norm z|t|s] [--top-k N] [--exclude-utt2spk FILE]]
           <plda> <enroll-rspecifier> <test-rspecifier> <trials> <scores-out>

The positional order is ivector-plda-scoring's (model first, trials fourth; score_cos takes the trials first).  --mean,
--transform and --front-normalize are the front chain of the two rspecifiers (score_cos's options); --smoothing is
ivector-copy-plda's; --num-utts is the `ark,t:` int table `key count` that stage 2 of run_extract_embeddings.sh writes beside
the speaker means (an enrolment key without an entry counts as 1; how many is reported on stderr).  Trials are lines
`key1 key2 [target|nontarget]`, key1 from the enrolment table, key2 from the test table; the output lines are `key1 key2
score` in trial order.  A trial whose key is missing is skipped and counted on stderr; the exit status is non-zero only if
no trial was scored.  --eer and --min-dcf need the third column and print `EER: x%` and `minDCF(p-target=P): x` of the
scores as written (sid/compute_min_dcf.py; exact, from the sorted scores, on the host).  Kaldi is absent from the reference
tree: **parity unpinned**.  --cohort and its options are score_cos's (score normalisation, snorm.py): the cohort goes through
the same front, then through prepare_test for the statistics of the enrolment rows and through prepare_enroll (num_utts 1) for
those of the test rows; the scores written and --eer / --min-dcf are then the normalised ones.  Training the model (ivector-compute-lda / -plda) is compute_lda.py / compute_plda.py; ivector-adapt-plda stays with Kaldi."""
import argparse
import sys

import numpy as np

from . import kaldi_io
from . import plda
from . import scoring
from .score_cos import _bool, _table, add_snorm_options, check_snorm_options, normalise_scores, select_trials, write_scores


def _min_dcf_arg(s):
    try:
        v = [float(p) for p in s.split(",")]
    except ValueError:
        v = []
    if not 1 <= len(v) <= 3 or not 0.0 < v[0] < 1.0 or any(not c > 0.0 for c in v[1:]):
        raise argparse.ArgumentTypeError("expected P_TARGET[,C_MISS[,C_FA]] with 0 < P_TARGET < 1 and positive costs, got %r" % s)
    return tuple(v + [1.0] * (3 - len(v)))


def read_num_utts(rspecifier):
    """`ark,t:` int table (lines `key count`) -> dict."""
    path = rspecifier.split(":", 1)[1] if ":" in rspecifier.split("/")[0] else rspecifier
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if len(p) != 2 or not p[1].isdigit() or int(p[1]) < 1:
                raise ValueError("%s:%d: expected `key count` with count >= 1, got %r" % (path, no, line.rstrip("\n")))
            out[p[0]] = int(p[1])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="score_plda", description=__doc__.split("\n\n")[0])
    ap.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--normalize-length", type=_bool, default=True, help="ivector-plda-scoring --normalize-length; default true")
    ap.add_argument("--simple-length-normalization", type=_bool, default=False,
                    help="ivector-plda-scoring --simple-length-normalization; default false")
    ap.add_argument("--num-utts", default="", help="ark,t: int table of utterance counts per enrolment key (default: 1)")
    ap.add_argument("--smoothing", type=float, default=0.0, help="ivector-copy-plda --smoothing; default 0.0")
    ap.add_argument("--mean", default="", help="Kaldi vector subtracted from every x-vector (ivector-subtract-global-mean)")
    ap.add_argument("--transform", default="", help="Kaldi matrix applied after the mean (transform-vec; the LDA matrix)")
    ap.add_argument("--front-normalize", type=_bool, default=True, help="ivector-normalize-length behind the transform; default true")
    ap.add_argument("--eer", action="store_true", help="print the exact EER of the scored trials (needs labelled trials)")
    ap.add_argument("--min-dcf", type=_min_dcf_arg, action="append", default=[], metavar="P_TARGET[,C_MISS[,C_FA]]",
                    help="print the minimum normalised DCF of the scored trials; may be given more than once")
    add_snorm_options(ap)
    ap.add_argument("plda")
    ap.add_argument("enroll_rspecifier")
    ap.add_argument("test_rspecifier")
    ap.add_argument("trials")
    ap.add_argument("scores_out")
    args = ap.parse_args(argv)
    if not 0.0 <= args.smoothing <= 1.0:
        ap.error("--smoothing must be in [0, 1]")
    check_snorm_options(ap, args)

    keys1, keys2, targets = scoring.read_trials(args.trials)
    if (args.eer or args.min_dcf) and targets is None:
        sys.stderr.write("score_plda: --eer / --min-dcf need trials with a target / nontarget column\n")
        return 2
    model = plda.smooth(plda.read_plda(args.plda), args.smoothing)
    mean = np.asarray(kaldi_io.read_vec_flt(args.mean), dtype=np.float32) if args.mean else None
    transform = np.asarray(kaldi_io.read_mat(args.transform), dtype=np.float32) if args.transform else None
    counts = read_num_utts(args.num_utts) if args.num_utts else None
    row1, x1 = _table(args.enroll_rspecifier, mean, transform, args.front_normalize, args.gpu)
    row2, x2 = _table(args.test_rspecifier, mean, transform, args.front_normalize, args.gpu)
    kept = select_trials("score_plda", keys1, keys2, row1, row2)
    if kept is None:
        return 1
    num_utts = None
    if counts is not None:
        num_utts = np.ones(len(row1), np.int64)
        for k, i in row1.items():
            num_utts[i] = counts.get(k, 1)
        absent = sum(1 for k in row1 if k not in counts)
        if absent:
            sys.stderr.write("score_plda: %d of %d enrolment keys have no --num-utts entry (counted as 1)\n" % (absent, len(row1)))
    norm = dict(normalize_length=args.normalize_length, simple_length_norm=args.simple_length_normalization, device=args.gpu)
    enroll = plda.prepare_enroll(model, x1, num_utts=num_utts, **norm)
    test = plda.prepare_test(model, x2, **norm)
    ia = np.fromiter((row1[keys1[t]] for t in kept), dtype=np.int64, count=len(kept))
    ib = np.fromiter((row2[keys2[t]] for t in kept), dtype=np.int64, count=len(kept))
    scores = plda.llr_pairs(enroll, test, ia, ib)
    if args.cohort:
        from . import snorm
        rowc, xc = _table(args.cohort, mean, transform, args.front_normalize, args.gpu)
        if not rowc:
            sys.stderr.write("score_plda: the cohort table is empty\n")
            return 1

        def stats(side, labels, cohort_labels):
            if side == "enroll":
                return snorm.plda_cohort_stats(enroll, plda.prepare_test(model, xc, **norm), per="enroll", top_k=args.top_k,
                                               labels=labels, cohort_labels=cohort_labels)
            return snorm.plda_cohort_stats(plda.prepare_enroll(model, xc, **norm), test, per="test", top_k=args.top_k,
                                           labels=labels, cohort_labels=cohort_labels)
        scores = normalise_scores("score_plda", args, scores, ia, ib, row1, row2, rowc, stats)
        if scores is None:
            return 1
    printed = write_scores("score_plda", args.scores_out, keys1, keys2, kept, scores)
    labels = [targets[t] for t in kept] if targets is not None else None
    if args.eer:
        print("EER: %.4g%%" % (100.0 * scoring.exact_eer(printed, labels)))
    for p_target, c_miss, c_fa in args.min_dcf:
        print("minDCF(p-target=%g): %.4f" % (p_target, scoring.min_dcf(printed, labels, p_target, c_miss, c_fa)[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
