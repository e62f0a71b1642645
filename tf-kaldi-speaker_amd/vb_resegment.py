"""VB-HMM resegmentation of a first clustering on the GPU (vbx.py; xv_vbx, csrc/vbx.hip): the "VBx" step that x-vector
diarization recipes run after agglomerative clustering.  The reference has no such step: **parity unpinned**;
include/xvec_hip.h states the rule.

    python -m tf_kaldi_speaker_amd.vb_resegment [--gpu 0] --plda plda [--smoothing 0.0] [--mean mean.vec]
           [--transform transform.mat] [--normalize true] [--lda-dim K] [--fa 0.3] [--fb 17] [--loop-prob 0.99]
           [--init-smoothing 5] [--max-iters 40] [--epsilon 1e-6] [--segments FILE [--rttm-out FILE]]
           <utt2reco> <xvector-rspecifier> <init-labels> <labels-out>

<utt2reco> holds lines `key recording`; every key of the x-vector table needs one.  <init-labels> is the `key label` file
that `cluster` writes (any integer labels); every key of the table needs one.  The table goes through the front of
score_cos (--mean, --transform, --normalize) and then through the affine of the Plda (--smoothing as ivector-copy-plda;
--lda-dim keeps its first K dimensions); no length normalisation happens behind the Plda.  A recording's rows must be in
time order: with --segments (lines `key recording start end`) they are ordered by (start, end, key), otherwise they stay
in archive order.  <labels-out> ('-': stdout) gets `key label` lines in the order of the table, labels from 1 per
recording, the surviving speakers numbered by their first row in time; with --rttm-out the labels are also written as RTTM
(cluster.rttm_lines).  stdout gets one summary line, `R recordings, N segments, B -> A speakers`."""
import argparse
import sys

import numpy as np


def read_labels(path):
    """Lines `key label` with an integer label -> dict."""
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            try:
                if len(p) != 2:
                    raise ValueError
                out[p[0]] = int(p[1])
            except ValueError:
                raise ValueError("%s:%d: expected `key label` with an integer label, got %r" % (path, no, line.rstrip("\n")))
    return out


def time_order(keys, segments):
    """The permutation that sorts the table by (start, end, key) of `segments` (cluster.read_segments); keys are unique per
    table, so the order inside every recording is total.  A key without a segment is a ValueError."""
    times = {key: (start, end) for key, _, start, end in segments}
    missing = [k for k in keys if k not in times]
    if missing:
        raise ValueError("%d keys have no segment (first: %s)" % (len(missing), missing[0]))
    return np.array(sorted(range(len(keys)), key=lambda i: times[keys[i]] + (keys[i],)), dtype=np.int64)


def parse_args(argv=None):
    from .score_cos import _bool
    ap = argparse.ArgumentParser(prog="vb_resegment", description=__doc__.split("\n\n")[0])
    ap.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--plda", default="", help="Kaldi Plda: the speaker model (required)")
    ap.add_argument("--smoothing", type=float, default=0.0, help="ivector-copy-plda --smoothing; default 0.0")
    ap.add_argument("--mean", default="", help="Kaldi vector subtracted from every x-vector (ivector-subtract-global-mean)")
    ap.add_argument("--transform", default="", help="Kaldi matrix applied after the mean (transform-vec; [d_out, d] or [d_out, d + 1])")
    ap.add_argument("--normalize", type=_bool, default=True, help="length-normalise last, before the Plda; default true")
    ap.add_argument("--lda-dim", type=int, default=None, help="keep the first K dimensions of the Plda space; default: all")
    ap.add_argument("--fa", type=float, default=0.3, help="scale of the acoustic statistics; default 0.3")
    ap.add_argument("--fb", type=float, default=17.0, help="scale of the speaker prior; default 17")
    ap.add_argument("--loop-prob", type=float, default=0.99, help="probability of staying with the speaker; default 0.99")
    ap.add_argument("--init-smoothing", type=float, default=5.0, help="gamma starts as softmax(this * onehot(label)); default 5")
    ap.add_argument("--max-iters", type=int, default=40, help="at most this many iterations; default 40")
    ap.add_argument("--epsilon", type=float, default=1e-6, help="stop when the ELBO improves by less; default 1e-6 (--epsilon=-inf: run all --max-iters)")
    ap.add_argument("--segments", default="", help="`key recording start end` lines: order every recording's rows in time")
    ap.add_argument("--rttm-out", default="", help="RTTM file to write; needs --segments")
    ap.add_argument("utt2reco")
    ap.add_argument("xvector_rspecifier")
    ap.add_argument("init_labels")
    ap.add_argument("labels_out")
    args = ap.parse_args(argv)
    if not args.plda:
        ap.error("--plda is required")
    if not 0.0 <= args.smoothing <= 1.0:
        ap.error("--smoothing must be in [0, 1]")
    if not (0.0 < args.fa < float("inf") and 0.0 < args.fb < float("inf")):
        ap.error("--fa and --fb must be positive")
    if not 0.0 <= args.loop_prob <= 1.0:
        ap.error("--loop-prob must be in [0, 1]")
    if not 0.0 <= args.init_smoothing < float("inf"):
        ap.error("--init-smoothing must be >= 0")
    if args.max_iters < 1:
        ap.error("--max-iters must be >= 1")
    if args.epsilon != args.epsilon:
        ap.error("--epsilon is NaN")
    if args.lda_dim is not None and args.lda_dim < 1:
        ap.error("--lda-dim must be >= 1")
    if args.rttm_out and not args.segments:
        ap.error("--rttm-out needs --segments")
    return args


def main(argv=None):
    args = parse_args(argv)
    from . import cluster
    from . import kaldi_io
    from . import plda as plda_mod
    from . import postprocess
    from . import vbx
    from .score_cos import _rspec, read_utt2spk
    utt2reco = read_utt2spk(args.utt2reco)
    keys, x = postprocess.read_vectors(_rspec(args.xvector_rspecifier))
    if not keys:
        sys.stderr.write("vb_resegment: the x-vector table is empty\n")
        return 1
    try:
        init = read_labels(args.init_labels)
        for what, table in ((args.utt2reco, utt2reco), (args.init_labels, init)):
            missing = [k for k in keys if k not in table]
            if missing:
                raise ValueError("%d keys have no entry in %s (first: %s)" % (len(missing), what, missing[0]))
        segments = cluster.read_segments(args.segments) if args.segments else None
        order = time_order(keys, segments) if segments is not None else np.arange(len(keys))
        recos = np.array([utt2reco[k] for k in keys], dtype=object).astype(str)
        labels_in = np.array([init[k] for k in keys], dtype=np.int64)
        mean = np.asarray(kaldi_io.read_vec_flt(args.mean), dtype=np.float32) if args.mean else None
        transform = np.asarray(kaldi_io.read_mat(args.transform), dtype=np.float32) if args.transform else None
        model = plda_mod.smooth(plda_mod.read_plda(args.plda), args.smoothing)
        sorted_labels, per = vbx.resegment(model, np.asarray(x)[order], recos[order], labels_in[order], fa=args.fa, fb=args.fb,
                                           loop_prob=args.loop_prob, init_smoothing=args.init_smoothing, max_iters=args.max_iters,
                                           epsilon=args.epsilon, lda_dim=args.lda_dim, mean=mean, transform=transform,
                                           normalize=args.normalize, device=args.gpu)
    except ValueError as e:
        sys.stderr.write("vb_resegment: %s\n" % e)
        return 1
    labels = np.zeros(len(keys), np.int32)
    labels[order] = sorted_labels
    text = cluster.format_labels(keys, labels)
    if args.labels_out == "-":
        sys.stdout.write(text)
    else:
        with open(args.labels_out, "w") as f:
            f.write(text)
    if args.rttm_out:
        with open(args.rttm_out, "w") as f:
            f.write(cluster.rttm_lines(segments, {k: int(l) + 1 for k, l in zip(keys, labels)}))
    before = sum(len(set(labels_in[recos == name].tolist())) for name in per)
    print("%d recordings, %d segments, %d -> %d speakers" % (len(per), len(keys), before, sum(r.num_speakers for r in per.values())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
