"""A PLDA model of a labelled table of x-vectors on the GPU: Kaldi's `ivector-compute-plda`, the last back-end training step
of the recipes (egs/voxceleb/v1/run.sh:396-400, egs/sre/v1/run.sh:406-411), without the Kaldi binary.

    ivector-compute-plda ark:spk2utt "ark:ivector-subtract-global-mean scp:xvector.scp ark:- | transform-vec transform.mat
        ark:- ark:- | ivector-normalize-length ark:- ark:- |" plda

    python -m tf_kaldi_speaker_amd.compute_plda [--gpu 0] [--num-em-iters 10] [--binary true] [--mean mean.vec]
           [--transform transform.mat] [--normalize-length] <spk2utt-rspecifier> <vector-rspecifier> <plda-out>

--mean, --transform and --normalize-length are the in-pipe steps of the vector rspecifier, as in compute_lda.  An utterance of
spk2utt without a vector is skipped and counted on stderr; a speaker with none is left out.  The output is a Kaldi `Plda`
file (plda.write_plda), what score_plda reads.  `ivector-adapt-plda` (sre only) stays with Kaldi.  **Parity unpinned**."""
import argparse
import sys

import numpy as np

from . import backend
from . import plda
from . import postprocess
from .compute_lda import add_front_options, read_front
from .score_cos import _bool


def main(argv=None):
    ap = argparse.ArgumentParser(prog="compute_plda", description=__doc__.split("\n\n")[0])
    add_front_options(ap)
    ap.add_argument("--num-em-iters", type=int, default=10, help="EM iterations (ivector-compute-plda --num-em-iters); default 10")
    ap.add_argument("--binary", type=_bool, default=True, help="write the model in binary mode; default true")
    ap.add_argument("spk2utt_rspecifier")
    ap.add_argument("vector_rspecifier")
    ap.add_argument("plda_out")
    args = ap.parse_args(argv)
    if args.num_em_iters < 0:
        ap.error("--num-em-iters must be >= 0")

    spk2utt = postprocess.read_spk2utt(backend.table_path(args.spk2utt_rspecifier))
    keys, rows = read_front(args)
    row = {k: i for i, k in enumerate(keys)}
    lists, listed, missing = [], 0, 0
    for _, utts in spk2utt:
        have = [row[u] for u in utts if u in row]
        listed += len(utts)
        missing += len(utts) - len(have)
        if have:
            lists.append(have)
    if missing:
        sys.stderr.write("compute_plda: skipped %d of %d utterances of spk2utt (no vector)\n" % (missing, listed))
    if not lists:
        sys.stderr.write("compute_plda: no speaker with a vector\n")
        return 1
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in lists])])
    try:
        stats = backend.scatter_stats(rows, (offsets, np.concatenate(lists)), device=args.gpu)
        model = backend.plda_from_stats(stats, args.num_em_iters)
    except ValueError as e:
        sys.stderr.write("compute_plda: %s\n" % e)
        return 1
    plda.write_plda(args.plda_out, model, binary=args.binary)
    sys.stderr.write("compute_plda: %d vectors of %d speakers, dimension %d, %d EM iterations\n"
                     % (stats.n, stats.num_classes, stats.dim, args.num_em_iters))
    return 0


if __name__ == "__main__":
    sys.exit(main())
