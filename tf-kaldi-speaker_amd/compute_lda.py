"""The LDA transform of a labelled table of x-vectors on the GPU: Kaldi's `ivector-compute-lda`, the second back-end step of
the recipes (egs/voxceleb/v1/run.sh:389-394, egs/sre/v1/run.sh:399-404), without the Kaldi binary.

    ivector-compute-lda --total-covariance-factor=0.0 --dim=$lda_dim "ark:ivector-subtract-global-mean scp:xvector.scp ark:- |"
        ark:utt2spk transform.mat

    python -m tf_kaldi_speaker_amd.compute_lda [--gpu 0] [--dim 100] [--total-covariance-factor 0.0] [--covariance-floor 1e-6]
           [--mean mean.vec] [--transform t.mat] [--normalize-length] <vector-rspecifier> <utt2spk-rspecifier> <lda-out>

--mean, --transform and --normalize-length are the in-pipe steps of the vector rspecifier (ivector-subtract-global-mean |
transform-vec | ivector-normalize-length), applied on the device in this order.  A vector whose key has no utt2spk entry is
skipped and counted on stderr.  The output is a binary Kaldi float matrix [dim, d + 1], the last column the offset
`transform-vec` adds: what --transform of score_cos / score_plda / compute_plda reads.  **Parity unpinned**."""
import argparse
import sys

import numpy as np

from . import backend
from . import kaldi_io
from . import postprocess
from .score_cos import _rspec


def add_front_options(ap):
    ap.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--mean", default="", help="Kaldi vector subtracted from every x-vector first (ivector-subtract-global-mean)")
    ap.add_argument("--transform", default="", help="Kaldi matrix applied after the mean (transform-vec; [d_out, d] or [d_out, d + 1])")
    ap.add_argument("--normalize-length", action="store_true",
                    help="length-normalise last, as ivector-normalize-length does by default (--scaleup=true): every row gets the "
                         "norm sqrt(dim), not 1.  This sets the scale of the mean / transform in the file written, not the scores")


def read_front(args):
    """-> (keys, rows on the device behind the in-pipe steps), or (keys, None) for an empty table."""
    keys, x = postprocess.read_vectors(_rspec(args.vector_rspecifier))
    if not keys:
        return keys, None
    mean = np.asarray(kaldi_io.read_vec_flt(args.mean), dtype=np.float32) if args.mean else None
    transform = np.asarray(kaldi_io.read_mat(args.transform), dtype=np.float32) if args.transform else None
    return keys, backend.front(x, mean, transform, args.normalize_length, args.gpu)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="compute_lda", description=__doc__.split("\n\n")[0])
    add_front_options(ap)
    ap.add_argument("--dim", type=int, default=100, help="rows of the transform (ivector-compute-lda --dim); default 100")
    ap.add_argument("--total-covariance-factor", type=float, default=0.0,
                    help="share of the total covariance in the matrix that is whitened; default 0.0")
    ap.add_argument("--covariance-floor", type=float, default=1e-6, help="eigenvalue floor of that matrix, relative to its largest; default 1e-6")
    ap.add_argument("vector_rspecifier")
    ap.add_argument("utt2spk_rspecifier")
    ap.add_argument("lda_out")
    args = ap.parse_args(argv)

    utt2spk = backend.read_utt2spk(backend.table_path(args.utt2spk_rspecifier))
    keys, rows = read_front(args)
    by_spk, missing = {}, 0
    for i, k in enumerate(keys):
        if k in utt2spk:
            by_spk.setdefault(utt2spk[k], []).append(i)
        else:
            missing += 1
    if missing:
        sys.stderr.write("compute_lda: skipped %d of %d vectors (no utt2spk entry)\n" % (missing, len(keys)))
    if not by_spk:
        sys.stderr.write("compute_lda: no labelled vector\n")
        return 1
    lists = list(by_spk.values())
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in lists])])
    try:
        stats = backend.scatter_stats(rows, (offsets, np.concatenate(lists)), device=args.gpu)
        lda = backend.lda_from_stats(stats, args.dim, args.total_covariance_factor, args.covariance_floor)
    except ValueError as e:
        sys.stderr.write("compute_lda: %s\n" % e)
        return 1
    kaldi_io.write_mat(args.lda_out, lda)
    sys.stderr.write("compute_lda: %d vectors of %d speakers, dimension %d -> %d\n" % (stats.n, stats.num_classes, stats.dim, lda.shape[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
