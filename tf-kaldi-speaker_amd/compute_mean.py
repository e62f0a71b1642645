"""The global mean of a table of x-vectors: Kaldi's `ivector-mean` in its two-argument form, the first back-end step of the
recipes (egs/voxceleb/v1/run.sh:385-387), without the Kaldi binary.

    python -m tf_kaldi_speaker_amd.compute_mean <vector-rspecifier> <mean-out>

The sum is taken in double and written as a binary Kaldi float vector, what `--mean` of score_cos / score_plda /
compute_lda / compute_plda reads.  Host only: one pass over the table.  **Parity unpinned** (Kaldi is absent from the
reference tree)."""
import argparse
import sys

from . import backend
from . import kaldi_io
from . import postprocess
from .score_cos import _rspec


def main(argv=None):
    ap = argparse.ArgumentParser(prog="compute_mean", description=__doc__.split("\n\n")[0])
    ap.add_argument("vector_rspecifier")
    ap.add_argument("mean_out")
    args = ap.parse_args(argv)
    keys, x = postprocess.read_vectors(_rspec(args.vector_rspecifier))
    if not keys:
        sys.stderr.write("compute_mean: no vector in %s\n" % args.vector_rspecifier)
        return 1
    kaldi_io.write_vec_flt(args.mean_out, backend.global_mean(x))
    sys.stderr.write("compute_mean: mean of %d vectors of dimension %d\n" % (x.shape[0], x.shape[1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
