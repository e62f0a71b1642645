#!/bin/bash
# Back-end training on one MI355X: stands in for the three Kaldi steps of egs/voxceleb/v1/run.sh:384-400
# (ivector-mean, ivector-compute-lda behind ivector-subtract-global-mean, ivector-compute-plda behind
# ivector-subtract-global-mean | transform-vec | ivector-normalize-length), in recipe order.  Reads <xvector-dir>/xvector.scp and
# <data-dir>/{utt2spk,spk2utt}; writes mean.vec, transform.mat and plda into <xvector-dir>, the files bin/score_cos.sh
# (--mean / --transform) and bin/score_plda.sh read.

gpuid=0
lda_dim=200
total_covariance_factor=0.0
num_em_iters=10

if [ -f path.sh ]; then . ./path.sh; fi
if [ -f parse_options.sh ] || command -v parse_options.sh >/dev/null 2>&1; then
  . parse_options.sh || exit 1;
else
  # minimal --name value parser when Kaldi's utils/parse_options.sh is not on PATH
  while [ $# -gt 0 ]; do
    case "$1" in
      --*) name=$(echo "${1#--}" | tr '-' '_'); eval "$name=\"$2\""; shift 2 ;;
      *) break ;;
    esac
  done
fi

if [ $# != 2 ]; then
  echo "Usage: $0 [options] <data-dir> <xvector-dir>"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --lda-dim <200>"
  echo "  --total-covariance-factor <0.0>"
  echo "  --num-em-iters <10>"
  echo ""
  exit 100
fi

data=$1
dir=$2

for f in $data/utt2spk $data/spk2utt $dir/xvector.scp; do
  [ ! -f $f ] && echo "No such file $f" && exit 1;
done

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.compute_mean scp:$dir/xvector.scp $dir/mean.vec || exit 1

python -m tf_kaldi_speaker_amd.compute_lda --gpu $gpuid --dim $lda_dim --total-covariance-factor $total_covariance_factor \
  --mean $dir/mean.vec scp:$dir/xvector.scp ark:$data/utt2spk $dir/transform.mat || exit 1

python -m tf_kaldi_speaker_amd.compute_plda --gpu $gpuid --num-em-iters $num_em_iters --mean $dir/mean.vec \
  --transform $dir/transform.mat --normalize-length ark:$data/spk2utt scp:$dir/xvector.scp $dir/plda || exit 1
