#!/bin/bash
# PLDA scoring of a trial list on one MI355X with a trained Kaldi Plda: stands in for the Kaldi pipeline of
# egs/voxceleb/v1/run.sh:410-426 (ivector-plda-scoring --normalize-length=true "ivector-copy-plda --smoothing=0.0 plda - |"
# behind ivector-subtract-global-mean | transform-vec | ivector-normalize-length on both sides).  Argument order as
# ivector-plda-scoring: <plda> <enroll> <test> <trials> <scores-out>.

gpuid=0
mean=
transform=
front_normalize=true
normalize_length=true
simple_length_normalization=false
num_utts=
smoothing=0.0
eer=false
min_dcf=
cohort=
norm=
top_k=
exclude_utt2spk=

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

if [ $# != 5 ]; then
  echo "Usage: $0 [options] <plda> <enroll-rspecifier> <test-rspecifier> <trials> <scores-out>"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --mean <mean.vec>"
  echo "  --transform <transform.mat>"
  echo "  --front-normalize <true>"
  echo "  --normalize-length <true>"
  echo "  --simple-length-normalization <false>"
  echo "  --num-utts <ark:num_utts.ark>"
  echo "  --smoothing <0.0>"
  echo "  --eer <false>"
  echo "  --min-dcf <p_target[,c_miss[,c_fa]]>"
  echo "  --cohort <cohort-rspecifier>        # score normalisation; the three below need it"
  echo "  --norm <s>                          # z, t or s"
  echo "  --top-k <0>                         # adaptive cohort size; 0: the whole cohort"
  echo "  --exclude-utt2spk <utt2spk>"
  echo ""
  exit 100
fi

opts=
if [ -n "$mean" ]; then opts="$opts --mean $mean"; fi
if [ -n "$transform" ]; then opts="$opts --transform $transform"; fi
if [ -n "$num_utts" ]; then opts="$opts --num-utts $num_utts"; fi
if [ -n "$min_dcf" ]; then opts="$opts --min-dcf $min_dcf"; fi
if $eer; then opts="$opts --eer"; fi
if [ -n "$cohort" ]; then opts="$opts --cohort $cohort"; fi
if [ -n "$norm" ]; then opts="$opts --norm $norm"; fi
if [ -n "$top_k" ]; then opts="$opts --top-k $top_k"; fi
if [ -n "$exclude_utt2spk" ]; then opts="$opts --exclude-utt2spk $exclude_utt2spk"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.score_plda --gpu $gpuid --front-normalize $front_normalize --normalize-length $normalize_length \
  --simple-length-normalization $simple_length_normalization --smoothing $smoothing $opts "$1" "$2" "$3" "$4" "$5"
