#!/bin/bash
# Cosine scoring of a trial list on one MI355X: stands in for the Kaldi pipeline of egs/voxceleb/v1/run.sh:362-365
# (ivector-normalize-length | ivector-compute-dot-products) and, with --mean / --transform, of :404-408
# (ivector-subtract-global-mean | transform-vec | ivector-normalize-length | ivector-compute-dot-products).

gpuid=0
mean=
transform=
normalize=true
eer=false
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

if [ $# != 4 ]; then
  echo "Usage: $0 [options] <trials> <xvector-rspecifier-1> <xvector-rspecifier-2> <scores-out>"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --mean <mean.vec>"
  echo "  --transform <transform.mat>"
  echo "  --normalize <true>"
  echo "  --eer <false>"
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
if $eer; then opts="$opts --eer"; fi
if [ -n "$cohort" ]; then opts="$opts --cohort $cohort"; fi
if [ -n "$norm" ]; then opts="$opts --norm $norm"; fi
if [ -n "$top_k" ]; then opts="$opts --top-k $top_k"; fi
if [ -n "$exclude_utt2spk" ]; then opts="$opts --exclude-utt2spk $exclude_utt2spk"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.score_cos --gpu $gpuid --normalize $normalize $opts "$1" "$2" "$3" "$4"
