#!/bin/bash
# Cosine scoring of a trial list on one MI355X: stands in for the Kaldi pipeline of egs/voxceleb/v1/run.sh:362-365
# (ivector-normalize-length | ivector-compute-dot-products) and, with --mean / --transform, of :404-408
# (ivector-subtract-global-mean | transform-vec | ivector-normalize-length | ivector-compute-dot-products).

gpuid=0
mean=
transform=
normalize=true
eer=false

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
  echo ""
  exit 100
fi

opts=
if [ -n "$mean" ]; then opts="$opts --mean $mean"; fi
if [ -n "$transform" ]; then opts="$opts --transform $transform"; fi
if $eer; then opts="$opts --eer"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.score_cos --gpu $gpuid --normalize $normalize $opts "$1" "$2" "$3" "$4"
