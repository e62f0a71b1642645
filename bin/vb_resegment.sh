#!/bin/bash
# VB-HMM resegmentation ("VBx") of a first clustering on one MI355X: the labels of bin/cluster.sh initialise a Bayesian HMM
# over the x-vector sequence of every recording, with the speakers modelled in the space of a Kaldi Plda.  The reference has no
# such step; tf-kaldi-speaker_amd/vbx.py states what is computed.

gpuid=0
plda=
smoothing=
mean=
transform=
normalize=true
lda_dim=
fa=
fb=
loop_prob=
init_smoothing=
max_iters=
epsilon=
segments=
rttm_out=

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

if [ $# != 4 ] || [ -z "$plda" ]; then
  echo "Usage: $0 --plda <plda> [options] <utt2reco> <xvector-rspecifier> <init-labels> <labels-out>"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --plda <plda>                       # the speaker model (required)"
  echo "  --smoothing <0.0>"
  echo "  --mean <mean.vec>"
  echo "  --transform <transform.mat>"
  echo "  --normalize <true>"
  echo "  --lda-dim <K>                       # keep the first K dimensions of the Plda space"
  echo "  --fa <0.3>  --fb <17>  --loop-prob <0.99>  --init-smoothing <5>  --max-iters <40>  --epsilon <1e-6>"
  echo "  --segments <segments>               # key recording start end: order every recording's rows in time"
  echo "  --rttm-out <rttm>                   # needs --segments"
  echo ""
  exit 100
fi

opts="--plda $plda"
if [ -n "$smoothing" ]; then opts="$opts --smoothing $smoothing"; fi
if [ -n "$mean" ]; then opts="$opts --mean $mean"; fi
if [ -n "$transform" ]; then opts="$opts --transform $transform"; fi
if [ -n "$lda_dim" ]; then opts="$opts --lda-dim $lda_dim"; fi
if [ -n "$fa" ]; then opts="$opts --fa $fa"; fi
if [ -n "$fb" ]; then opts="$opts --fb $fb"; fi
if [ -n "$loop_prob" ]; then opts="$opts --loop-prob $loop_prob"; fi
if [ -n "$init_smoothing" ]; then opts="$opts --init-smoothing $init_smoothing"; fi
if [ -n "$max_iters" ]; then opts="$opts --max-iters $max_iters"; fi
if [ -n "$epsilon" ]; then opts="$opts --epsilon=$epsilon"; fi
if [ -n "$segments" ]; then opts="$opts --segments $segments"; fi
if [ -n "$rttm_out" ]; then opts="$opts --rttm-out $rttm_out"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.vb_resegment --gpu $gpuid --normalize $normalize $opts "$1" "$2" "$3" "$4"
