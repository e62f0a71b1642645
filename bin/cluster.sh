#!/bin/bash
# Speaker clustering on one MI355X: average-linkage agglomerative clustering of the sub-segment x-vectors of every recording,
# by cosine or (with --plda) by PLDA log likelihood ratio, behind the front of bin/score_cos.sh (--mean / --transform /
# --normalize): the step of Kaldi's diarization/cluster.sh.  The reference has no clustering step;
# tf-kaldi-speaker_amd/cluster.py states what is computed.

gpuid=0
threshold=
reco2num_spk=
mean=
transform=
normalize=true
plda=
smoothing=
target_energy=
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

if [ $# != 3 ]; then
  echo "Usage: $0 [options] <utt2reco> <xvector-rspecifier> <labels-out>"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --threshold <0.0>                   # stop when the best average linkage (a score) is below this"
  echo "  --reco2num-spk <reco2num_spk>       # instead of a threshold: clusters per recording"
  echo "  --mean <mean.vec>"
  echo "  --transform <transform.mat>"
  echo "  --normalize <true>"
  echo "  --plda <plda>                       # PLDA instead of cosine"
  echo "  --smoothing <0.0>                   # needs --plda"
  echo "  --target-energy <E>                 # needs --plda: per-recording PCA as ivector-plda-scoring-dense (Kaldi: 0.1)"
  echo "  --segments <segments>               # with --rttm-out: key recording start end"
  echo "  --rttm-out <rttm>"
  echo ""
  exit 100
fi

opts=
if [ -n "$threshold" ]; then opts="$opts --threshold $threshold"; fi
if [ -n "$reco2num_spk" ]; then opts="$opts --reco2num-spk $reco2num_spk"; fi
if [ -n "$mean" ]; then opts="$opts --mean $mean"; fi
if [ -n "$transform" ]; then opts="$opts --transform $transform"; fi
if [ -n "$plda" ]; then opts="$opts --plda $plda"; fi
if [ -n "$smoothing" ]; then opts="$opts --smoothing $smoothing"; fi
if [ -n "$target_energy" ]; then opts="$opts --target-energy $target_energy"; fi
if [ -n "$segments" ]; then opts="$opts --segments $segments"; fi
if [ -n "$rttm_out" ]; then opts="$opts --rttm-out $rttm_out"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.cluster --gpu $gpuid --normalize $normalize $opts "$1" "$2" "$3"
