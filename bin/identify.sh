#!/bin/bash
# Closed-set speaker identification on one MI355X: for every query x-vector the top-K entries of a gallery, by cosine or
# (with --plda) by PLDA log likelihood ratio, behind the front of bin/score_cos.sh (--mean / --transform / --normalize).
# The reference has no identification step; tf-kaldi-speaker_amd/identify.py states what is computed.

gpuid=0
top_k=10
mean=
transform=
normalize=true
plda=
num_utts=
smoothing=
exclude_utt2spk=
gallery_utt2spk=
query_utt2spk=
ranks=

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
  echo "Usage: $0 [options] <gallery-rspecifier> <query-rspecifier> <hits-out>"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --top-k <10>                        # hits per query, 1..1024"
  echo "  --mean <mean.vec>"
  echo "  --transform <transform.mat>"
  echo "  --normalize <true>"
  echo "  --plda <plda>                       # PLDA instead of cosine; the two below need it"
  echo "  --num-utts <ark:num_utts.ark>"
  echo "  --smoothing <0.0>"
  echo "  --exclude-utt2spk <utt2spk>"
  echo "  --gallery-utt2spk <utt2spk>         # with --query-utt2spk: print the identification rates"
  echo "  --query-utt2spk <utt2spk>"
  echo "  --ranks <1,5,10>"
  echo ""
  exit 100
fi

opts=
if [ -n "$mean" ]; then opts="$opts --mean $mean"; fi
if [ -n "$transform" ]; then opts="$opts --transform $transform"; fi
if [ -n "$plda" ]; then opts="$opts --plda $plda"; fi
if [ -n "$num_utts" ]; then opts="$opts --num-utts $num_utts"; fi
if [ -n "$smoothing" ]; then opts="$opts --smoothing $smoothing"; fi
if [ -n "$exclude_utt2spk" ]; then opts="$opts --exclude-utt2spk $exclude_utt2spk"; fi
if [ -n "$gallery_utt2spk" ]; then opts="$opts --gallery-utt2spk $gallery_utt2spk"; fi
if [ -n "$query_utt2spk" ]; then opts="$opts --query-utt2spk $query_utt2spk"; fi
if [ -n "$ranks" ]; then opts="$opts --ranks $ranks"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.identify --gpu $gpuid --top-k $top_k --normalize $normalize $opts "$1" "$2" "$3"
