#!/bin/bash
# Validation of a checkpoint on one MI355X: stands in for what egs/voxceleb/v1/nnet/lib/train.py:106-155 does after every epoch
# (trainer.build("valid"); trainer.valid(...); compute_cos_pairwise_eer; one line appended to nnet/valid_loss).

gpuid=0
checkpoint=
precision=
eer=true
append=false

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
  echo "Usage: $0 [options] <nnet-dir> <valid-data-dir> <valid-spklist>"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --checkpoint <model-N>   # default: the one <nnet-dir>/nnet/checkpoint names"
  echo "  --precision <f32|bf16x3|f16x3|f16f6>"
  echo "  --eer <true>"
  echo "  --append <false>         # append 'step loss eer' to <nnet-dir>/nnet/valid_loss"
  echo ""
  exit 100
fi

opts=
if [ -n "$checkpoint" ]; then opts="$opts --checkpoint $checkpoint"; fi
if [ -n "$precision" ]; then opts="$opts --precision $precision"; fi
if ! $eer; then opts="$opts --no-eer"; fi
if $append; then opts="$opts --append"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.valid --gpu $gpuid $opts "$1" "$2" "$3"
