#!/bin/bash
# Train a network from scratch on one MI355X: nnet/run_train_nnet.sh -> nnet/lib/train.py, with its positional arguments.

gpuid=0
continue_training=false
seed=
prefetch=
batch_norm=
precision=

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

if [ $# != 6 ]; then
  echo "Usage: $0 [options] <config> <train-data-dir> <train-spklist> <valid-data-dir> <valid-spklist> <nnet-dir>"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --continue-training <false>  # go on from the last checkpoint of <nnet-dir> and its optimizer file"
  echo "  --seed <N>                   # of the initial values and the batches; default: params.seed or 0"
  echo "  --prefetch <2>               # batches staged and decoded ahead of the step; 0: inline"
  echo "  --batch-norm <batch>         # batch: the statistics of the batch (the reference's training mode); moving: constant"
  echo "  --precision <f32|bf16x3|f16x3|f16f6>   # of the validation forward"
  echo ""
  exit 100
fi

opts=
if $continue_training; then opts="$opts -c"; fi
if [ -n "$seed" ]; then opts="$opts --seed $seed"; fi
if [ -n "$prefetch" ]; then opts="$opts --prefetch $prefetch"; fi
if [ -n "$batch_norm" ]; then opts="$opts --batch-norm $batch_norm"; fi
if [ -n "$precision" ]; then opts="$opts --precision $precision"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.train --gpu $gpuid $opts --config "$1" "$2" "$3" "$4" "$5" "$6"
