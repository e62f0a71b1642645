#!/bin/bash
# Train a new classifier head on a frozen pre-trained encoder on one MI355X: stage one of
# egs/voxceleb/v1/nnet/lib/finetune.py ("train the new softmax first"), with its positional arguments.

gpuid=0
checkpoint=
config=
seed=
precision=
keep_head=false
segment_layers=false
frame_layers=false
conv_layers=false
batch_norm=

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
  echo "Usage: $0 [options] <pretrain-nnet-dir> <train-data-dir> <train-spklist> <valid-data-dir> <valid-spklist> <finetune-nnet-dir>"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --checkpoint <model-N>   # default: the one <pretrain-nnet-dir>/nnet/checkpoint names"
  echo "  --config <new.json>      # the configuration of the new model; default: the pre-trained one"
  echo "  --seed <N>               # default: params.seed or 0"
  echo "  --precision <f32|bf16x3|f16x3|f16f6>"
  echo "  --keep-head <false>      # start from the checkpoint's own softmax kernel when its shape fits"
  echo "  --segment-layers <false> # also train the two dense layers behind the pooling node (run the head alone first)"
  echo "  --frame-layers <false>   # also train the 1-tap frame layers in front of the pooling node; implies --segment-layers"
  echo "                           # (run the head alone first, then --segment-layers, then this)"
  echo "  --conv-layers <false>    # train every frame-level layer, the multi-tap convolutions included; implies the other two"
  echo "                           # (on a resnet_18 model: every 2-D convolution and block, conv5, dense1, dense2)"
  echo "                           # (the fourth run, after --frame-layers)"
  echo "  --batch-norm <moving>    # moving: inference-mode batch norm, the moving statistics stay constant; batch: the"
  echo "                           # statistics of the batch and moving-average updates in the trained layers (needs one of"
  echo "                           # --segment-layers, --frame-layers, --conv-layers)"
  echo ""
  exit 100
fi

opts=
if [ -n "$checkpoint" ]; then opts="$opts --checkpoint $checkpoint"; fi
if [ -n "$config" ]; then opts="$opts --config $config"; fi
if [ -n "$seed" ]; then opts="$opts --seed $seed"; fi
if [ -n "$precision" ]; then opts="$opts --precision $precision"; fi
if $keep_head; then opts="$opts --keep-head"; fi
if $segment_layers; then opts="$opts --segment-layers"; fi
if $frame_layers; then opts="$opts --frame-layers"; fi
if $conv_layers; then opts="$opts --conv-layers"; fi
if [ -n "$batch_norm" ]; then opts="$opts --batch-norm $batch_norm"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.train_head --gpu $gpuid $opts "$1" "$2" "$3" "$4" "$5" "$6"
