#!/bin/bash
# Score calibration and fusion on one MI355X: logistic-regression calibration of Kaldi-style score files, which the reference
# recipes leave to outside tools (their only fusion is misc/utils/average_score.py, an equal-weight mean of two score files).
#   calibrate.sh train [--prior 0.01] [--gpu 0] <trials> <model-out> <scores1> [<scores2> ...]
#   calibrate.sh apply [--gpu 0] <model> <llr-out> <scores1> [<scores2> ...]
#   calibrate.sh eval  [--gpu 0] [--p-target P[,C_MISS[,C_FA]]]... <trials> <scores>

if [ -f path.sh ]; then . ./path.sh; fi

if [ $# -lt 3 ]; then
  sed -n '2,6p' "$0"
  exit 100
fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.calibrate "$@"
