#!/bin/bash
# Resolve the augmented wav.scp of a data directory on one MI355X: every `wav-reverberate ... |` line written by
# steps/data/reverberate_data_dir.py / augment_data_dir.py (stage 2 of egs/sre/v1/run.sh and egs/voxceleb/v2/run_aug.sh)
# becomes a wav file under <wav-dir> (default data/x/wav), and data/x/wav.scp is rewritten to name those files (the
# original is kept as wav.scp.pipes).  No Kaldi binary runs.

gpuid=0
sample_frequency=0

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

if [ $# -lt 1 ] || [ $# -gt 2 ]; then
  echo "Usage: $0 [options] <data-dir> [<wav-dir>]"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --sample-frequency <0>     # refuse files of another rate (0: any)"
  echo ""
  exit 100
fi

data=$1
wavdir=${2:-$data/wav}
[ -f $data/wav.scp ] || { echo "$0: no such file $data/wav.scp"; exit 1; }
mkdir -p $wavdir || exit 1

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.augment_wav --gpu $gpuid --sample-frequency $sample_frequency \
  scp:$data/wav.scp $wavdir || exit 1
cp $data/wav.scp $data/wav.scp.pipes || exit 1
cp $wavdir/wav.scp $data/wav.scp || exit 1
echo "$0: wrote $(wc -l < $data/wav.scp) lines to $data/wav.scp (pipelines resolved into $wavdir)"
