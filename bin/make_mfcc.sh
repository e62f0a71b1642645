#!/bin/bash
# MFCC features and energy VAD of a data directory on one MI355X: stands in for the pair
#   steps/make_mfcc.sh --mfcc-config conf/mfcc.conf ... data/x        (compute-mfcc-feats)
#   sid/compute_vad_decision.sh ... data/x                            (compute-vad-decision)
# of egs/voxceleb/v1/run.sh:57-65.  Reads data/x/wav.scp; writes feats.scp, vad.scp and utt2num_frames into data/x and
# the arks into <feat-dir> (default data/x/data).

gpuid=0
mfcc_config=
vad_config=
channel=-1

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
  echo "Usage: $0 [options] <data-dir> [<feat-dir>]"
  echo "Options:"
  echo "  --gpuid <0>"
  echo "  --mfcc-config <conf/mfcc.conf>"
  echo "  --vad-config <conf/vad.conf>"
  echo "  --channel <-1>"
  echo ""
  exit 100
fi

data=$1
featdir=${2:-$data/data}
[ -f $data/wav.scp ] || { echo "$0: no such file $data/wav.scp"; exit 1; }
mkdir -p $featdir || exit 1
featdir=$(cd $featdir && pwd)
name=$(basename $data)

mopts=
vopts=
if [ -n "$mfcc_config" ]; then mopts="--config $mfcc_config"; fi
if [ -n "$vad_config" ]; then vopts="--config $vad_config"; fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.compute_mfcc --gpu $gpuid $mopts --channel $channel \
  --write-utt2num-frames $data/utt2num_frames scp:$data/wav.scp \
  ark,scp:$featdir/raw_mfcc_$name.ark,$data/feats.scp || exit 1
python -m tf_kaldi_speaker_amd.compute_vad --gpu $gpuid $vopts scp:$data/feats.scp \
  ark,scp:$featdir/vad_$name.ark,$data/vad.scp || exit 1
echo "$0: wrote $data/feats.scp, $data/vad.scp and $data/utt2num_frames"
