#!/bin/bash
# Log mel filterbank features of a data directory on one MI355X: stands in for
#   steps/make_fbank.sh --write-utt2num-frames true --fbank-config fbank.conf ... data/x      (compute-fbank-feats)
# of egs/voxceleb/v3/run.sh:54.  Reads data/x/wav.scp; writes feats.scp and utt2num_frames into data/x and the ark into
# <feat-dir> (default data/x/data).  An fbank file made with --use-energy=false has no energy column for
# sid/compute_vad_decision.sh to read (run.sh:58 copies the VAD of the MFCC version instead); with --vad-config the energy VAD
# is decided here, on the frame log energy the feature kernel computes on the way, and vad.scp is written too.

gpuid=0
fbank_config=
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
  echo "  --fbank-config <conf/fbank.conf>"
  echo "  --vad-config <conf/vad.conf>      # also write vad.scp, decided on the frame log energy"
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

fopts=
vopts=
wrote="$data/feats.scp and $data/utt2num_frames"
if [ -n "$fbank_config" ]; then fopts="--config $fbank_config"; fi
if [ -n "$vad_config" ]; then
  vopts="--vad-config $vad_config --vad-wspecifier ark,scp:$featdir/vad_$name.ark,$data/vad.scp"
  wrote="$data/feats.scp, $data/vad.scp and $data/utt2num_frames"
fi

here=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
export PYTHONPATH=$here:$PYTHONPATH

python -m tf_kaldi_speaker_amd.compute_fbank --gpu $gpuid $fopts $vopts --channel $channel \
  --write-utt2num-frames $data/utt2num_frames scp:$data/wav.scp \
  ark,scp:$featdir/raw_fbank_$name.ark,$data/feats.scp || exit 1
echo "$0: wrote $wrote"
