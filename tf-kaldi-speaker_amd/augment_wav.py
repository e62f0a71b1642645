"""Resolve the `wav-reverberate ... |` lines of a wav.scp on the GPU and write the waveforms out:

    python -m tf_kaldi_speaker_amd.augment_wav [-g GPU] [--sample-frequency F] [--batch-samples N] scp:wav.scp out_dir

writes out_dir/<key>.wav for every pipeline line and out_dir/wav.scp, in which those lines name the new files and every
other line is copied through.  The rule is that of tf_kaldi_speaker_amd.augment.  **parity unpinned**."""
import argparse
import logging
import os
import sys

from . import augment
from .mfcc import read_wav_scp

log = logging.getLogger("xvec.augment_wav")


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-g", "--gpu", type=int, default=0, help="The GPU id.")
    parser.add_argument("--sample-frequency", type=float, default=0.0, help="Refuse files of another rate (0: any, equal per line)")
    parser.add_argument("--batch-samples", type=int, default=32 << 20, help="Input samples packed into one device batch")
    parser.add_argument("wav_rspecifier", type=str, help="scp:wav.scp")
    parser.add_argument("out_dir", type=str)
    return parser


class _Rate(object):
    def __init__(self, fs):
        self.sample_frequency = fs or None


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if not args.wav_rspecifier.startswith("scp:"):
        sys.exit("augment_wav: the input must be scp:wav.scp")
    os.makedirs(args.out_dir, exist_ok=True)
    lines, todo, failed = [], [], set()
    for key, spec in read_wav_scp(args.wav_rspecifier):
        try:
            is_pipe = augment.parse_command(spec) is not None
        except ValueError as e:
            log.warning("[WARNING] %s: %s" % (key, e))
            failed.add(key)
            continue
        lines.append((key, spec, is_pipe))
        if is_pipe:
            todo.append((key, spec))

    def on_error(key, e):
        failed.add(key)
        log.warning("[WARNING] %s: %s" % (key, e))

    import torch
    rates = {}
    done = 0
    with torch.cuda.device(args.gpu):
        b_rate = _Rate(args.sample_frequency)
        for keys, wave, off in augment.native_batches(iter(todo), b_rate, args.batch_samples, -1, on_error, "cuda:%d" % args.gpu,
                                                      rates=rates):
            host = wave.cpu().numpy()
            for i, key in enumerate(keys):
                augment.write_wav(os.path.join(args.out_dir, key + ".wav"), rates[key], host[off[i]:off[i + 1]])
                done += 1
    with open(os.path.join(args.out_dir, "wav.scp"), "w") as f:
        for key, spec, is_pipe in lines:
            if key not in failed:
                f.write("%s %s\n" % (key, os.path.abspath(os.path.join(args.out_dir, key + ".wav")) if is_pipe else spec))
    log.info("Resolved %d pipelines, copied %d lines, %d with errors." % (done, len(lines) - len(todo), len(failed)))
    return 0 if done > 0 or not todo else 1


if __name__ == "__main__":
    sys.exit(main())
