"""compute-fbank-feats on the GPU: wav.scp in, Kaldi feature matrices out (the steps/make_fbank.sh step of
egs/voxceleb/v3/run.sh:54), and optionally the energy VAD of the same frames.

    python -m tf_kaldi_speaker_amd.compute_fbank [--config F] [--name=value ...] [--write-utt2num-frames F]
        [--vad-wspecifier W --vad-config V] scp:wav.scp ark,scp:feats.ark,feats.scp

Options are Kaldi's (see tf_kaldi_speaker_amd.fbank); --dither must be 0.  Output matrices are uncompressed float (`FM`).
A file made with --use-energy=false holds no energy column for compute-vad-decision to read (run.sh:58,66-68); with
--vad-wspecifier the decisions are made here, on the frame log energy the kernel computes on the way (--raw-energy and
--energy-floor of the fbank config apply to it).
**parity unpinned**."""
import argparse
import logging
import sys

from .compute_mfcc import TableWriter, device_batches
from .fbank import FbankOptions
from .mfcc import VadOptions, vad_packed

log = logging.getLogger("xvec.compute_fbank")


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-g", "--gpu", type=int, default=0, help="The GPU id.")
    parser.add_argument("--config", type=str, default="", help="Kaldi config file (--name=value lines), e.g. conf/fbank.conf")
    parser.add_argument("--channel", type=int, default=-1, help="Channel to extract (-1: the wav must be mono)")
    parser.add_argument("--write-utt2num-frames", type=str, default="", help="Write `key frames` lines to this file")
    parser.add_argument("--vad-wspecifier", type=str, default="", help="Also write the energy VAD decisions: ark:vad.ark or ark,scp:vad.ark,vad.scp")
    parser.add_argument("--vad-config", type=str, default="", help="Kaldi conf/vad.conf for --vad-wspecifier (default: Kaldi's defaults)")
    parser.add_argument("--batch-samples", type=int, default=32 << 20, help="Samples packed into one device batch (extension)")
    parser.add_argument("--native-reverberate", action="store_true",
                        help="Resolve `wav-reverberate ... |` lines on the GPU (tf_kaldi_speaker_amd.augment) instead of running Kaldi")
    FbankOptions.add_arguments(parser)
    parser.add_argument("wav_rspecifier", type=str, help="scp:wav.scp")
    parser.add_argument("feats_wspecifier", type=str, help="ark:feats.ark or ark,scp:feats.ark,feats.scp")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    try:
        opts = FbankOptions()
        if args.config:
            opts.update_from_config(args.config)
        opts.update_from_args(args)
        if args.vad_config and not args.vad_wspecifier:
            raise ValueError("--vad-config goes with --vad-wspecifier")
        vopts = VadOptions.from_config(args.vad_config) if args.vad_config else VadOptions()
    except ValueError as e:
        sys.exit("compute_fbank: %s" % e)
    if not args.wav_rspecifier.startswith("scp:"):
        sys.exit("compute_fbank: the input must be scp:wav.scp")
    import torch
    from .fbank import Fbank
    dev = "cuda:%d" % args.gpu
    fbank = Fbank(opts, args.gpu)
    writer = TableWriter(args.feats_wspecifier)
    vad_writer = TableWriter(args.vad_wspecifier) if args.vad_wspecifier else None
    u2n = open(args.write_utt2num_frames, "w") if args.write_utt2num_frames else None
    done = failed = 0

    def on_error(key, e):
        nonlocal failed
        failed += 1
        log.warning("[WARNING] %s: %s" % (key, e))

    with torch.cuda.device(args.gpu):
        for keys, samples, offsets in device_batches(args, opts, dev, on_error):
            vad = None
            if vad_writer:
                feats, foff, energy = fbank.compute(samples, offsets, energy=True)
                vad = vad_packed(energy.view(-1, 1), foff, vopts).cpu().numpy()
            else:
                feats, foff = fbank.compute(samples, offsets)
            feats = feats.cpu().numpy()
            for i, key in enumerate(keys):
                if foff[i + 1] == foff[i]:
                    failed += 1
                    log.warning("[WARNING] %s: no frames for %d samples, skipped" % (key, offsets[i + 1] - offsets[i]))
                    continue
                writer.write_mat(key, feats[foff[i]:foff[i + 1]])
                if vad_writer:
                    vad_writer.write_vec(key, vad[foff[i]:foff[i + 1]])
                if u2n:
                    u2n.write("%s %d\n" % (key, foff[i + 1] - foff[i]))
                done += 1
    writer.close()
    if vad_writer:
        vad_writer.close()
    if u2n:
        u2n.close()
    fbank.close()
    log.info("Done %d utterances, %d with errors." % (done, failed))
    return 0 if done > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
