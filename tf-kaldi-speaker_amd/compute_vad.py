"""compute-vad-decision on the GPU: feature table in, per-frame 0/1 vectors out (the sid/compute_vad_decision.sh step of
egs/voxceleb/v1/run.sh:57-65).

    python -m tf_kaldi_speaker_amd.compute_vad [--config F] [--name=value ...] scp:feats.scp ark,scp:vad.ark,vad.scp

**parity unpinned**."""
import argparse
import logging
import sys

import numpy as np

from .compute_mfcc import TableWriter
from .mfcc import VadOptions, vad_packed

log = logging.getLogger("xvec.compute_vad")


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-g", "--gpu", type=int, default=0, help="The GPU id.")
    parser.add_argument("--config", type=str, default="", help="Kaldi config file (--name=value lines), e.g. conf/vad.conf")
    parser.add_argument("--batch-frames", type=int, default=1 << 18, help="Frames packed into one device batch (extension)")
    VadOptions.add_arguments(parser)
    parser.add_argument("feats_rspecifier", type=str, help="scp:feats.scp or ark:feats.ark")
    parser.add_argument("vad_wspecifier", type=str, help="ark:vad.ark or ark,scp:vad.ark,vad.scp")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    try:
        vopts = VadOptions()
        if args.config:
            vopts.update_from_config(args.config)
        vopts.update_from_args(args)
    except ValueError as e:
        sys.exit("compute_vad: %s" % e)
    import torch
    from . import native_ark
    dev = "cuda:%d" % args.gpu
    reader = native_ark.ArkBatchReader(args.feats_rspecifier, batch_frames=args.batch_frames, min_frames=1)
    writer = TableWriter(args.vad_wspecifier)
    done = skipped = 0
    try:
        with torch.cuda.device(args.gpu):
            for keys, offsets, feats in reader:
                offsets = np.asarray(offsets, dtype=np.int32)
                vad = vad_packed(torch.from_numpy(np.ascontiguousarray(feats)).to(dev), offsets, vopts).cpu().numpy()
                for i, key in enumerate(keys):
                    writer.write_vec(key, vad[offsets[i]:offsets[i + 1]])
                    done += 1
        skipped = reader.skipped
    finally:
        reader.close()
        writer.close()
    log.info("Applied energy based voice activity detection; processed %d utterances (%d empty ones skipped)." % (done, skipped))
    return 0 if done > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
