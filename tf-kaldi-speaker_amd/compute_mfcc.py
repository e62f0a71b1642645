"""compute-mfcc-feats on the GPU: wav.scp in, Kaldi feature matrices out (the steps/make_mfcc.sh step of
egs/voxceleb/v1/run.sh:57-65).

    python -m tf_kaldi_speaker_amd.compute_mfcc [--config F] [--name=value ...] scp:wav.scp ark,scp:feats.ark,feats.scp

Options are Kaldi's (see tf_kaldi_speaker_amd.mfcc); --dither must be 0.  Output matrices are uncompressed float (`FM`).
**parity unpinned**."""
import argparse
import logging
import sys

import numpy as np

from .mfcc import MfccOptions, read_wav_scp, wav_batches

log = logging.getLogger("xvec.compute_mfcc")


class TableWriter(object):
    """`ark:F`, `scp:`-less `ark,scp:F.ark,F.scp` or a bare path: binary records plus the optional `key F.ark:offset` table."""

    def __init__(self, wspecifier):
        spec = wspecifier.strip()
        head, _, rest = spec.partition(":")
        kinds = head.split(",") if _ and head.split(",")[0] in ("ark", "scp") else None
        if kinds is None:
            kinds, rest = ["ark"], spec
        if "t" in kinds:
            raise ValueError("text-mode output is not supported: %s" % wspecifier)
        files = [f.strip() for f in rest.split(",")]
        tables = [k for k in kinds if k in ("ark", "scp")]
        if tables == ["ark"] and len(files) == 1:
            self.ark_path, self.scp_path = files[0], None
        elif tables == ["ark", "scp"] and len(files) == 2:
            self.ark_path, self.scp_path = files
        else:
            raise ValueError("wspecifier must be ark:FILE or ark,scp:FILE.ark,FILE.scp, got %s" % wspecifier)
        self.ark = open(self.ark_path, "wb")
        self.scp = open(self.scp_path, "w") if self.scp_path else None

    def _put(self, key, header, payload):
        rec = (key + " ").encode("latin1")
        self.ark.write(rec)
        if self.scp:
            self.scp.write("%s %s:%d\n" % (key, self.ark_path, self.ark.tell()))
        self.ark.write(header)
        self.ark.write(payload)

    def write_mat(self, key, m):
        import struct
        m = np.ascontiguousarray(m, dtype=np.float32)
        self._put(key, b"\0BFM \x04" + struct.pack("<I", m.shape[0]) + b"\x04" + struct.pack("<I", m.shape[1]), m.tobytes())

    def write_vec(self, key, v):
        import struct
        v = np.ascontiguousarray(v, dtype=np.float32)
        self._put(key, b"\0BFV \x04" + struct.pack("<I", v.shape[0]), v.tobytes())

    def close(self):
        self.ark.close()
        if self.scp:
            self.scp.close()


def device_batches(args, opts, dev, on_error):
    """(keys, int16 CUDA tensor, sample offsets) per batch of the wav.scp: read on the host and copied, or, with
    --native-reverberate, wav-reverberate pipelines resolved on the device (other lines go through read_wav as before)."""
    import torch
    items = read_wav_scp(args.wav_rspecifier)
    if args.native_reverberate:
        from .augment import native_batches
        return native_batches(items, opts, args.batch_samples, args.channel, on_error, dev)
    return ((keys, torch.from_numpy(samples).to(dev), offsets)
            for keys, samples, offsets in wav_batches(items, opts, args.batch_samples, args.channel, on_error))


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("-g", "--gpu", type=int, default=0, help="The GPU id.")
    parser.add_argument("--config", type=str, default="", help="Kaldi config file (--name=value lines), e.g. conf/mfcc.conf")
    parser.add_argument("--channel", type=int, default=-1, help="Channel to extract (-1: the wav must be mono)")
    parser.add_argument("--write-utt2num-frames", type=str, default="", help="Write `key frames` lines to this file")
    parser.add_argument("--batch-samples", type=int, default=32 << 20, help="Samples packed into one device batch (extension)")
    parser.add_argument("--native-reverberate", action="store_true",
                        help="Resolve `wav-reverberate ... |` lines on the GPU (tf_kaldi_speaker_amd.augment) instead of running Kaldi")
    MfccOptions.add_arguments(parser)
    parser.add_argument("wav_rspecifier", type=str, help="scp:wav.scp")
    parser.add_argument("feats_wspecifier", type=str, help="ark:feats.ark or ark,scp:feats.ark,feats.scp")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    try:
        opts = MfccOptions()
        if args.config:
            opts.update_from_config(args.config)
        opts.update_from_args(args)
    except ValueError as e:
        sys.exit("compute_mfcc: %s" % e)
    if not args.wav_rspecifier.startswith("scp:"):
        sys.exit("compute_mfcc: the input must be scp:wav.scp")
    import torch
    from .mfcc import Mfcc
    dev = "cuda:%d" % args.gpu
    mfcc = Mfcc(opts, args.gpu)
    writer = TableWriter(args.feats_wspecifier)
    u2n = open(args.write_utt2num_frames, "w") if args.write_utt2num_frames else None
    done = failed = 0

    def on_error(key, e):
        nonlocal failed
        failed += 1
        log.warning("[WARNING] %s: %s" % (key, e))

    with torch.cuda.device(args.gpu):
        for keys, samples, offsets in device_batches(args, opts, dev, on_error):
            feats, foff = mfcc.compute(samples, offsets)
            feats = feats.cpu().numpy()
            for i, key in enumerate(keys):
                if foff[i + 1] == foff[i]:
                    failed += 1
                    log.warning("[WARNING] %s: no frames for %d samples, skipped" % (key, offsets[i + 1] - offsets[i]))
                    continue
                writer.write_mat(key, feats[foff[i]:foff[i + 1]])
                if u2n:
                    u2n.write("%s %d\n" % (key, foff[i + 1] - foff[i]))
                done += 1
    writer.close()
    if u2n:
        u2n.close()
    mfcc.close()
    log.info("Done %d utterances, %d with errors." % (done, failed))
    return 0 if done > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
