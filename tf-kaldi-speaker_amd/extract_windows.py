"""Sliding-window x-vectors: every input matrix is cut into overlapping windows and each window is embedded on its own, the
sub-segment embeddings that speaker clustering (cluster.py) groups into speakers.  What Kaldi's
diarization/nnet3/xvector/extract_xvectors.sh does with --window / --period / --min-segment; the reference has no such step.

    python -m tf_kaldi_speaker_amd.extract_windows [-g GPU] [--window 150] [--period 75] [--min-segment 25]
           [--frame-shift 0.01] [--cmn-window W] [--node NODE] [--precision P] [-n] [--batch-frames N]
           model_dir <feats-rspecifier> <xvector-wspecifier> <segments-out>

The windows of an input of T frames are [k * period, min(k * period + window, T)) for k = 0, 1, ... up to the first that ends
at the last frame; a final window shorter than --min-segment frames is dropped, and an input shorter than --min-segment is
skipped with extract's message.  Each window goes through Trainer.predict_list as an utterance of its own and is written under
the key `<utt>-<start:07d>-<end:07d>` (frames); <segments-out> gets one line `key utt start_s end_s` per window with the
times in seconds (frame * --frame-shift).  --cmn-window W applies extract's centred sliding-window CMN to the whole input
before it is cut.  No VAD is applied: the inputs are the speech segments."""
import argparse
import logging
import os
import sys

import numpy as np

from .params import Params

log = logging.getLogger("xvec.extract_windows")


def plan_windows(num_frames, window, period, min_segment):
    """(start, end) frame ranges of the windows of an input of num_frames frames, in order; [] for one shorter than min_segment."""
    if window < 1 or period < 1 or min_segment < 1:
        raise ValueError("window, period and min_segment must be positive")
    if num_frames < min_segment:
        return []
    out, start = [], 0
    for _ in range(num_frames):                     # a window per frame at the very most
        end = min(start + window, num_frames)
        if end - start < min_segment:
            break
        out.append((start, end))
        if end == num_frames:
            break
        start += period
    return out


def window_key(utt, start, end):
    return "%s-%07d-%07d" % (utt, start, end)


def segment_line(utt, start, end, frame_shift):
    return "%s %s %.3f %.3f\n" % (window_key(utt, start, end), utt, start * frame_shift, end * frame_shift)


def build_parser():
    ap = argparse.ArgumentParser(prog="extract_windows", description=__doc__.split("\n\n")[0])
    ap.add_argument("-g", "--gpu", type=int, default=0, help="HIP device")
    ap.add_argument("--window", type=int, default=150, help="frames per window; default 150")
    ap.add_argument("--period", type=int, default=75, help="frames between window starts; default 75")
    ap.add_argument("--min-segment", type=int, default=25, help="shortest window (and input) that is embedded; default 25")
    ap.add_argument("--frame-shift", type=float, default=0.01, help="seconds per frame, for <segments-out>; default 0.01")
    ap.add_argument("--cmn-window", type=int, default=0, help="centred sliding-window CMN over the whole input first (0: off)")
    ap.add_argument("--node", type=str, default="", help="The node to output the embeddings.")
    ap.add_argument("--precision", type=str, default="", help="f32 | bf16x3 | f16x3 | f16f6 (default: library default)")
    ap.add_argument("-n", "--normalize", action="store_true", help="L2-normalise every embedding")
    ap.add_argument("--batch-frames", type=int, default=153600, help="frames packed into one device batch")
    ap.add_argument("model_dir")
    ap.add_argument("feats_rspecifier")
    ap.add_argument("xvector_wspecifier")
    ap.add_argument("segments_out")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.window < 1 or args.period < 1 or args.min_segment < 1:
        ap.error("--window, --period and --min-segment must be positive")
    if args.min_segment > args.window:
        ap.error("--min-segment %d is longer than --window %d" % (args.min_segment, args.window))
    if not args.frame_shift > 0.0:
        ap.error("--frame-shift must be positive")
    if args.cmn_window < 0 or args.batch_frames < 1:
        ap.error("--cmn-window must be >= 0 and --batch-frames positive")
    return args


def run(trainer, items, writer, seg_file, args, cmn=None):
    """items yields (utt, [T, d] matrix).  -> (windows written, inputs skipped)."""
    done = skipped = 0
    keys, pieces, frames = [], [], 0

    def flush():
        nonlocal done, keys, pieces, frames
        if keys:
            emb = np.asarray(trainer.predict_list(pieces))
            if args.normalize:
                emb = emb / np.sqrt(np.sum(np.square(emb), axis=1, keepdims=True))
            writer.write(keys, emb)
            done += len(keys)
        keys, pieces, frames = [], [], 0

    for utt, feature in items:
        t = feature.shape[0]
        plan = plan_windows(t, args.window, args.period, args.min_segment)
        if not plan:
            log.info("[INFO] Key %s length too short, %d < %d, skip.", utt, t, args.min_segment)
            skipped += 1
            continue
        if cmn is not None:
            feature = cmn(feature)
        for start, end in plan:
            keys.append(window_key(utt, start, end))
            pieces.append(feature[start:end])
            seg_file.write(segment_line(utt, start, end, args.frame_shift))
            frames += end - start
        if frames >= args.batch_frames:
            flush()
    flush()
    return done, skipped


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    config_json = os.path.join(args.model_dir, "nnet/config.json")
    if not os.path.isfile(config_json):
        sys.exit("Cannot find params.json in %s" % config_json)
    params = Params(config_json)
    if args.node:
        params.embedding_node = args.node
    with open(os.path.join(args.model_dir, "nnet", "feature_dim"), "r") as f:
        dim = int(f.readline().strip())
    from . import native_ark
    from .kaldi_io import read_mat_ark
    from .trainer import Trainer
    trainer = Trainer(params, args.model_dir, dim, single_cpu=True, device=args.gpu, precision=args.precision or None)
    trainer.build("predict")
    if trainer.model is not None and os.path.isfile(os.path.join(trainer.model, "checkpoint")):
        trainer.load()
    cmn = None
    if args.cmn_window > 0:
        import torch
        from .frontend import cmn_select_packed

        def cmn(feature):
            with torch.cuda.device(args.gpu):
                raw = torch.from_numpy(np.ascontiguousarray(feature, dtype=np.float32)).to("cuda:%d" % args.gpu)
                out, _, _ = cmn_select_packed(raw, [0, feature.shape[0]], None, cmn_window=args.cmn_window, min_frames=0)
                return out.cpu().numpy()

    writer = native_ark.VectorWriter(args.xvector_wspecifier)
    with open(args.segments_out, "w") as seg_file:
        done, skipped = run(trainer, read_mat_ark(args.feats_rspecifier), writer, seg_file, args, cmn)
    rc = writer.close()
    trainer.close()
    log.info("Extracted %d window embeddings (%d inputs skipped)" % (done, skipped))
    if rc != 0:
        log.error("the output command of %s exited with code %d" % (args.xvector_wspecifier, rc))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
