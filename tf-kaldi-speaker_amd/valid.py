"""Validation of a checkpoint on the GPU: what the reference does after every epoch (egs/voxceleb/v1/nnet/lib/train.py:106-155):
`trainer.build("valid")`, `trainer.valid(valid_dir, valid_spklist, output_embeddings=True)`, `compute_cos_pairwise_eer` and one
`epoch loss eer` line appended to <model_dir>/nnet/valid_loss (train.py:33 joins "nnet" to the model directory first).

    python -m tf_kaldi_speaker_amd.valid [--gpu N] [--checkpoint NAME] [--precision P] [--no-eer] [--append]
                                         model_dir valid_dir valid_spklist

prints one line `step <step> loss <loss> acc <top-1 accuracy> eer <eer>`.  The batch plan (plan_batches, read_batch) is pure
host code; the forward pass, the loss heads (losses.py) and the pairwise EER (scoring.py) run on the GPU and have no CPU path."""
import argparse
import collections
import os
import sys

import numpy as np

from . import model_io
from .kaldi_io import read_mat
from .params import Params

Batch = collections.namedtuple("Batch", "keys rxfiles labels length")


def read_speaker_info(data, spklist):
    """get_speaker_info (dataset/data_loader.py:36-77) -> (spk2features {index: [(key, rxfile)]}, number of speakers in
    spklist).  A speaker of spklist may be absent from the data (:48-49); a speaker of the data that spklist does not name is a
    KeyError, as in the reference."""
    spk2index = {}
    with open(spklist, "r") as f:
        for line in f:
            if line.strip():
                spk, index = line.strip().split(" ")
                spk2index[spk] = int(index)
    utt2spk = {}
    with open(os.path.join(data, "spk2utt"), "r") as f:
        for line in f:
            if line.strip():
                spk, utts = line.strip().split(" ", 1)
                for utt in utts.split(" "):
                    utt2spk[utt] = spk2index[spk]
    spk2features = {}
    with open(os.path.join(data, "feats.scp"), "r") as f:
        for line in f:
            if line.strip():
                key, rxfile = line.strip().split(" ", 1)
                spk2features.setdefault(utt2spk[key], []).append((key, rxfile.strip()))
    return spk2features, len(spk2index)


def read_utt2num_frames(data):
    """FeatureReader.utt2num_frames (dataset/data_loader.py): $data/utt2num_frames, `key frames` per line."""
    path = os.path.join(data, "utt2num_frames")
    if not os.path.isfile(path):
        raise IOError("%s is missing: the batch length is clipped to the shortest utterance of the batch from it "
                      "(dataset/data_loader.py:537-541)" % path)
    out = {}
    with open(path, "r") as f:
        for line in f:
            if line.strip():
                key, frames = line.split()
                out[key] = int(frames)
    return out


def plan_batches(data, spklist, batch_size, target_len, max_iterations=None):
    """The batches KaldiDataSeqQueue(num_parallel=2, shuffle=False) + batch_sequence (dataset/data_loader.py:498-661) yield
    with min_len == max_len == target_len -> [Batch(keys, rxfiles, labels, length)]:

      1. the feature list is built speaker by speaker, feats.scp order inside a speaker.  The reference iterates a Python-2 dict
         over the speaker indices, whose order the language leaves open; HERE THE ORDER IS ASCENDING SPEAKER INDEX;
      2. it is split in two at len // 2 (one sub-list per reader process, :593-598);
      3. each sub-list yields len // B + 1 batches of min(B, len) utterances, the list wrapped round to fill the last (:528-532);
         the reference's two processes feed one queue in the order they happen to finish; here the first sub-list's batches
         come first, then the second's;
      4. the length of a batch is target_len shortened to its shortest utterance by utt2num_frames (:537-541), every segment
         starting at frame 0 (shuffle=False);
      5. the walk stops after `max_iterations` batches (valid_max_iterations, model/trainer.py:860)."""
    batch_size, target_len = int(batch_size), int(target_len)
    if batch_size < 1 or target_len < 1:
        raise ValueError("batch size and segment length must be positive, got %d and %d" % (batch_size, target_len))
    spk2features, _ = read_speaker_info(data, spklist)
    frames = read_utt2num_frames(data)
    features = []
    for spk in sorted(spk2features):
        features += [(key, rx, spk) for key, rx in spk2features[spk]]
    half = len(features) // 2
    out = []
    for sub in (features[:half], features[half:]):
        if not sub:
            continue          # the reference's process would divide by zero on an empty sub-list (:532) and never finish
        num_batches = len(sub) // batch_size + 1
        b = min(batch_size, len(sub))
        for i in range(num_batches):
            items = [sub[(i * b + j) % len(sub)] for j in range(b)]
            length = min([target_len] + [frames[key] for key, _, _ in items])
            out.append(Batch([k for k, _, _ in items], [r for _, r, _ in items], np.array([s for _, _, s in items], dtype=np.int32),
                             length))
    if max_iterations is not None:
        out = out[:int(max_iterations)]
    return out


def plan_for_params(data, spklist, params):
    """plan_batches with the sizes Trainer.valid takes from the config (model/trainer.py:832-838, 860)."""
    p = params.dict
    return plan_batches(data, spklist, int(p["num_speakers_per_batch"]) * int(p["num_segments_per_speaker"]),
                        (int(p["min_segment_len"]) + int(p["max_segment_len"])) // 2, p.get("valid_max_iterations"))


def read_batch(batch, dim, cache=None):
    """-> float32 [B, length, dim]: the first `length` frames of every utterance; columns beyond `dim` are dropped
    (model/trainer.py:865-866), fewer than `dim` is a ValueError.  `cache` ({rxfile: matrix}) spares re-reading wrapped rows."""
    out = np.zeros((len(batch.keys), batch.length, dim), dtype=np.float32)
    for j, (key, rx) in enumerate(zip(batch.keys, batch.rxfiles)):
        mat = cache.get(rx) if cache is not None else None
        if mat is None:
            mat = read_mat(rx)
            if cache is not None:
                cache[rx] = mat
        if mat.shape[1] < dim:
            raise ValueError("%s: features have %d columns, the network needs %d" % (key, mat.shape[1], dim))
        if mat.shape[0] < batch.length:
            raise ValueError("%s: %d frames in the archive, utt2num_frames promised at least %d" % (key, mat.shape[0], batch.length))
        out[j] = mat[:batch.length, :dim]
    return out


def format_valid_loss(step, loss, eer):
    """The line of <model_dir>/nnet/valid_loss (train.py:154-155), the checkpoint step in place of the epoch."""
    return "%d %f %f\n" % (step, loss, eer)


def format_report(step, loss, acc, eer):
    return "step %d loss %f acc %f eer %s" % (step, loss, acc, "nan" if eer is None else "%f" % eer)


def build_parser():
    parser = argparse.ArgumentParser(description="Validation loss, top-1 accuracy and cosine pairwise EER of a checkpoint.")
    parser.add_argument("-g", "--gpu", type=int, default=-1, help="The GPU id (-1: LOCAL_RANK or 0; there is no CPU path).")
    parser.add_argument("--checkpoint", type=str, default="", help="Checkpoint name under <model_dir>/nnet (e.g. model-120000); "
                        "default: the one nnet/checkpoint names.")
    parser.add_argument("--precision", type=str, default="", help="f32 | bf16x3 | f16x3 | f16f6 (default: the trainer's)")
    parser.add_argument("--no-eer", action="store_true", help="Skip the pairwise EER.")
    parser.add_argument("--append", action="store_true", help="Append `step loss eer` to <model_dir>/nnet/valid_loss (train.py:33,154-155).")
    parser.add_argument("model_dir", type=str, help="The model directory.")
    parser.add_argument("valid_dir", type=str, help="The Kaldi data directory of the validation set.")
    parser.add_argument("valid_spklist", type=str, help="The spklist of the validation set: `speaker index` per line.")
    parser.epilog = ("The EER is taken over ALL pairs of the validation embeddings (scoring.pairwise_eer, score histograms on the GPU). "
                     "The reference down-samples to 1000 rows (misc/utils.py:319-323) only because its pair loop runs in Python.")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.append and args.no_eer:
        sys.exit("--append writes `step loss eer`: it cannot be combined with --no-eer")
    nnet_dir = os.path.join(args.model_dir, "nnet")
    config_json = os.path.join(nnet_dir, "config.json")
    if not os.path.isfile(config_json):
        sys.exit("Cannot find params.json in %s" % config_json)
    params = Params(config_json)
    with open(os.path.join(nnet_dir, "feature_dim"), "r") as f:
        dim = int(f.readline().strip())
    if "selected_dim" in params.dict:
        dim = params.selected_dim
    from . import scoring
    from .trainer import Trainer
    trainer = Trainer(params, args.model_dir, dim, single_cpu=True, device=args.gpu if args.gpu >= 0 else None,
                      precision=args.precision or None)
    trainer.build("valid")
    if args.checkpoint:
        weights, step = model_io.load_weights(nnet_dir, name=args.checkpoint)
        if weights is None:
            sys.exit("Cannot find checkpoint %s in %s" % (args.checkpoint, nnet_dir))
        trainer.load_weights(weights, step)
    loss, emb, labels = trainer.valid(args.valid_dir, args.valid_spklist, batch_type=params.dict.get("batch_type", "softmax"),
                                      output_embeddings=not args.no_eer)
    eer = None
    if not args.no_eer:
        eer = scoring.pairwise_eer(emb, labels, device=trainer._device_index)[0]
    step = int(trainer._step or 0)
    print(format_report(step, loss, trainer.valid_accuracy, eer))
    if args.append:
        with open(os.path.join(nnet_dir, "valid_loss"), "a") as f:
            f.write(format_valid_loss(step, loss, eer))
    trainer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
