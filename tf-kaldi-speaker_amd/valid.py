"""Validation of a checkpoint on the GPU: what the reference does after every epoch (egs/voxceleb/v1/nnet/lib/train.py:106-155):
`trainer.build("valid")`, `trainer.valid(valid_dir, valid_spklist, output_embeddings=True)`, `compute_cos_pairwise_eer` and one
`epoch loss eer` line appended to <model_dir>/nnet/valid_loss (train.py:33 joins "nnet" to the model directory first).

    python -m tf_kaldi_speaker_amd.valid [--gpu N] [--checkpoint NAME] [--precision P] [--no-eer] [--append]
                                         model_dir valid_dir valid_spklist

prints one line `step <step> loss <loss> acc <top-1 accuracy> eer <eer>`.  The batch plan (plan_batches, plan_end2end_batches,
read_batch) is pure host code; the forward pass, the loss heads (losses.py, metric_losses.py) and the pairwise EER (scoring.py)
run on the GPU and have no CPU path.  A checkpoint trained with `semihard_triplet_loss` or `angular_triplet_loss` goes through
metric_valid instead of Trainer.valid (model/trainer.py:407-436: the angular triplet loss is validated with e2e_valid_loss)."""
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


def plan_end2end_batches(data, spklist, num_speakers, num_segments, target_len, max_iterations=None):
    """Batches of N speakers x M segments, what KaldiDataRandomQueue (dataset/data_loader.py:289-356) feeds the end-to-end
    losses, made deterministic where the reference draws from os.urandom -> [Batch(keys, rxfiles, labels, length)]:

      1. an utterance is eligible when utt2num_frames > target_len (strict, :334); the speakers are those with an eligible
         utterance, in ascending index, S of them.  S < N is a ValueError (the reference would draw a speaker twice there and
         make two classes of one voice);
      2. `max_iterations` batches (valid_max_iterations: the reference's queue never ends), ceil(S / N) without it;
      3. batch b takes the speakers (b N + i) mod S, i = 0 .. N - 1; the t-th appearance of a speaker (t from 0) takes its
         eligible utterances (t M + j) mod E, j = 0 .. M - 1, in feats.scp order (the wrap is the list duplication of :345-346);
      4. every segment is the frames [0, target_len); rows are speaker-major and the label is the speaker index."""
    n, m, target_len = int(num_speakers), int(num_segments), int(target_len)
    if n < 1 or m < 1 or target_len < 1:
        raise ValueError("speakers, segments and segment length must be positive, got %d, %d and %d" % (n, m, target_len))
    spk2features, _ = read_speaker_info(data, spklist)
    frames = read_utt2num_frames(data)
    eligible = {}
    for spk in sorted(spk2features):
        utts = [(key, rx) for key, rx in spk2features[spk] if frames[key] > target_len]
        if utts:
            eligible[spk] = utts
    speakers = sorted(eligible)
    if len(speakers) < n:
        raise ValueError("%d speakers have an utterance of more than %d frames, a batch needs %d" % (len(speakers), target_len, n))
    num_batches = -(-len(speakers) // n) if max_iterations is None else int(max_iterations)
    seen = dict.fromkeys(speakers, 0)
    out = []
    for b in range(num_batches):
        keys, rxfiles, labels = [], [], []
        for i in range(n):
            spk = speakers[(b * n + i) % len(speakers)]
            utts = eligible[spk]
            for j in range(m):
                key, rx = utts[(seen[spk] * m + j) % len(utts)]
                keys.append(key)
                rxfiles.append(rx)
                labels.append(spk)
            seen[spk] += 1
        out.append(Batch(keys, rxfiles, np.array(labels, dtype=np.int32), target_len))
    return out


METRIC_LOSSES = ("semihard_triplet_loss", "angular_triplet_loss")      # validated by metric_valid, not by Trainer.valid


def metric_valid(trainer, data, spklist, batch_type="softmax", output_embeddings=False):
    """Trainer.valid for a checkpoint trained with a metric-learning loss -> (loss, embeddings or None, labels or None).
    The network runs to the `output` endpoint exactly as Trainer.valid runs it; the batches are those of plan_for_params
    (batch_type "softmax") or of plan_end2end_batches with num_valid_speakers_per_batch x num_valid_segments_per_speaker
    ("end2end", model/trainer.py:839-853); all of them go to the head metric_losses.from_params names in ONE call, and the
    loss is the mean of the batch losses.  trainer.valid_accuracy holds the top-1 accuracy of the ge2e head, nan otherwise."""
    from . import metric_losses
    assert batch_type == "softmax" or batch_type == "end2end", "The batch_type can only be softmax or end2end"
    params = trainer.params
    head = metric_losses.from_params(params, validation=True, device=trainer._device_index)
    p = params.dict
    if batch_type == "end2end":
        assert "num_valid_speakers_per_batch" in p and "num_valid_segments_per_speaker" in p, \
            "Valid parameters should be set if E2E loss is selected"                  # trainer.py:843-844
        plan = plan_end2end_batches(data, spklist, p["num_valid_speakers_per_batch"], p["num_valid_segments_per_speaker"],
                                    (int(p["min_segment_len"]) + int(p["max_segment_len"])) // 2, p.get("valid_max_iterations"))
    else:
        plan = plan_for_params(data, spklist, params)
    if not plan:
        raise ValueError("no validation batch in %s" % data)
    trainer.build("predict")
    trainer.embeddings = "output"                                                     # valid_setup, trainer.py:460
    embs, labs, cache = [], [], {}
    for batch in plan:
        embs.append(trainer.predict(read_batch(batch, trainer.dim, cache)))
        labs.append(batch.labels)
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in labs])]).astype(np.int64)
    emb, labels = np.concatenate(embs, axis=0), np.concatenate(labs, axis=0)
    res = head(emb, labels, offsets)
    trainer.valid_num_batches = len(plan)
    trainer.valid_accuracy = float(np.mean(res.top1 == labels)) if res.top1 is not None else float("nan")
    if output_embeddings:
        return res.loss, emb, labels
    return res.loss, None, None


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
    metric = params.dict.get("loss_func") in METRIC_LOSSES
    trainer.build("predict" if metric else "valid")
    if args.checkpoint:
        weights, step = model_io.load_weights(nnet_dir, name=args.checkpoint)
        if weights is None:
            sys.exit("Cannot find checkpoint %s in %s" % (args.checkpoint, nnet_dir))
        trainer.load_weights(weights, step)
    run = (lambda *a, **k: metric_valid(trainer, *a, **k)) if metric else trainer.valid
    loss, emb, labels = run(args.valid_dir, args.valid_spklist, batch_type=params.dict.get("batch_type", "softmax"),
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
