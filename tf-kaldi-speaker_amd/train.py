"""Train a network from nothing: the stage of egs/*/run.sh between the prepared features and the extraction
(nnet/run_train_nnet.sh -> nnet/lib/train.py), with that script's positional arguments, `-c` and `--config`.

    python -m tf_kaldi_speaker_amd.train [--gpu N] [-c] [--config nnet_conf/x.json] [--seed S] [--prefetch K]
                                         [--batch-norm {batch,moving}] train_dir train_spklist valid_dir valid_spklist model_dir

It writes <model_dir>/nnet/config.json and feature_dim, starts from fresh_weights (or, with -c, from the last checkpoint and
its optimizer file), builds the trainer head_train.train_head(conv_layers=True, batch_norm="batch") builds for the configuration
(conv_train.ConvTrainer, att_train.AttConvTrainer for self_attention pooling, resnet_train.ResNetTrainer; behind the metric door
for the two triplet losses) and runs num_steps_per_epoch steps per epoch on the batches of train_input.Loader.  After every epoch:
head_train.finish_epoch (checkpoint, validation on the written directory, pairwise EER, one line each in valid_loss and
learning_rate), nnet/optimizer-<step>.npz beside the checkpoint, and the stopping rule of train.py:157-163 with
early_stop_epochs defaulting to 10.  `save_checkpoints_steps` writes a checkpoint pair inside an epoch, `keep_checkpoint_max`
prunes older pairs.  is_training=True is the reference's mode, so --batch-norm batch is the default here.

Departures from the reference, both **parity unpinned**: the batches are head_train.plan_train_batches' (deterministic, a function
of the seed and the epoch, where KaldiDataRandomQueue seeds its workers from os.urandom), and the initial values are
fresh_weights' (TensorFlow's default initialisers, drawn from numpy streams).  Out of scope: more than one GPU (-n above 1 is
refused), TensorFlow-bundle output, summaries, sample_with_prob, raw features with VAD and CMN at batch time, augmentation on
the fly, and everything the trainers' check_supported refuse (PReLU, feature_norm, aux_loss_func, ...)."""
import argparse
import glob
import json
import os
import re
import sys
import time

import numpy as np

from . import head_train
from . import model_io
from . import synth
from .params import Params

_ONE = ("gamma", "moving_variance")
_ZERO = ("bias", "beta", "moving_mean")


def _truncated_normal(rs, shape, stddev):
    """tf.initializers.truncated_normal: values beyond two standard deviations are drawn again."""
    x = rs.standard_normal(shape)
    while True:
        bad = np.abs(x) > 2.0
        if not bad.any():
            return (stddev * x).astype(np.float32)
        x[bad] = rs.standard_normal(int(bad.sum()))


def fresh_weights(params, dim, num_speakers, seed, channels=512, width=64):
    """Every variable of the network under its TensorFlow name and in the checkpoint's shape, with TensorFlow's default initial
    values: kernels glorot_uniform (limit sqrt(6 / (fan_in + fan_out)), the fans times the receptive field), biases and beta 0,
    gamma 1, moving_mean 0, moving_variance 1, the attention query by model/pooling.py:173-183 (Xavier when att_query_init is
    "xavier_init", else truncated normal of stddev 0.1), softmax/output/kernel from head_train.xavier_uniform and a zero
    softmax/output/bias for the plain softmax; no head for the two triplet losses.  The variable set is the one
    synth.synth_weights / synth.synth_resnet_weights enumerate (`channels` / `width`: 512 / 64 in the reference).  Variable i in
    sorted-name order draws from numpy.random.RandomState([seed, i]): one seed gives the same bits everywhere.  **Parity
    unpinned** against TensorFlow's random streams.  What the trainers refuse is refused here, with their messages."""
    metric = check_supported(params)[1]
    d = params if isinstance(params, dict) else params.dict
    if d.get("network_type", "tdnn") == "resnet_18":
        shapes = synth.synth_resnet_weights(params, 0, width)
    else:
        shapes = synth.synth_weights(params, int(dim), 0, channels)
    shapes = {k: tuple(v.shape) for k, v in shapes.items()}
    if not metric:
        from . import tail_train
        embed_dim = shapes[tail_train.segment_variables(params)[1].kernel][1]
        shapes[model_io.SOFTMAX_KERNEL] = (embed_dim, int(num_speakers))
        if d.get("loss_func") == "softmax":
            shapes[model_io.SOFTMAX_BIAS] = (int(num_speakers),)
    out = {}
    for i, name in enumerate(sorted(shapes)):
        shape, leaf = shapes[name], name.rsplit("/", 1)[-1]
        stream = [int(seed) & 0xFFFFFFFF, i]
        if name == model_io.SOFTMAX_KERNEL:
            out[name] = head_train.xavier_uniform(shape[0], shape[1], stream)
        elif leaf == "kernel":
            out[name] = synth._glorot(np.random.RandomState(stream), shape)
        elif leaf == "query":
            rs = np.random.RandomState(stream)
            out[name] = synth._glorot(rs, shape) if d.get("att_query_init") == "xavier_init" else _truncated_normal(rs, shape, 0.1)
        elif leaf in _ONE:
            out[name] = np.ones(shape, dtype=np.float32)
        elif leaf in _ZERO:
            out[name] = np.zeros(shape, dtype=np.float32)
        else:
            raise NotImplementedError("%s: no initial value for this variable" % name)
    return out


def check_supported(params):
    """The checks head_train.train_head(conv_layers=True) makes before it touches anything -> (which trainer: "attention",
    "resnet" or "conv", whether the metric door is taken)."""
    from . import valid as valid_mod
    d = params if isinstance(params, dict) else params.dict
    metric = d.get("loss_func") in valid_mod.METRIC_LOSSES
    if metric and (int(d.get("num_segments_per_speaker", 0)) < 2 or int(d.get("num_speakers_per_batch", 0)) < 2):
        raise ValueError("%s needs num_speakers_per_batch >= 2 and num_segments_per_speaker >= 2 (a negative and a positive "
                         "pair in every batch), got %s and %s" % (d.get("loss_func"), d.get("num_speakers_per_batch"),
                                                                  d.get("num_segments_per_speaker")))
    if d.get("pooling_type") == "self_attention":
        from . import att_train
        att_train.check_supported(params, True, metric)
        kind = "attention"
    elif d.get("network_type") == "resnet_18":
        from . import resnet_train
        resnet_train.check_supported(params, metric)
        kind = "resnet"
    else:
        from . import conv_train
        conv_train.check_supported(params, metric)
        kind = "conv"
    from . import tail_train
    tail_train.check_supported(params, metric)
    return kind, metric


def build_trainer(params, weights, num_classes, device=0, seed=0, batch_norm="batch"):
    """The trainer of the configuration on `weights`, the head from the weights' own softmax/output/* (fresh_weights' or a
    checkpoint's)."""
    kind, metric = check_supported(params)
    kernel, bias = (None, None) if metric else (weights.get(model_io.SOFTMAX_KERNEL), weights.get(model_io.SOFTMAX_BIAS))
    if kind == "attention":
        from .att_train import AttConvTrainer as make
    elif kind == "resnet":
        from .resnet_train import ResNetTrainer as make
    else:
        from .conv_train import ConvTrainer as make
    return make(params, weights, num_classes, device, seed, kernel, bias, batch_norm, metric)


def feature_dim(train_dir, params):
    """FeatureReader(train_dir).get_dim() (train.py:80-82): the columns of the first matrix of feats.scp, or selected_dim."""
    d = params if isinstance(params, dict) else params.dict
    if "selected_dim" in d:
        return int(d["selected_dim"])
    from .kaldi_io import read_mat
    from .native_ark import read_scp_table
    table = read_scp_table(os.path.join(train_dir, "feats.scp"))
    if not table:
        raise IOError("%s/feats.scp is empty" % train_dir)
    return int(read_mat(table[0][1]).shape[1])


# ---------------------------------------------------------------------------------------------- checkpoints, continuing
def optimizer_path(nnet, step):
    return os.path.join(nnet, "optimizer-%d.npz" % step)


def save_optimizer(nnet, step, state):
    os.makedirs(nnet, exist_ok=True)
    np.savez(optimizer_path(nnet, step), **state)


def load_optimizer(nnet, step):
    """The optimizer file of checkpoint `step`; a missing one is an error that names it, not a cold start."""
    path = optimizer_path(nnet, step)
    if not os.path.isfile(path):
        raise FileNotFoundError("%s is missing: -c continues with the optimizer's state of checkpoint model-%d and does not "
                                "start it cold" % (path, step))
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def prune_checkpoints(nnet, keep):
    """keep_checkpoint_max: remove all but the `keep` newest model-<step>.npz / optimizer-<step>.npz pairs."""
    steps = sorted(int(m.group(1)) for m in (re.fullmatch(r"model-(\d+)\.npz", os.path.basename(p))
                                             for p in glob.glob(os.path.join(nnet, "model-*.npz"))) if m)
    for step in steps[:-int(keep)] if keep and int(keep) > 0 else []:
        for path in (os.path.join(nnet, "model-%d.npz" % step), optimizer_path(nnet, step)):
            if os.path.isfile(path):
                os.remove(path)


def read_valid_loss_file(path):
    """[(epoch, loss, eer)] of a valid_loss file."""
    out = []
    with open(path, "r") as f:
        for line in f:
            if line.strip():
                epoch, loss, eer = line.split()
                out.append((int(epoch), float(loss), float(eer)))
    return out


def rule_defaults(params):
    """train.py:108-115: the defaults of the training script (early_stop_epochs 10, where finetune.py has 5)."""
    d = dict(params if isinstance(params, dict) else params.dict)
    d.setdefault("early_stop_epochs", 10)
    d.setdefault("min_learning_rate", 1e-5)
    d.setdefault("lr_start_decay_epoch", 0)
    d.setdefault("learning_rate_reduce_factor", 2)
    return d


def make_rule(params, nnet=None, start_epoch=0):
    """The LearningRateRule of a run (train.py:54-78, 89-92) -> (rule, number of epochs).  With `nnet` and start_epoch > 0 the
    state of a run that stopped is rebuilt from its files: the validation losses of nnet/valid_loss are played through the rule
    again (they give the minimum, its epoch and the shifts a reduction made), and the rates are those of nnet/learning_rate,
    which must hold start_epoch + 1 of them (train.py:76).  The files hold six decimals: two losses closer than that compare as
    equal here."""
    d = rule_defaults(params)
    learning_rate = d["learning_rate"]
    num_epochs = int(d["num_epochs"])
    if os.path.isfile(str(learning_rate)):
        schedule = head_train.read_learning_rate_file(str(learning_rate))
        if num_epochs >= len(schedule):
            num_epochs = len(schedule) - 1
        return head_train.LearningRateRule(d, schedule[0], schedule), num_epochs
    assert float(learning_rate) > 0, "The learning rate should be a number greater than 0 if it is not a file"
    rule = head_train.LearningRateRule(d, learning_rate)
    if nnet is not None and start_epoch > 0:
        path = os.path.join(nnet, "valid_loss")
        history = read_valid_loss_file(path) if os.path.isfile(path) else []
        if [e for e, _, _ in history[:start_epoch]] != list(range(start_epoch)):
            raise ValueError("%s does not hold the epochs 0 .. %d the checkpoint has behind it" % (path, start_epoch - 1))
        for epoch, loss, _ in history[:start_epoch]:
            rule.after(epoch, loss)
        path = os.path.join(nnet, "learning_rate")
        if os.path.isfile(path):
            rates = head_train.read_learning_rate_file(path)
            assert len(rates) >= start_epoch + 1, "Not enough learning rates in the learning_rate file."
            rule.rates = rates[:start_epoch + 1]
    return rule, num_epochs


def _regularization(head):
    """sum over the trained kernels of l2 / 2 |w|^2 (tf.contrib.layers.l2_regularizer), for the log line."""
    total = 0.0
    for name, w, _, _ in head.tensors():
        if head.l2[name] > 0:
            total += 0.5 * head.l2[name] * float((w.double() ** 2).sum())
    return total


# ---------------------------------------------------------------------------------------------- the driver
def train(train_dir, train_spklist, valid_dir, valid_spklist, model_dir, config=None, cont=False, seed=None, prefetch=2, device=0,
          batch_norm="batch", precision=None, log=None, on_step=None, num_gpus=1, channels=512, width=64):
    """The function behind the command (the module's docstring).  config: a JSON path, a dict or a Params; with cont it defaults
    to <model_dir>/nnet/config.json.  log(line) receives the progress lines, on_step(step, StepResult) every step's result.
    -> [(epoch, step, valid loss, eer, learning rate)] of the epochs this call finished."""
    if int(num_gpus) != 1:
        raise NotImplementedError("num_gpus %d: training on more than one GPU is not implemented" % int(num_gpus))
    if batch_norm not in ("moving", "batch"):
        raise ValueError("batch_norm must be moving or batch, got %r" % (batch_norm,))
    from . import train_input
    from . import valid as valid_mod
    nnet = os.path.join(model_dir, "nnet")
    if config is None:
        if not cont:
            raise ValueError("a configuration is needed unless the run continues (-c)")
        config = os.path.join(nnet, "config.json")
    params = config if isinstance(config, Params) else (Params(**dict(config)) if isinstance(config, dict) else Params(config))
    p = params.dict
    given = dict(p)            # what config.json holds: a Trainer writes its defaults into the params it is built with
    kind, metric = check_supported(params)                                    # before anything is written
    if p.get("sample_with_prob"):
        raise NotImplementedError("sample_with_prob is not implemented")
    seed = int(p.get("seed", 0)) if seed is None else int(seed)
    spe = int(p["num_steps_per_epoch"])
    _, num_classes = valid_mod.read_speaker_info(train_dir, train_spklist)
    dim = feature_dim(train_dir, params)
    step = 0
    if cont:
        weights, step = model_io.load_weights(nnet)
        if weights is None:
            raise RuntimeError("Cannot load checkpoint from %s" % nnet)
        state = load_optimizer(nnet, step)
    else:
        weights = fresh_weights(params, dim, num_classes, seed, channels, width)
    start_epoch = step // spe if spe > 0 else 0
    rule, num_epochs = make_rule(params, nnet if cont else None, start_epoch)
    os.makedirs(nnet, exist_ok=True)
    with open(os.path.join(nnet, "config.json"), "w") as f:
        json.dump(given, f, indent=2)
    with open(os.path.join(nnet, "feature_dim"), "w") as f:
        f.write("%d\n" % dim)
    head = build_trainer(params, weights, num_classes, device, seed, batch_norm)
    if cont:
        head.load_optimizer_state(state)
    loader = train_input.Loader(train_dir, train_spklist, params, seed, dim, device, prefetch)
    show = int(p.get("show_training_progress", 0) or 0)
    save_steps = int(p.get("save_checkpoints_steps", 0) or 0)
    keep = p.get("keep_checkpoint_max")

    def variables():
        out = dict(weights)
        out.update(head.variables())
        return out

    history = []
    for epoch in range(start_epoch, num_epochs):
        lr = rule.rate(epoch)
        if log is not None:
            log("Epoch %d, learning rate: %f" % (epoch, lr))
        t0 = time.time()
        for feats, offsets, labels, _ in loader.epoch(epoch, skip=step - epoch * spe):
            res = head.step(feats, offsets, labels, lr, global_step=step)
            step += 1
            done = step - epoch * spe                                         # steps of this epoch behind us
            if on_step is not None:
                on_step(step, res)
            if log is not None and show > 0 and (done - 1) % show == 0:
                t1 = time.time()
                log("Epoch: [%2d] step: [%2d/%2d] time: %.4f s/step, raw loss: %f, total loss: %f"
                    % (epoch, done - 1, spe, t1 - t0, res.loss, res.loss + _regularization(head)))
            t0 = time.time()
            if save_steps > 0 and done % save_steps == 0 and done != spe:     # trainer.py:664; the epoch's end writes its own
                save_optimizer(nnet, step, head.optimizer_state())
                model_io.save_model(model_dir, given, dim, variables(), step=step)
                prune_checkpoints(nnet, keep)
        save_optimizer(nnet, step, head.optimizer_state())
        valid_loss, eer, new_lr, stop = head_train.finish_epoch(Params(**dict(given)), dim, model_dir, variables(), step, epoch, rule,
                                                                valid_dir, valid_spklist, device, precision, metric)
        prune_checkpoints(nnet, keep)
        history.append((epoch, step, valid_loss, eer, lr))
        if log is not None:
            log("[INFO] Valid loss: %f, EER: %f, next learning rate %.8f" % (valid_loss, eer, new_lr))
        if stop:
            break
    return history


def build_parser():
    parser = argparse.ArgumentParser(description="Train a network from scratch (nnet/lib/train.py).")
    parser.add_argument("-c", "--cont", action="store_true", help="Continue training from the last checkpoint of model_dir.")
    parser.add_argument("--config", type=str, default="", help="The configuration file (with -c: default <model_dir>/nnet/config.json).")
    parser.add_argument("-g", "--gpu", type=int, default=-1, help="The GPU id (-1: LOCAL_RANK or 0; there is no CPU path).")
    parser.add_argument("-n", "--num-gpus", type=int, default=1, help="More than one GPU is refused.")
    parser.add_argument("--seed", type=int, default=-1, help="Seed of the initial values and of the batches (default: params.seed or 0).")
    parser.add_argument("--prefetch", type=int, default=2, help="Batches staged and decoded ahead of the step (0: inline).")
    parser.add_argument("--batch-norm", choices=("batch", "moving"), default="batch", help="batch = the reference's is_training=True "
                        "(default); moving = inference-mode batch norm with constant moving statistics.")
    parser.add_argument("--precision", type=str, default="", help="f32 | bf16x3 | f16x3 | f16f6 of the validation forward.")
    parser.add_argument("train_dir", type=str, help="The data directory of the training set.")
    parser.add_argument("train_spklist", type=str, help="The spklist file maps the TRAINING speakers to the indices.")
    parser.add_argument("valid_dir", type=str, help="The data directory of the validation set.")
    parser.add_argument("valid_spklist", type=str, help="The spklist maps the VALID speakers to the indices.")
    parser.add_argument("model", type=str, help="The output model directory.")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.num_gpus != 1:
        parser.error("-n %d: training on more than one GPU is not implemented" % args.num_gpus)
    config = args.config or (os.path.join(args.model, "nnet", "config.json") if args.cont else "")
    if not config or not os.path.isfile(config):
        sys.exit("Cannot find the configuration %s" % (config or "(give --config)"))
    device = args.gpu if args.gpu >= 0 else int(os.environ.get("LOCAL_RANK", 0))
    try:
        history = train(args.train_dir, args.train_spklist, args.valid_dir, args.valid_spklist, args.model, config=config,
                        cont=args.cont, seed=args.seed if args.seed >= 0 else None, prefetch=args.prefetch, device=device,
                        batch_norm=args.batch_norm, precision=args.precision or None, log=print)
    except NotImplementedError as e:
        sys.exit("[ERROR] %s" % e)
    for epoch, step, loss, eer, lr in history:
        print("epoch %d step %d loss %f eer %f lr %.8f" % (epoch, step, loss, eer, lr))
    return 0


if __name__ == "__main__":
    sys.exit(main())
