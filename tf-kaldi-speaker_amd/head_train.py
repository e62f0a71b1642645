"""Train a new classifier head on a frozen encoder: stage one of every fine-tune
(egs/voxceleb/v1/nnet/lib/finetune.py:6-7: "If a new softmax layer is added to the pre-trained layer, it is better to train the
new softmax first and then update the entire network").

Everything below the loss layer stays as the pre-trained checkpoint has it, so a step is: the frozen forward to the `output`
endpoint (Trainer.predict), one xv_loss_classifier_grad (csrc/loss_grad.hip: loss and the gradients of the four softmax-family
heads), one xv_opt_step per tensor (csrc/opt_step.hip: l2, tf.clip_by_norm, sgd / momentum / adam as TensorFlow 1.x applies
them).  The encoder runs in INFERENCE mode: moving batch-norm statistics, no dropout.  The reference's `noupdate_var_list`
route feeds is_training=True to the whole graph, so its frozen layers still normalise with batch statistics (and update their
moving averages); with the encoder frozen here the head is trained on the embeddings extraction will later produce.

plan_train_batches stands in for KaldiDataRandomQueue (dataset/data_loader.py:289-356), made deterministic: **parity
unpinned**, like valid.plan_end2end_batches.  No CPU path: HeadTrainer needs a HIP device; plan_train_batches, xavier_uniform
and LearningRateRule are pure host code."""
import collections
import os

import numpy as np

from . import _lib
from ._lib import ptr
from . import losses
from . import model_io

TrainBatch = collections.namedtuple("TrainBatch", "keys rxfiles labels length starts")
StepResult = collections.namedtuple("StepResult", "loss accuracy")

_KINDS = {"sgd": _lib.XV_OPT_SGD, "momentum": _lib.XV_OPT_MOMENTUM, "adam": _lib.XV_OPT_ADAM}


def xavier_uniform(embed_dim, num_classes, seed=0):
    """tf.contrib.layers.xavier_initializer() on [E, C] (model/loss.py:130; the glorot_uniform default of tf.layers.dense has the
    same limit): uniform in +-sqrt(6 / (E + C)), drawn from numpy.random.RandomState(seed)."""
    limit = np.sqrt(6.0 / (int(embed_dim) + int(num_classes)))
    return np.random.RandomState(seed).uniform(-limit, limit, (int(embed_dim), int(num_classes))).astype(np.float32)


def optimizer_config(params):
    """-> (kind id, momentum, use_nesterov, l2 of the kernel, clip_norm) from the params the reference reads
    (model/trainer.py:225-246 make_optimizer, :529-533 clip_gradient, model/loss.py:26-28)."""
    d = params if isinstance(params, dict) else params.dict
    name = d.get("optimizer", "sgd")                        # trainer.py:226-228
    if name not in _KINDS:
        raise ValueError("Optimizer %s is not supported." % name)
    if name == "sgd" and "momentum" in d:
        raise ValueError("Using sgd as the optimizer and you should not specify the momentum.")
    momentum = float(d["momentum"]) if name == "momentum" else 0.0
    nesterov = bool(d.get("use_nesterov", False)) if name == "momentum" else False
    l2 = float(d["output_weight_l2_regularizer"] if "output_weight_l2_regularizer" in d else d.get("weight_l2_regularizer", 0.0))
    clip = float(d["clip_gradient_norm"]) if d.get("clip_gradient") else 0.0
    if l2 < 0 or clip < 0:
        raise ValueError("weight_l2_regularizer and clip_gradient_norm must not be negative")
    return _KINDS[name], momentum, nesterov, l2, clip


class HeadTrainer(object):
    """The raw class rows [C, ldc] (the transpose of `softmax/output/kernel`), the bias (plain softmax only) and the optimizer
    slots on the device.  Without `kernel` the layer starts as the reference starts a variable the checkpoint does not hold:
    Xavier uniform from RandomState(seed), zero bias."""

    def __init__(self, params, embed_dim, num_classes, device=0, seed=0, kernel=None, bias=None):
        d = params if isinstance(params, dict) else params.dict
        func = losses.head_config(params, 0, False)[0]           # NotImplementedError: other losses, aux_loss_func, asoftmax m
        if d.get("sample_with_prob"):
            raise NotImplementedError("sample_with_prob is not implemented")
        self.kind, self.momentum, self.nesterov, self.l2, self.clip_norm = optimizer_config(params)
        embed_dim, num_classes = int(embed_dim), int(num_classes)
        if embed_dim < 1 or embed_dim > 2048 or num_classes < 1:
            raise ValueError("embed_dim must lie in [1, 2048] and num_classes be positive, got %d and %d" % (embed_dim, num_classes))
        if kernel is None:
            kernel = xavier_uniform(embed_dim, num_classes, seed)
        if tuple(kernel.shape) != (embed_dim, num_classes):
            raise ValueError("kernel: expected [%d, %d], got shape %s" % (embed_dim, num_classes, tuple(kernel.shape)))
        if func == "softmax" and bias is None:
            bias = np.zeros(num_classes, dtype=np.float32)
        self.params, self.loss_func = params, func
        self.head = losses.ClassifierHead(kernel, bias, params, device)      # holds the raw rows and the bias: the parameters
        torch = losses._need_device()
        self._torch, self._lib, self.device = torch, _lib.load(), int(device)
        rows = self.head.raw_rows
        with torch.cuda.device(self.device):
            self._grad_rows = torch.zeros_like(rows)                        # the padding columns stay zero
            self._grad_bias = None if self.head.bias is None else torch.zeros_like(self.head.bias)
            slots = {_lib.XV_OPT_SGD: 0, _lib.XV_OPT_MOMENTUM: 1, _lib.XV_OPT_ADAM: 2}[self.kind]
            self._row_slots = [torch.zeros_like(rows) for _ in range(slots)]
            self._bias_slots = [] if self.head.bias is None else [torch.zeros_like(self.head.bias) for _ in range(slots)]
            self._ws = torch.empty(max(int(self._lib.xv_opt_workspace(rows.numel())), 8), dtype=torch.uint8, device=rows.device)
        self.num_steps = 0                                                   # adam's t

    def _apply(self, w, g, slots, lr, l2):
        stream = _lib.stream(self.device)
        _lib.check(self._lib.xv_opt_step(self.device, self.kind, int(self.nesterov), ptr(w), ptr(g), ptr(slots[0]) if slots else None,
                                         ptr(slots[1]) if len(slots) > 1 else None, w.numel(), float(lr), l2, self.clip_norm,
                                         self.momentum, self.num_steps, ptr(self._ws), self._ws.numel(), stream))

    def step(self, x, labels, learning_rate, global_step=0):
        """One training step on a batch of embeddings x [n, E]: the mean loss of the head at `global_step` (its margin annealing),
        its gradients, then l2 (kernel only), the per-tensor clip and the update -> StepResult(mean loss, top-1 accuracy), both
        of the parameters BEFORE the update."""
        torch = self._torch
        with torch.cuda.device(self.device):
            out, top1, _, _, _ = self.head._grad_device(x, labels, global_step, None, False, self._grad_rows, self._grad_bias)
            self.num_steps += 1
            self._apply(self.head.raw_rows, self._grad_rows, self._row_slots, learning_rate, self.l2)
            if self.head.bias is not None:
                self._apply(self.head.bias, self._grad_bias, self._bias_slots, learning_rate, 0.0)
            n = int(out.shape[1])
            lab = losses._labels_dev(labels, n, out.device, torch)
            return StepResult(float(out[0].double().mean()) if n else float("nan"),
                              float((top1 == lab).double().mean()) if n else float("nan"))

    def kernel(self):
        """`softmax/output/kernel` [E, C], float32 numpy."""
        return np.ascontiguousarray(self.head.raw_rows[:, :self.head.embed_dim].t().cpu().numpy())

    def bias(self):
        """`softmax/output/bias` [C] or None."""
        return None if self.head.bias is None else self.head.bias.cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------- batches
def plan_train_batches(data, spklist, params, seed, epoch):
    """`num_steps_per_epoch` batches of num_speakers_per_batch x num_segments_per_speaker chunks, a deterministic stand-in for
    KaldiDataRandomQueue (dataset/data_loader.py:289-356; the reference seeds its workers from os.urandom): **parity unpinned**.
    From numpy.random.RandomState([seed, epoch]), per batch and in this order: one length from [min_segment_len,
    max_segment_len]; speakers one by one, without replacement, a speaker with no utterance of at least that length being
    redrawn (ValueError when fewer than num_speakers_per_batch qualify); per speaker num_segments_per_speaker utterances among
    those long enough, with replacement, each with a uniform start in [0, frames - length].  Rows are speaker-major and the
    label is the speaker's index -> [TrainBatch(keys, rxfiles, labels, length, starts)]."""
    from . import valid as valid_mod
    p = params if isinstance(params, dict) else params.dict
    n_spk, n_seg = int(p["num_speakers_per_batch"]), int(p["num_segments_per_speaker"])
    lo, hi, steps = int(p["min_segment_len"]), int(p["max_segment_len"]), int(p["num_steps_per_epoch"])
    if n_spk < 1 or n_seg < 1 or lo < 1 or hi < lo or steps < 0:
        raise ValueError("bad batch parameters: %d speakers x %d segments, lengths [%d, %d], %d steps" % (n_spk, n_seg, lo, hi, steps))
    if p.get("sample_with_prob"):
        raise NotImplementedError("sample_with_prob is not implemented")
    spk2features, _ = valid_mod.read_speaker_info(data, spklist)
    frames = valid_mod.read_utt2num_frames(data)
    speakers = sorted(spk2features)
    rs = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(epoch)])
    out = []
    for _ in range(steps):
        length = int(rs.randint(lo, hi + 1))
        pool = list(speakers)
        keys, rxfiles, labels, starts = [], [], [], []
        chosen = 0
        while chosen < n_spk:
            if not pool:
                raise ValueError("%d speakers have an utterance of at least %d frames, a batch needs %d" % (chosen, length, n_spk))
            spk = pool.pop(int(rs.randint(len(pool))))
            utts = [(key, rx) for key, rx in spk2features[spk] if frames[key] >= length]
            if not utts:
                continue                                         # redrawn
            for _ in range(n_seg):
                key, rx = utts[int(rs.randint(len(utts)))]
                keys.append(key)
                rxfiles.append(rx)
                labels.append(spk)
                starts.append(int(rs.randint(frames[key] - length + 1)))
            chosen += 1
        out.append(TrainBatch(keys, rxfiles, np.array(labels, dtype=np.int32), length, starts))
    return out


def read_train_batch(batch, dim):
    """-> float32 [B, length, dim]: frames [start, start + length) of every chunk.  Every utterance is read from its archive
    when it is drawn and dropped once its chunk is copied: nothing is kept between chunks, so host memory stays at one batch plus
    one utterance whatever the size of the training set.  (kaldi_io.read_mat decodes a whole matrix: compressed archives and
    piped rxfiles have no row access.)"""
    from .kaldi_io import read_mat
    out = np.zeros((len(batch.keys), batch.length, dim), dtype=np.float32)
    for j, (key, rx, start) in enumerate(zip(batch.keys, batch.rxfiles, batch.starts)):
        mat = read_mat(rx)
        if mat.shape[1] < dim:
            raise ValueError("%s: features have %d columns, the network needs %d" % (key, mat.shape[1], dim))
        if mat.shape[0] < start + batch.length:
            raise ValueError("%s: %d frames in the archive, utt2num_frames promised at least %d" % (key, mat.shape[0], start + batch.length))
        out[j] = mat[start:start + batch.length, :dim]
    return out


# ---------------------------------------------------------------------------------------------- learning rate
class LearningRateRule(object):
    """The per-epoch rule of finetune.py:125-132, 154-172, 185-191 as a state machine: after(epoch, valid_loss) -> (the learning
    rate of epoch + 1, stop).  With `schedule` (the rates of a learning-rate file, :74-86) the rates are read off and nothing
    stops early."""

    def __init__(self, params, learning_rate, schedule=None):
        d = params if isinstance(params, dict) else params.dict
        self.reduce_lr_epochs = d.get("reduce_lr_epochs")
        self.factor = d.get("learning_rate_reduce_factor", 2)
        self.start_decay_epoch = d.get("lr_start_decay_epoch", 0)
        self.min_learning_rate = d.get("min_learning_rate", 1e-5)
        self.early_stop_epochs = d.get("early_stop_epochs", 5)
        self.schedule = None if schedule is None else [float(v) for v in schedule]
        if self.schedule is None and self.reduce_lr_epochs is None:
            raise KeyError("reduce_lr_epochs: the config must set it unless learning_rate names a file")
        self.rates = [float(learning_rate)] if self.schedule is None else list(self.schedule)
        self.min_loss, self.min_loss_epoch = 1e16, -1                   # misc/utils.py ValidLoss

    def rate(self, epoch):
        return self.rates[epoch]

    def after(self, epoch, valid_loss):
        if self.schedule is not None:
            return self.rates[epoch + 1], False
        new = self.rates[epoch]
        if valid_loss < self.min_loss:
            self.min_loss, self.min_loss_epoch = valid_loss, epoch
        elif epoch - self.min_loss_epoch >= self.reduce_lr_epochs and epoch >= self.start_decay_epoch:
            new /= self.factor
            self.min_loss_epoch += self.reduce_lr_epochs / 2          # finetune.py:168 (true division)
        self.rates.append(new)
        stop = new < (self.min_learning_rate - 1e-12) or epoch - self.min_loss_epoch >= self.early_stop_epochs
        return new, stop


def read_learning_rate_file(path):
    """finetune.py:74-81: `epoch rate` or `rate` per line."""
    out = []
    with open(path, "r") as f:
        for line in f:
            fields = line.strip().split(" ")
            out.append(float(fields[1]) if len(fields) > 1 else float(fields[0]))
    return out


# ---------------------------------------------------------------------------------------------- the driver
BATCH_NORM_ALONE = ("--batch-norm batch needs --segment-layers, --frame-layers or --conv-layers: the head has no batch norm, and "
                    "everything in front of it is frozen")


def _frame_step(trainer, head, feats, labels, lr, step):
    """One FrameTrainer step on the batch feats [B, T, dim]: the frozen forward to trainer.embeddings (a frame-level node) hands
    its packed rows over on the device; utterance b owns out_rows / B of them (T less the node's context)."""
    if not trainer.is_loaded:
        trainer._lazy_load()
    torch = trainer._torch
    b, t, d = feats.shape
    with torch.cuda.device(trainer._device_index):
        dev = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32).reshape(b * t, d)).to("cuda:%d" % trainer._device_index)
        offsets = np.arange(b + 1, dtype=np.int32) * t
        frames = trainer.predict_packed(dev, offsets)
        try:                                             # the range guard of the fp16 precisions, as Trainer.predict applies it
            trainer.raise_on_flags(trainer.check_overflow())
        except FloatingPointError as e:
            if not trainer._range_fallback:
                raise
            frames = trainer._fallback_trainer(str(e)).predict_packed(dev, offsets, trainer.embeddings)
        per = int(frames.shape[0]) // b
        if per * b != int(frames.shape[0]) or per < 1:
            raise RuntimeError("%s returned %d rows for %d chunks of %d frames" % (trainer.embeddings, int(frames.shape[0]), b, t))
        return head.step(frames, np.arange(b + 1, dtype=np.int64) * per, labels, lr, global_step=step)


def _conv_step(trainer, head, feats, labels, lr, step):
    """One ConvTrainer step on the batch feats [B, T, dim]: the packed features go straight in, there is no frozen forward."""
    if not trainer.is_loaded:
        trainer._lazy_load()
    torch = trainer._torch
    b, t, d = feats.shape
    with torch.cuda.device(trainer._device_index):
        dev = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32).reshape(b * t, d)).to("cuda:%d" % trainer._device_index)
        return head.step(dev, np.arange(b + 1, dtype=np.int64) * t, labels, lr, global_step=step)


def finish_epoch(params, dim, out_model_dir, variables, step, epoch, rule, valid_dir, valid_spklist, device, precision, metric):
    """The tail of an epoch, of train_head and of train.train: write model-<step>.npz (model_io.save_model), judge the written
    directory (Trainer.valid, or valid.metric_valid behind the metric door), scoring.pairwise_eer, rule.after, and one line each
    in valid_loss and learning_rate in finetune.py's formats -> (valid loss, eer, the next learning rate, stop)."""
    from . import scoring
    from . import valid as valid_mod
    from .trainer import Trainer
    p = params.dict
    nnet = os.path.join(out_model_dir, "nnet")
    model_io.save_model(out_model_dir, p, dim, variables, step=step)
    judge = Trainer(params, out_model_dir, dim, single_cpu=True, device=device, precision=precision)
    if metric:
        valid_loss, emb, labels = valid_mod.metric_valid(judge, valid_dir, valid_spklist,
                                                         batch_type=p.get("batch_type", "softmax"), output_embeddings=True)
    else:
        judge.build("valid")
        valid_loss, emb, labels = judge.valid(valid_dir, valid_spklist, batch_type=p.get("batch_type", "softmax"),
                                              output_embeddings=True)
    judge.close()
    eer = scoring.pairwise_eer(emb, labels, device=device)[0]
    new_lr, stop = rule.after(epoch, valid_loss)
    if epoch == 0:
        with open(os.path.join(nnet, "learning_rate"), "a") as f:
            f.write("0 %.8f\n" % rule.rate(0))
    with open(os.path.join(nnet, "learning_rate"), "a") as f:
        f.write("%d %.8f\n" % (epoch + 1, new_lr))
    with open(os.path.join(nnet, "valid_loss"), "a") as f:
        f.write("%d %f %f\n" % (epoch, valid_loss, eer))
    return valid_loss, eer, new_lr, stop


METRIC_HEAD_ONLY = ("loss_func %s has no classifier layer: there is no head to train; give --segment-layers, --frame-layers or "
                    "--conv-layers")


def train_head(trainer, train_dir, train_spklist, valid_dir, valid_spklist, out_model_dir, weights=None, seed=0, keep_head=False,
               precision=None, log=None, segment_layers=False, frame_layers=False, conv_layers=False, batch_norm="moving"):
    """Train the head of `trainer` (a Trainer built for "predict" with the pre-trained weights loaded; its params name the head,
    the optimizer and the schedule) on train_dir and write <out_model_dir>/nnet after every epoch of num_steps_per_epoch steps:
    model-<step>.npz (model_io.save_model: every variable of `weights` unchanged plus the new softmax/output/kernel and bias),
    config.json, feature_dim, and one line each in valid_loss (`epoch loss eer`) and learning_rate (`epoch rate`) in
    finetune.py's formats (:174-183).  Validation is the existing Trainer.valid + scoring.pairwise_eer on the new directory.
    `weights` defaults to the trainer's checkpoint; keep_head starts from its softmax kernel when the shape fits.
    With segment_layers the frozen forward stops at the `pooling` node and the two segment-level layers behind it are trained
    with the head (tail_train.TailTrainer): the checkpoints then also hold their new kernels, biases, gamma and beta; every
    other variable, their moving statistics included, is unchanged.
    With frame_layers (which implies segment_layers) the frozen forward stops at frame_train.frozen_node (tdnn3_relu, or
    tdnn7_relu for the extended TDNN): its packed frames stay on the device (Trainer.predict_packed) and the 1-tap frame layers
    behind it, the statistics pooling, the segment-level layers and the head are trained by frame_train.FrameTrainer.  The
    checkpoints then hold the new frame-layer kernels, biases, gamma and beta as well.
    With conv_layers (which implies the other two) nothing is frozen: conv_train.ConvTrainer trains every frame-level layer, the
    multi-tap convolutions included, on the packed features, in exact fp32 whatever `precision` says.  The checkpoints then hold
    the new convolution kernels in the shape the input had, and biases, gamma and beta; the moving statistics and every other
    variable are unchanged.
    On a ResNet-18 conv_layers goes to resnet_train.ResNetTrainer (after resnet_train.check_supported): every 2-D convolution,
    conv5, dense1 and dense2 are trained as well, the convolutions' kernels written in their HWIO shape; frame_layers alone stays
    refused there.
    On a self_attention model frame_layers and conv_layers go to att_train.AttFrameTrainer / AttConvTrainer (after
    att_train.check_supported): the key and value networks and the query are trained and written as well.
    batch_norm="batch" (with any of the three; alone it is refused, the head has no batch norm) runs the batch norms of the
    trained layers in training mode (tail_train.batch_stats_options): the checkpoints then also hold their moving_mean and
    moving_variance, and the validation after each epoch, the unchanged Trainer.valid on the written checkpoint, normalises with
    them.  The default "moving" changes nothing.
    With `semihard_triplet_loss` or `angular_triplet_loss` (valid.METRIC_LOSSES) the trainers are built through their metric
    door (tail_train.check_supported): there is no classifier layer, so at least one of the three layer switches is needed and
    keep_head means nothing; a batch needs two speakers and two segments of each (a negative and a positive); every variable
    of `weights`, any softmax/output/* included, is written back unchanged unless a layer trains it; and each epoch's checkpoint
    is judged by valid.metric_valid (e2e_valid_loss for the angular triplet loss, as save_and_set_valid_loss decides).
    -> [(epoch, step, valid loss, eer, learning rate)]."""
    if batch_norm not in ("moving", "batch"):
        raise ValueError("batch_norm must be moving or batch, got %r" % (batch_norm,))
    if batch_norm == "batch" and not (segment_layers or frame_layers or conv_layers):
        raise ValueError(BATCH_NORM_ALONE)
    from . import valid as valid_mod
    params = trainer.params
    p = params.dict
    metric = p.get("loss_func") in valid_mod.METRIC_LOSSES
    if metric:
        if not (segment_layers or frame_layers or conv_layers):
            raise ValueError(METRIC_HEAD_ONLY % p.get("loss_func"))
        if int(p.get("num_segments_per_speaker", 0)) < 2 or int(p.get("num_speakers_per_batch", 0)) < 2:
            raise ValueError("%s needs num_speakers_per_batch >= 2 and num_segments_per_speaker >= 2 (a negative and a positive "
                             "pair in every batch), got %s and %s" % (p.get("loss_func"), p.get("num_speakers_per_batch"),
                                                                      p.get("num_segments_per_speaker")))
    if weights is None:
        weights, _ = model_io.load_weights(trainer.model)
        if weights is None:
            raise RuntimeError("Cannot find a checkpoint in %s" % trainer.model)
    _, num_classes = valid_mod.read_speaker_info(train_dir, train_spklist)
    learning_rate = p["learning_rate"]
    schedule = read_learning_rate_file(str(learning_rate)) if os.path.isfile(str(learning_rate)) else None
    num_epochs = int(p["num_epochs"])
    if schedule is not None and num_epochs >= len(schedule):
        num_epochs = len(schedule) - 1                                   # finetune.py:82-83; every epoch needs the next rate
    if schedule is None:
        assert float(learning_rate) > 0, "The learning rate should be a number greater than 0 if it is not a file"
    rule = LearningRateRule(params, learning_rate if schedule is None else schedule[0], schedule)

    endpoint = trainer.embeddings
    attention = (conv_layers or frame_layers) and p.get("pooling_type") == "self_attention"
    if attention:                                                        # the attention trainers of att_train.py, same steps
        from . import att_train
        att_train.check_supported(params, conv_layers, metric)           # before the trainer is touched
    resnet = bool(conv_layers) and not attention and p.get("network_type") == "resnet_18"
    if resnet:                                                           # resnet_train.py: the grid convolutions and the blocks
        from . import resnet_train
        resnet_train.check_supported(params, metric)                     # before the trainer is touched
        segment_layers = frame_layers = True
    elif conv_layers:
        from . import conv_train
        if not attention:
            conv_train.check_supported(params, metric)                   # before the trainer is touched
        segment_layers = frame_layers = True
    elif frame_layers:
        from . import frame_train
        if not attention:
            frame_train.check_supported(params, metric)                  # before the trainer is touched
        segment_layers = True
        trainer.embeddings = frame_train.frozen_node(params)
    else:
        trainer.embeddings = "pooling" if segment_layers else "output"   # the caller's trainer gets its endpoint back on exit
    try:
        if segment_layers:
            from . import tail_train
            tail_train.check_supported(params, metric)
            embed_dim = int(weights[tail_train.segment_variables(params)[1].kernel].shape[1])
        else:
            probe = trainer.predict(np.zeros((1, int(p["min_segment_len"]), trainer.dim), dtype=np.float32))
            embed_dim = int(probe.shape[-1])
        kernel = bias = None
        if keep_head and not metric:
            k = weights.get(model_io.SOFTMAX_KERNEL)
            if k is not None and tuple(k.shape) == (embed_dim, num_classes):
                kernel, bias = np.asarray(k), weights.get(model_io.SOFTMAX_BIAS)
        if attention:
            make = att_train.AttConvTrainer if conv_layers else att_train.AttFrameTrainer
            head = make(params, weights, num_classes, trainer._device_index, seed, kernel, bias, batch_norm, metric)
        elif resnet:
            head = resnet_train.ResNetTrainer(params, weights, num_classes, trainer._device_index, seed, kernel, bias, batch_norm, metric)
        elif conv_layers:
            head = conv_train.ConvTrainer(params, weights, num_classes, trainer._device_index, seed, kernel, bias, batch_norm, metric)
        elif frame_layers:
            head = frame_train.FrameTrainer(params, weights, num_classes, trainer._device_index, seed, kernel, bias, batch_norm, metric)
        elif segment_layers:
            head = tail_train.TailTrainer(params, weights, num_classes, trainer._device_index, seed, kernel, bias, batch_norm, metric)
        else:
            head = HeadTrainer(params, embed_dim, num_classes, trainer._device_index, seed, kernel, bias)
        # the metric door trains no head: whatever softmax/output/* the checkpoint holds is kept as it is
        frozen = dict(weights) if metric else {k: v for k, v in weights.items()
                                               if k not in (model_io.SOFTMAX_KERNEL, model_io.SOFTMAX_BIAS)}
        history, step = [], 0
        for epoch in range(num_epochs):
            lr = rule.rate(epoch)
            for batch in plan_train_batches(train_dir, train_spklist, params, seed, epoch):
                feats = read_train_batch(batch, trainer.dim)
                if conv_layers:
                    res = _conv_step(trainer, head, feats, batch.labels, lr, step)
                elif frame_layers:
                    res = _frame_step(trainer, head, feats, batch.labels, lr, step)
                else:
                    res = head.step(trainer.predict(feats), batch.labels, lr, global_step=step)
                step += 1
                if log is not None:
                    log("epoch %d step %d loss %f acc %f" % (epoch, step, res.loss, res.accuracy))
            out = dict(frozen)
            if segment_layers:
                out.update(head.variables())
            else:
                out[model_io.SOFTMAX_KERNEL] = head.kernel()
                if head.bias() is not None:
                    out[model_io.SOFTMAX_BIAS] = head.bias()
            valid_loss, eer, new_lr, stop = finish_epoch(params, trainer.dim, out_model_dir, out, step, epoch, rule, valid_dir,
                                                         valid_spklist, trainer._device_index, precision or trainer._precision, metric)
            history.append((epoch, step, valid_loss, eer, lr))
            if log is not None:
                log("epoch %d valid loss %f eer %f next learning rate %.8f" % (epoch, valid_loss, eer, new_lr))
            if stop:
                break
        return history
    finally:
        trainer.embeddings = endpoint
