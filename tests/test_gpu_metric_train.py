"""Fine-tuning with the triplet losses (the metric door of the trainers, head_train.train_head and the train_head command): one
step of every trainer under `semihard_triplet_loss` and `angular_triplet_loss` ("all", amsoftmax) against a torch float64 model
of the same stack, a batch of 6 speakers x 4 segments; one sgd step ties the gradient to the forward on the device; the command
end to end.  Every gradient, updated variable, moved statistic and the inference forward is held to 1e-4 relative L2, the bar
of tests/test_gpu_bn_train.py and tests/test_gpu_att_train.py.  Precondition of every comparison, asserted on the CPU: the torch
model's decision margins (tests/helpers/ref_metric_grad.margins on its output rows) exceed 1e-6.

The torch model is TorchStack / AttTorchStack of those tests.  They end in cross_entropy(out @ K + b, labels); here K is the
identity, b zero and the stack's cross_entropy the metric loss, so the very same stacks run under the metric head."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_att_train as rat                                         # noqa: E402
import ref_loss_grad as rlg                                         # noqa: E402
import ref_metric_grad as rg                                        # noqa: E402
import test_gpu_att_train as att                                    # noqa: E402
from test_gpu_bn_train import HEAD_B, HEAD_K, TorchStack, device_grads, rel           # noqa: E402
from test_gpu_conv_train import CHANNELS, LENGTHS, POOL, small_model, toy_segments  # noqa: E402
from test_metric_grad_host import AM, torch_loss_of                 # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
SPEAKERS, SEGMENTS = 6, 4
RATE, MOMENTUM = 0.05, 0.5
EXTRA = dict(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=1e-3, batchnorm_momentum=MOMENTUM)
LOSSES = {"semihard": (dict(loss_func="semihard_triplet_loss", margin=0.2, triplet_loss_squared=False),
                       "semihard", dict(margin=0.2, squared=False, normalize=True)),
          "angular": (dict(loss_func="angular_triplet_loss", margin=0.2, triplet_type="all", loss_type=AM),
                      "all", dict(loss_type=AM, margin=0.2))}
LABELS = np.repeat(np.arange(SPEAKERS), SEGMENTS).astype(np.int32)


class _Functional(object):
    def __init__(self, loss):
        self.cross_entropy = loss

    def __getattr__(self, name):
        import torch
        return getattr(torch.nn.functional, name)


class _Torch(object):
    """torch, but for nn.functional.cross_entropy."""

    def __init__(self, loss):
        self.nn = types.SimpleNamespace(functional=_Functional(loss))

    def __getattr__(self, name):
        import torch
        return getattr(torch, name)


def metric_torch(stack, kind, o):
    """The stack's torch with cross_entropy replaced by the metric loss of the rows it is given (see the module's docstring)."""
    stack.torch = _Torch(lambda rows, labels: torch_loss_of(kind, rows, labels.numpy(), **o))
    return stack


def run_stack(stack, variables, x, offsets, labels, train, embed_dim):
    """TorchStack.run with the identity head -> (output rows, gradients without the head's, column sums of |gz|)."""
    full = dict(variables)
    full[HEAD_K], full[HEAD_B] = np.eye(embed_dim), np.zeros(embed_dim)
    y, grads, gz = stack.run(full, x, offsets, labels, train)
    if grads is not None:
        grads = {k: v for k, v in grads.items() if k not in (HEAD_K, HEAD_B)}
    return y, grads, gz


def make(which, loss, mode, optimizer=None):
    """-> (trainer, twin, weights, stack factory, x, offsets, step arguments as a function of the device rows)."""
    import torch
    from tf_kaldi_speaker_amd import att_train, conv_train, frame_train, synth, tail_train
    from tf_kaldi_speaker_amd.params import Params
    extra = dict(optimizer or EXTRA, **LOSSES[loss][0])
    r = np.random.RandomState(6)
    if which == "att":
        net, keys = att.MODELS["front-h1"]
        params = dict(synth.TDNN_STAT_PARAMS, network_type=net, **dict(att.EXTRA, **dict(keys, **extra)))
        weights = synth.synth_weights(params, att.DIM, seed=4, channels=att.CHANNELS)
        cls = att_train.AttConvTrainer
    else:
        params, weights = small_model(**extra)
        cls = dict(tail=tail_train.TailTrainer, frame=frame_train.FrameTrainer, conv=conv_train.ConvTrainer)[which]
    build = lambda: cls(Params(**params), weights, SPEAKERS, device=0, seed=3, batch_norm=mode, metric=True)      # noqa: E731
    trainer, twin = build(), build()
    if which == "tail":
        x = (r.standard_normal((LABELS.size, 2 * POOL)) + 0.5 * LABELS[:, None]).astype(np.float32)
        offsets, args = [0], lambda dev: (x,)
    elif which == "frame":
        lens = [(23, 31, 20, 36, 27, 29)[i % 6] for i in range(LABELS.size)]
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        x = np.maximum(r.standard_normal((int(offsets[-1]), CHANNELS)) + 0.3 * LABELS[np.repeat(np.arange(LABELS.size), lens)][:, None],
                       0.0).astype(np.float32)
        args = lambda dev: (dev, offsets)                             # noqa: E731
    else:
        x, offsets, labels = toy_segments(17, SPEAKERS, SEGMENTS, LENGTHS["tdnn"])
        assert np.array_equal(labels, LABELS)
        args = lambda dev: (dev, offsets)                             # noqa: E731
    bessel = {spec.kernel: layer.bessel for spec, layer in zip(trainer.specs, trainer.layers)}
    if which == "att":
        stack = rat.AttTorchStack(trainer, weights, bessel)
    else:
        stack = TorchStack(getattr(trainer, "frame_specs", ()), getattr(trainer, "tail", trainer).specs, weights, bessel, pool=which != "tail")
    dev = torch.from_numpy(x).cuda()
    return trainer, twin, weights, metric_torch(stack, *LOSSES[loss][1:]), x, offsets, args(dev)


def clear_margins(kind, o, rows, floor=1e-6):
    m = rg.margins(rg.grad(kind, rows, LABELS, **o))
    assert min(m.values()) > floor, "the torch model's output holds a near-tie: %s" % (m,)


CASES = [("tail", "moving"), ("frame", "moving"), ("conv", "moving"), ("conv", "batch"), ("att", "moving")]


@pytest.mark.parametrize("loss", sorted(LOSSES))
@pytest.mark.parametrize("which,mode", CASES, ids=["%s-%s" % c for c in CASES])
def test_one_step_against_torch(which, mode, loss):
    trainer, twin, weights, stack, x, offsets, args = make(which, loss, mode)
    kind, o = LOSSES[loss][1:]
    batch = mode == "batch"
    names = [n for n, _, _, _ in trainer.tensors()]
    before = {k: v for k, v in trainer.variables().items() if "moving" not in k}
    assert set(before) == set(names) and not any(n.startswith("softmax/") for n in names)
    assert set(trainer.l2) == set(names)
    embed = trainer.embed_dim
    y, grads, gz_sums = run_stack(stack, before, x, offsets, LABELS, batch, embed)
    clear_margins(kind, o, y)
    want_loss = rg.grad(kind, y, LABELS, **o)["res"]["loss"]
    fwd_args = args if which != "tail" else (__import__("torch").from_numpy(x).cuda(),)
    y_dev = twin._forward(*fwd_args, training=True).cpu().numpy()
    res = trainer.step(*args, LABELS, RATE, global_step=0)
    assert np.isnan(res.accuracy) and np.isfinite(res.loss)
    worst = dict(output=rel(y_dev, y), loss=abs(res.loss - want_loss) / abs(want_loss))
    got = device_grads(trainer)
    assert set(got) == set(grads)
    for name in sorted(grads):
        zero = batch and name in gz_sums and any(s.bias == name and s.bn for s in trainer.specs)
        if zero:                                                      # the exact gradient is zero: judged against |gz|
            worst["grad " + name] = np.linalg.norm(got[name] - grads[name]) / np.linalg.norm(gz_sums[name])
        else:
            worst["grad " + name] = rel(got[name], grads[name])
    after = trainer.variables()
    assert not any(k.startswith("softmax/") for k in after)
    for name, w0 in before.items():                                   # momentum's first step from zero slots
        want = rlg.opt_step(rlg.MOMENTUM, w0, np.asarray(grads[name], dtype=np.float32), np.zeros_like(w0), lr=RATE, l2=trainer.l2[name],
                            momentum=0.9)[0]
        worst["var " + name] = rel(after[name], want)
    moving = [k for k in after if "moving" in k]
    assert bool(moving) == batch
    for name in moving:
        worst["stat " + name] = rel(after[name], stack.R[name].numpy())
        assert rel(after[name], weights[name]) > 100 * TOL, name
    final = {k: v for k, v in after.items() if "moving" not in k}
    want, _, _ = run_stack(stack, final, x, offsets, None, False, embed)
    fwd = trainer.forward(*args).cpu().numpy()
    worst["forward"] = float((np.linalg.norm(fwd - want, axis=1) / np.linalg.norm(want, axis=1)).max())
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print("%s %s %s: largest relative L2 " % (which, mode, loss) + ", ".join("%s %.2e" % kv for kv in top))
    assert all(v <= TOL for v in worst.values()), {k: v for k, v in worst.items() if v > TOL}


SGD_RATE = 0.02


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_an_sgd_step_lowers_the_loss_by_the_gradients_square(loss):
    """loss(w - lr g) = loss(w) - lr |g|^2 to first order: the decrease on the device lies within 0.5 .. 1.5 of lr |g|^2, at a
    rate at which the torch model's does."""
    from tf_kaldi_speaker_amd import metric_losses as ml
    from tf_kaldi_speaker_amd.params import Params
    trainer, _, _, stack, x, offsets, args = make("tail", loss, "moving", optimizer=dict(optimizer="sgd", weight_l2_regularizer=0.0))
    kind, o = LOSSES[loss][1:]
    before = trainer.variables()
    y, grads, _ = run_stack(stack, before, x, offsets, LABELS, False, trainer.embed_dim)
    clear_margins(kind, o, y)
    square = sum(float(np.sum(np.square(g))) for g in grads.values())
    moved = {k: np.asarray(v, dtype=np.float64) - SGD_RATE * grads[k] for k, v in before.items()}
    y1, _, _ = run_stack(stack, moved, x, offsets, None, False, trainer.embed_dim)
    clear_margins(kind, o, y1)
    loss0, loss1 = (rg.grad(kind, rows, LABELS, **o)["res"]["loss"] for rows in (y, y1))
    ratio = (loss0 - loss1) / (SGD_RATE * square)
    print("%s torch: loss %.6f -> %.6f, lr |g|^2 %.3e, ratio %.3f" % (loss, loss0, loss1, SGD_RATE * square, ratio))
    assert 0.5 <= ratio <= 1.5, "the rate is too large for the first-order statement on the torch model itself"
    res = trainer.step(*args, LABELS, SGD_RATE, global_step=0)
    got = device_grads(trainer)
    square_dev = sum(float(np.sum(np.square(g.astype(np.float64)))) for g in got.values())
    head = ml.MetricHead(Params(**LOSSES[loss][0]), 0)
    after = head.loss(trainer.forward(*args), LABELS).loss
    ratio = (res.loss - after) / (SGD_RATE * square_dev)
    print("%s device: loss %.6f -> %.6f, lr |g|^2 %.3e, ratio %.3f" % (loss, res.loss, after, SGD_RATE * square_dev, ratio))
    assert 0.5 <= ratio <= 1.5


# ------------------------------------------------------------------------------------------------ the command
def run_command(tmp_path, capsys, name, loss, flags):
    from test_gpu_head_train import train_setup
    from tf_kaldi_speaker_amd import model_io, train_head, valid
    params, weights, pre, data, spklist = train_setup(tmp_path)
    new = dict(params, num_steps_per_epoch=2, num_speakers_per_batch=3, num_segments_per_speaker=2, **LOSSES[loss][0])
    config = str(tmp_path / ("%s.json" % name))
    with open(config, "w") as f:
        import json
        json.dump(new, f)
    outs = []
    for run in range(2):
        out = str(tmp_path / ("%s-%d" % (name, run)))
        assert train_head.main(["--gpu", "0", "--config", config, "--seed", "5", "--precision", "f32", "--keep-head"] + flags +
                               [pre, data, spklist, data, spklist, out]) == 0
        outs.append(out)
    capsys.readouterr()
    nnet = os.path.join(outs[0], "nnet")
    for f in ("model-2.npz", "config.json", "feature_dim", "valid_loss", "learning_rate"):
        assert os.path.isfile(os.path.join(nnet, f)), f
    assert valid.main(["--gpu", "0", "--precision", "f32", outs[0], data, spklist]) == 0
    report = capsys.readouterr().out.strip().splitlines()[-1].split()
    line = open(os.path.join(nnet, "valid_loss")).read().split()
    print("valid_loss line %s, valid command %s" % (line, report))
    assert line[0] == "0" and report[1] == "2" and line[1] == report[3] and line[2] == report[7] and np.isfinite(float(line[1]))
    saved, step = model_io.load_weights(nnet)
    assert step == 2 and set(saved) == set(weights)
    assert open(os.path.join(nnet, "model-2.npz"), "rb").read() == open(os.path.join(outs[1], "nnet", "model-2.npz"), "rb").read()
    return new, weights, saved


def test_train_head_segment_layers_with_the_angular_triplet_loss(tmp_path, capsys):
    from tf_kaldi_speaker_amd import tail_train
    params, weights, saved = run_command(tmp_path, capsys, "angular", "angular", ["--segment-layers"])
    names = set(tail_train.metric_trained_names(params))
    assert names and not any(n.startswith("softmax/") for n in names) and "softmax/output/kernel" in weights
    for k, v in weights.items():
        assert (saved[k].tobytes() != np.asarray(v, dtype=np.float32).tobytes()) == (k in names), k


def test_train_head_conv_layers_batch_norm_with_the_semihard_loss(tmp_path, capsys):
    from tf_kaldi_speaker_amd import conv_train
    params, weights, saved = run_command(tmp_path, capsys, "semihard", "semihard", ["--conv-layers", "--batch-norm", "batch"])
    names = set(conv_train.metric_trained_names(params))
    moving = set(k for k in weights if k.endswith("/moving_mean") or k.endswith("/moving_variance"))
    # a bias in front of a batch norm in training mode has the exact gradient zero: it may stay as it was
    for k, v in weights.items():
        changed = saved[k].tobytes() != np.asarray(v, dtype=np.float32).tobytes()
        assert not changed or k in names or k in moving, k                 # every untrained variable byte for byte
        assert changed or not (k in names and k.endswith("/kernel")), k
