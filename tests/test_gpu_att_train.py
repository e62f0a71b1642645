"""GPU: att_train.AttFrameTrainer / AttConvTrainer on a narrow attention TDNN and extended TDNN (16 channels, a two-layer key
network, heads 1 and 2, att_key_input in front of att_value_input and both on one node) against a torch float64 model of the
same stack (tests/helpers/ref_att_train.py), in batch_norm "moving" and "batch".

One step: every gradient, every updated variable, the moved statistics and the inference forward within the project's parity
bar, 1e-4 relative L2 per tensor (the bar of tests/test_gpu_bn_train.py; the bias in front of a batch norm in training mode has
the exact gradient zero and is judged against the column sums of |gz|, as there; so has the bias of a linear last value layer).  The observed maxima are printed.  Then:
forward() against Trainer.predict at `output` on the same weights, a few steps on separable frames lower the loss, two runs with
one seed write the same bits, and a checkpoint written by train_head(conv_layers=True) on an attention model validates and
extracts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pool_grad_cases as pc                                        # noqa: E402
import ref_att_train as rat                                         # noqa: E402
from test_gpu_bn_train import device_grads, rel                     # noqa: E402
from test_gpu_conv_train import toy_segments                        # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
DIM, CHANNELS, POOL, LAST, CLASSES = 30, 16, 24, 16, 3
MOMENTUM, RATE, L2 = 0.5, 0.05, 1e-3
LENGTHS = {"tdnn": (30, 33, 37, 40, 31, 35), "extended_tdnn": (34, 37, 41, 44, 35, 39)}
EXTRA = dict(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=L2, batchnorm_momentum=MOMENTUM,
             num_nodes_pooling_layer=POOL, num_nodes_last_layer=LAST, pooling_type="self_attention", att_apply_nonlinear=False,
             att_penalty_term=0)
# name -> (network_type, the attention's keys): the key in front of the value with one head, both on one node with two heads and
# a value network, the extended TDNN
MODELS = {
    "front-h1": ("tdnn", dict(att_key_input="tdnn4_relu", att_key_num_nodes=[12, 8], att_key_network_type=1, att_value_input="tdnn5_relu",
                              att_value_num_nodes=[], att_value_network_type=0, att_use_scale=True, att_num_heads=1,
                              att_split_key=True, att_split_value=True)),
    "same-h2": ("tdnn", dict(att_key_input="tdnn5_relu", att_key_num_nodes=[12, 8], att_key_network_type=2, att_value_input="tdnn5_relu",
                             att_value_num_nodes=[10, 6], att_value_network_type=0, att_use_scale=True, att_num_heads=2,
                             att_split_key=True, att_split_value=False)),
    "etdnn-h2": ("extended_tdnn", dict(att_key_input="tdnn9_relu", att_key_num_nodes=[12, 8], att_key_network_type=1,
                                       att_value_input="tdnn10_relu", att_value_num_nodes=[], att_value_network_type=0,
                                       att_use_scale=False, att_num_heads=2, att_split_key=False, att_split_value=True)),
}


def model(name, seed=4):
    from tf_kaldi_speaker_amd import synth
    net, att = MODELS[name]
    params = dict(synth.TDNN_STAT_PARAMS, network_type=net, **dict(EXTRA, **att))
    return params, synth.synth_weights(params, DIM, seed=seed, channels=CHANNELS)


def make_trainer(name, conv, mode, seed=3):
    from tf_kaldi_speaker_amd import att_train
    from tf_kaldi_speaker_amd.params import Params
    params, weights = model(name)
    cls = att_train.AttConvTrainer if conv else att_train.AttFrameTrainer
    return cls(Params(**params), weights, CLASSES, device=0, seed=seed, batch_norm=mode), params, weights


def inputs(name, conv):
    """-> (rows float32, offsets int64, labels int32): packed features for the convolutional trainer, packed frames of the
    frozen node's width (non-negative, as a ReLU hands them on) for the frame trainer."""
    net = MODELS[name][0]
    if conv:
        return toy_segments(17, CLASSES, 2, LENGTHS[net])
    frames, off, labels = pc.separable_frames(5, CLASSES, 2, CHANNELS, (23, 31, 20, 36, 27, 29))
    return frames, off.astype(np.int64), labels


@pytest.mark.parametrize("mode", ["moving", "batch"])
@pytest.mark.parametrize("conv", [False, True], ids=["frame", "conv"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_step_against_torch(name, conv, mode):
    import torch
    import ref_loss_grad as rg
    trainer, params, weights = make_trainer(name, conv, mode)
    twin, _, _ = make_trainer(name, conv, mode)
    x, offsets, labels = inputs(name, conv)
    dev = torch.from_numpy(x).cuda()
    batch = mode == "batch"
    bessel = {spec.kernel: layer.bessel for spec, layer in zip(trainer.specs, trainer.layers)}
    assert not any(bessel[s.kernel] for s in trainer.att_specs)               # rank-2 kernels: the biased variance
    assert all(layer.batch_stats == (batch and spec.bn is not None) for spec, layer in zip(trainer.specs, trainer.layers))
    stack = rat.AttTorchStack(trainer, weights, bessel)
    before = {k: v for k, v in trainer.variables().items() if "moving" not in k}
    assert set(before) == set(n for n, _, _, _ in trainer.tensors())
    y_dev = twin._forward(dev, offsets, training=True).cpu().numpy()          # the mode's own forward, on a twin
    res = trainer.step(dev, offsets, labels, RATE, global_step=0)
    assert np.isfinite(res.loss)
    y, grads, gz_sums = stack.run(before, x, offsets, labels, batch)
    worst = dict(output=rel(y_dev, y))
    got = device_grads(trainer)
    assert set(got) == set(grads)
    # a linear last value layer adds its bias to every pooled mean (the weights of an utterance sum to 1), and the batch norm of
    # the first segment layer, in training mode, subtracts what all rows share: that bias has the exact gradient zero as well
    shift = [s.bias for s in trainer.value_specs[-1:] if batch and not s.bn and s.act == 0]
    for gname in sorted(grads):
        zero = batch and gname in gz_sums and (gname in shift or any(s.bias == gname and s.bn for s in trainer.specs))
        if zero:                                                              # the exact gradient is zero: judged against |gz|
            err = np.linalg.norm(got[gname] - grads[gname]) / np.linalg.norm(gz_sums[gname])
        else:
            err = rel(got[gname], grads[gname])
        worst["grad " + gname] = err
    after = trainer.variables()
    l2 = trainer.l2
    for vname, w0 in before.items():                                          # momentum's first step from zero slots
        want = rg.opt_step(rg.MOMENTUM, w0, np.asarray(grads[vname], dtype=np.float32), np.zeros_like(w0), lr=RATE, l2=l2[vname],
                           momentum=0.9)[0]
        worst["var " + vname] = rel(after[vname], want)
        zero = batch and (vname in shift or any(s.bias == vname and s.bn for s in trainer.specs))
        assert zero or after[vname].tobytes() != w0.tobytes(), vname          # every trained variable with a gradient moved
    moving = [k for k in after if "moving" in k]
    assert bool(moving) == batch
    for vname in moving:
        worst["stat " + vname] = rel(after[vname], stack.R[vname].numpy())
        assert rel(after[vname], weights[vname]) > 100 * TOL, vname
    if batch:
        assert sum(1 for k in moving if "/attention/" in k) == 2 * sum(1 for s in trainer.att_specs if s.bn)
    final = {k: v for k, v in after.items() if "moving" not in k}
    want, _, _ = stack.run(final, x, offsets, None, False)
    fwd = trainer.forward(dev, offsets).cpu().numpy()
    worst["forward"] = float((np.linalg.norm(fwd - want, axis=1) / np.linalg.norm(want, axis=1)).max())
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print("%s %s %s: largest relative L2 " % (name, "conv" if conv else "frame", mode) + ", ".join("%s %.2e" % kv for kv in top))
    assert all(v <= TOL for v in worst.values()), {k: v for k, v in worst.items() if v > TOL}


@pytest.mark.parametrize("name", ["front-h1", "same-h2"])
def test_forward_is_trainer_predict(name):
    import torch
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    trainer, params, weights = make_trainer(name, True, "moving")
    feats, offsets, _ = toy_segments(9, CLASSES, 2, (36,))
    got = trainer.forward(torch.from_numpy(feats).cuda(), offsets).cpu().numpy()
    tr = Trainer(Params(**params), None, DIM, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights)
    tr.embeddings = "output"
    want = tr.predict(feats.reshape(len(offsets) - 1, 36, DIM))
    tr.close()
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    print("%s: forward() against Trainer.predict at output, relative L2 per row, largest %.3e" % (name, float(err.max())))
    assert err.max() <= TOL


def test_a_few_steps_lower_the_loss_and_one_seed_gives_the_same_bits():
    import torch
    frames, off, labels = pc.separable_frames(11, CLASSES, 4, CHANNELS, (20, 25, 31))
    dev = torch.from_numpy(frames).cuda()
    runs = []
    for _ in range(2):
        trainer, _, _ = make_trainer("front-h1", False, "moving", seed=7)
        losses = [trainer.step(dev, off.astype(np.int64), labels, 0.1, global_step=t).loss for t in range(8)]
        runs.append((losses, trainer.variables()))
    losses = runs[0][0]
    print("loss over eight steps: " + " ".join("%.4f" % v for v in losses))
    assert losses[-1] < 0.7 * losses[0]
    assert runs[0][0] == runs[1][0] and all(runs[0][1][k].tobytes() == runs[1][1][k].tobytes() for k in runs[0][1])


def test_train_head_conv_layers_on_an_attention_model(tmp_path):
    """train_head(conv_layers=True) on a synthetic attention model directory: the checkpoint holds every trained variable
    changed and the rest unchanged, the validation ran on it, and Trainer.predict extracts from it."""
    from test_gpu_head_train import f32, make_data_dir
    from tf_kaldi_speaker_amd import att_train, head_train, model_io, synth
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    extra = dict(loss_func="softmax", num_speakers_per_batch=4, num_segments_per_speaker=2, min_segment_len=30, max_segment_len=40,
                 valid_max_iterations=100, num_steps_per_epoch=4, num_epochs=1, learning_rate=0.1, reduce_lr_epochs=2, seed=5)
    params = dict(synth.TDNN_STAT_PARAMS, **dict(EXTRA, **dict(MODELS["front-h1"][1], **extra)))
    weights = synth.synth_weights(params, 30, seed=4, channels=8)
    rs = np.random.RandomState(21)
    weights["softmax/output/kernel"] = f32(rs.standard_normal((16, 3)))
    weights["softmax/output/bias"] = f32(rs.standard_normal(3))
    pre = str(tmp_path / "pretrain")
    model_io.save_model(pre, params, 30, weights, step=4321)
    spk_utts = [("spk%d" % s, ["spk%d-u%d" % (s, u) for u in range(3)]) for s in (3, 0, 5, 1, 4, 2)]
    lens = {u: int(t) for (_, us) in spk_utts for u, t in zip(us, rs.randint(42, 61, 18))}
    data, spklist, _ = make_data_dir(tmp_path, spk_utts, lens, dim=32, spklist=[("spk%d" % s, s) for s in range(6)], seed=22)
    tr = Trainer(Params(**params), pre, 30, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    out = str(tmp_path / "att")
    hist = head_train.train_head(tr, data, spklist, data, spklist, out, weights=weights, seed=5, precision="f32", conv_layers=True)
    tr.close()
    assert len(hist) == 1 and hist[0][1] == 4 and np.isfinite(hist[0][2]) and 0.0 <= hist[0][3] <= 1.0
    saved, _ = model_io.load_weights(os.path.join(out, "nnet"))
    names = set(att_train.trained_names(params, True))
    assert "tdnn/attention/query" in names and set(saved) >= set(weights)
    for k, v in weights.items():
        if k.startswith("softmax/"):
            continue
        assert (saved[k].tobytes() != np.asarray(v, dtype=np.float32).tobytes()) == (k in names), k
    ex = Trainer(Params(**params), out, 30, single_cpu=True, device=0, precision="f32")
    ex.build("predict")
    ex.load_weights(saved)
    ex.embeddings = "output"
    feats = np.random.RandomState(3).standard_normal((2, 40, 30)).astype(np.float32)
    emb = ex.predict(feats)
    ex.close()
    assert emb.shape == (2, 16) and np.all(np.isfinite(emb))
