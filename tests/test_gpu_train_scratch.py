"""GPU: training from scratch (tf_kaldi_speaker_amd/train.py) on a synthetic data directory of tests/helpers/train_arks.py:
6 speakers x 4 utterances of 40 to 80 frames, dimension 8, half of them in a 'CM ' archive and half in an 'FM ' one, a mean
per speaker; chunks of 24 to 32 frames, 3 speakers x 2 segments per batch, 3 steps per epoch.

The driver must add nothing to the trainers: the same fresh weights, stepped by hand over the plan's batches as the native reader
decodes them, give the bytes the driver writes.  prefetch changes nothing, and a run that stops and continues (-c), at the end
of an epoch or inside one, writes the variables and the optimizer's arrays of the run that did not stop."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import train_arks as ta                                            # noqa: E402

pytestmark = pytest.mark.gpu

DIM, CHANNELS, POOL, LAST = 8, 8, 24, 16
BATCH = dict(num_speakers_per_batch=3, num_segments_per_speaker=2, min_segment_len=24, max_segment_len=32, num_steps_per_epoch=3,
             num_epochs=2, reduce_lr_epochs=2, valid_max_iterations=100, seed=5, show_training_progress=1,
             num_nodes_pooling_layer=POOL, num_nodes_last_layer=LAST, weight_l2_regularizer=1e-3, batchnorm_momentum=0.5)
OPTIMIZERS = {"momentum": dict(optimizer="momentum", momentum=0.9, use_nesterov=True, learning_rate=0.05),
              "adam": dict(optimizer="adam", learning_rate=2e-3)}
ATTENTION = dict(pooling_type="self_attention", att_key_input="tdnn4_relu", att_key_num_nodes=[12, 8], att_key_network_type=1,
                 att_value_input="tdnn5_relu", att_value_num_nodes=[], att_value_network_type=0, att_apply_nonlinear=False,
                 att_use_scale=True, att_num_heads=1, att_split_key=True, att_split_value=True, att_penalty_term=0)
TRIPLET = dict(loss_func="angular_triplet_loss", margin=0.2, triplet_type="all", loss_type="additive_margin_softmax")
# "it learns": the values chosen on the torch float64 model (the docstring of the test)
LEARN_OFFSET, LEARN_RATE, LEARN_STEPS = 4.0, 0.05, 40
LEARN_CHANNELS, LEARN_POOL, LEARN_LAST = 32, 64, 32


def tdnn_params(optimizer="momentum", **extra):
    from tf_kaldi_speaker_amd import synth
    return dict(synth.TDNN_STAT_PARAMS, **dict(dict(BATCH, **OPTIMIZERS[optimizer]), **extra))


def resnet_params(**extra):
    from tf_kaldi_speaker_amd import synth
    own = dict(BATCH, min_segment_len=16, max_segment_len=16, resnet_blocks=[2, 1, 1, 1], num_epochs=1, **OPTIMIZERS["momentum"])
    return dict(synth.RESNET_PARAMS, **dict(own, **extra))


class World(object):
    """The data directories and every run of train.train the tests share, made once."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.data, self.spklist, self.mats = ta.make_train_dir(tmp / "d8", dim=DIM, offset=LEARN_OFFSET, seed=2)
        self.runs = {}
        self._wide = None

    def wide(self):
        """The 40-dimensional directory of the ResNet (model/resnet.py:190)."""
        if self._wide is None:
            self._wide = ta.make_train_dir(self.tmp / "d40", dim=40, offset=LEARN_OFFSET, seed=3)
        return self._wide

    def run(self, name, params, data=None, model=None, **kw):
        """train.train once per name -> (model dir, history, [log lines])."""
        from tf_kaldi_speaker_amd import train
        if name not in self.runs:
            data, spklist = (self.data, self.spklist) if data is None else data
            model = model or str(self.tmp / name)
            lines = []
            kw.setdefault("channels", CHANNELS)
            kw.setdefault("width", 4)
            hist = train.train(data, spklist, data, spklist, model, config=params, precision="f32", log=lines.append, **kw)
            self.runs[name] = (model, hist, lines)
        return self.runs[name]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    import torch
    assert torch.cuda.is_available()
    return World(tmp_path_factory.mktemp("scratch"))


def arrays(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def same_arrays(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
                                          for k in a)


def text(model, name):
    with open(os.path.join(model, "nnet", name), "rb") as f:
        return f.read()


def same_directories(a, b, skip=()):
    """The same files; every array of every .npz and every byte of every other file (an .npz holds its own time stamps)."""
    names = sorted(os.listdir(os.path.join(a, "nnet")))
    assert names == sorted(os.listdir(os.path.join(b, "nnet")))
    for n in names:
        if n in skip:
            continue
        if n.endswith(".npz"):
            assert same_arrays(arrays(os.path.join(a, "nnet", n)), arrays(os.path.join(b, "nnet", n))), n
        else:
            assert text(a, n) == text(b, n), n


def native_batch(mats, batch, dim):
    """The batch as the native reader decodes it -> (float32 [B * length, dim], offsets)."""
    rows = [mats[k][s:s + batch.length, :dim] for k, s in zip(batch.keys, batch.starts)]
    return np.ascontiguousarray(np.concatenate(rows), dtype=np.float32), np.arange(len(rows) + 1, dtype=np.int64) * batch.length


def by_hand(make, params, data, spklist, mats, dim, rates, width_kw):
    """fresh_weights handed to the trainer `make` builds, stepped over the plan's batches of len(rates) epochs -> variables."""
    import torch
    from tf_kaldi_speaker_amd import head_train, train
    from tf_kaldi_speaker_amd.params import Params
    classes = 6
    weights = train.fresh_weights(params, dim, classes, params["seed"], **width_kw)
    metric = "softmax/output/kernel" not in weights
    trainer = make(Params(**params), weights, classes, 0, params["seed"], weights.get("softmax/output/kernel"),
                   weights.get("softmax/output/bias"), "batch", metric)
    step = 0
    for epoch, lr in enumerate(rates):
        for batch in head_train.plan_train_batches(data, spklist, params, params["seed"], epoch):
            feats, offsets = native_batch(mats, batch, dim)
            trainer.step(torch.from_numpy(feats).cuda(), offsets, batch.labels, lr, global_step=step)
            step += 1
    out = dict(weights)
    out.update(trainer.variables())
    return out, trainer.optimizer_state()


def test_two_epochs_from_nothing_write_the_directory(world):
    from tf_kaldi_speaker_amd import model_io, synth
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params = tdnn_params("momentum")
    model, hist, lines = world.run("momentum", params)
    nnet = os.path.join(model, "nnet")
    assert sorted(os.listdir(nnet)) == sorted(["model-3.npz", "model-6.npz", "optimizer-3.npz", "optimizer-6.npz", "checkpoint",
                                               "config.json", "feature_dim", "valid_loss", "learning_rate"])
    assert len(text(model, "valid_loss").splitlines()) == 2 and len(text(model, "learning_rate").splitlines()) == 3
    assert text(model, "feature_dim") == b"8\n" and model_io.read_checkpoint_state(nnet) == "model-6"
    assert json.loads(text(model, "config.json").decode()) == params                      # as given: no default written into it
    assert [(e, s) for e, s, _, _, _ in hist] == [(0, 3), (1, 6)] and all(np.isfinite(h[2]) and 0.0 <= h[3] <= 1.0 for h in hist)
    saved = arrays(os.path.join(nnet, "model-6.npz"))
    assert set(saved) == set(synth.synth_weights(params, DIM, 0, CHANNELS)) | {"softmax/output/kernel", "softmax/output/bias"}
    state = arrays(os.path.join(nnet, "optimizer-6.npz"))
    assert int(state["num_steps"]) == 6 and len(state) == 1 + len([k for k in saved if "moving" not in k])      # one slot per tensor
    progress = [line for line in lines if line.startswith("Epoch: [")]
    assert len(progress) == 6 and progress[0].startswith("Epoch: [ 0] step: [ 0/ 3] time: ") and ", raw loss: " in progress[0]
    tr = Trainer(Params(**params), model, DIM, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(saved)
    emb = tr.predict(np.stack([world.mats["spk0-u0"][:40], world.mats["spk3-u1"][:40]]))
    tr.close()
    assert emb.shape == (2, CHANNELS) and np.isfinite(emb).all() and np.abs(emb).max() > 0      # embedding_node tdnn6_dense


@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
def test_the_driver_adds_nothing_to_the_conv_trainer(world, optimizer):
    from tf_kaldi_speaker_amd import conv_train
    params = tdnn_params(optimizer)
    model, hist, _ = world.run(optimizer, params)
    want, state = by_hand(conv_train.ConvTrainer, params, world.data, world.spklist, world.mats, DIM, [h[4] for h in hist],
                          dict(channels=CHANNELS))
    assert len(hist) == 2 and same_arrays(arrays(os.path.join(model, "nnet", "model-6.npz")), {k: np.asarray(v) for k, v in want.items()})
    assert same_arrays(arrays(os.path.join(model, "nnet", "optimizer-6.npz")), state)
    slots = 2 if optimizer == "adam" else 1
    assert len(state) == 1 + slots * len([k for k in want if "moving" not in k])


def test_the_driver_adds_nothing_to_the_attention_trainer(world):
    from tf_kaldi_speaker_amd import att_train
    params = tdnn_params("momentum", num_epochs=1, **ATTENTION)
    model, hist, _ = world.run("attention", params)
    want, _ = by_hand(att_train.AttConvTrainer, params, world.data, world.spklist, world.mats, DIM, [h[4] for h in hist],
                      dict(channels=CHANNELS))
    assert len(hist) == 1 and "tdnn/attention/query" in want
    assert same_arrays(arrays(os.path.join(model, "nnet", "model-3.npz")), {k: np.asarray(v) for k, v in want.items()})


def test_the_driver_adds_nothing_to_the_resnet_trainer(world):
    from tf_kaldi_speaker_amd import resnet_train
    params = resnet_params()
    data, spklist, mats = world.wide()
    model, hist, _ = world.run("resnet", params, data=(data, spklist))
    want, _ = by_hand(resnet_train.ResNetTrainer, params, data, spklist, mats, 40, [h[4] for h in hist], dict(width=4))
    assert len(hist) == 1 and "resnet_18/conv1a_conv0/kernel" in want
    assert same_arrays(arrays(os.path.join(model, "nnet", "model-3.npz")), {k: np.asarray(v) for k, v in want.items()})


def test_the_driver_adds_nothing_behind_the_metric_door(world):
    from tf_kaldi_speaker_amd import conv_train
    params = tdnn_params("momentum", num_epochs=1, **TRIPLET)
    model, hist, _ = world.run("triplet", params)
    want, _ = by_hand(conv_train.ConvTrainer, params, world.data, world.spklist, world.mats, DIM, [h[4] for h in hist],
                      dict(channels=CHANNELS))
    assert len(hist) == 1 and "softmax/output/kernel" not in want and np.isfinite(hist[0][2])
    assert same_arrays(arrays(os.path.join(model, "nnet", "model-3.npz")), {k: np.asarray(v) for k, v in want.items()})


def test_prefetch_changes_nothing(world):
    params = tdnn_params("momentum")
    ahead, _, _ = world.run("momentum", params)
    inline, _, _ = world.run("inline", params, prefetch=0)
    same_directories(ahead, inline)


@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
def test_one_epoch_and_one_more_are_two_epochs(world, optimizer):
    params = tdnn_params(optimizer)
    straight, _, _ = world.run(optimizer, params)
    model, first, _ = world.run(optimizer + "-first", dict(params, num_epochs=1))
    assert [(e, s) for e, s, _, _, _ in first] == [(0, 3)]
    _, more, _ = world.run(optimizer + "-more", params, model=model, cont=True)
    assert [(e, s) for e, s, _, _, _ in more] == [(1, 6)]
    same_directories(straight, model)


@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
def test_continuing_inside_an_epoch(world, optimizer):
    """save_checkpoints_steps = 2 writes model-2 and model-5 beside the epochs' own; a directory cut back to model-2 and continued
    ends as the run that did not stop."""
    params = tdnn_params(optimizer, save_checkpoints_steps=2)
    straight, _, _ = world.run(optimizer, tdnn_params(optimizer))
    marked, _, _ = world.run(optimizer + "-marked", params)
    names = sorted(os.listdir(os.path.join(marked, "nnet")))
    assert [n for n in names if n.endswith(".npz")] == sorted("%s-%d.npz" % (w, s) for w in ("model", "optimizer") for s in (2, 3, 5, 6))
    for n in ("model-3.npz", "model-6.npz", "optimizer-3.npz", "optimizer-6.npz"):                  # a checkpoint changes nothing
        assert same_arrays(arrays(os.path.join(marked, "nnet", n)), arrays(os.path.join(straight, "nnet", n))), n
    assert text(marked, "valid_loss") == text(straight, "valid_loss")
    cut = str(world.tmp / (optimizer + "-cut"))
    os.makedirs(os.path.join(cut, "nnet"))
    for n in ("model-2.npz", "optimizer-2.npz", "config.json", "feature_dim"):
        shutil.copy(os.path.join(marked, "nnet", n), os.path.join(cut, "nnet", n))
    with open(os.path.join(cut, "nnet", "checkpoint"), "w") as f:
        f.write('model_checkpoint_path: "model-2"\nall_model_checkpoint_paths: "model-2"\n')
    _, more, _ = world.run(optimizer + "-cut", None, model=cut, cont=True)
    assert [(e, s) for e, s, _, _, _ in more] == [(0, 3), (1, 6)]
    for n in ("model-3.npz", "model-5.npz", "model-6.npz", "optimizer-3.npz", "optimizer-5.npz", "optimizer-6.npz"):
        assert same_arrays(arrays(os.path.join(cut, "nnet", n)), arrays(os.path.join(marked, "nnet", n))), n
    assert text(cut, "valid_loss") == text(marked, "valid_loss") and text(cut, "learning_rate") == text(marked, "learning_rate")


def test_keep_checkpoint_max_prunes_the_pairs(world):
    params = tdnn_params("momentum", save_checkpoints_steps=1, keep_checkpoint_max=2)
    model, _, _ = world.run("pruned", params)
    assert sorted(n for n in os.listdir(os.path.join(model, "nnet")) if n.endswith(".npz")) == [
        "model-5.npz", "model-6.npz", "optimizer-5.npz", "optimizer-6.npz"]


def torch_losses(params, data, spklist, mats, steps, rate, channels, batch_stats=True):
    """The torch float64 model of the stack (tests/test_gpu_bn_train.TorchStack, training mode), trained with plain sgd on the
    plan's batches from fresh_weights -> the training loss of every step."""
    from test_gpu_bn_train import TorchStack
    from tf_kaldi_speaker_amd import conv_train, head_train, tail_train, train
    weights = train.fresh_weights(params, DIM, 6, params["seed"], channels=channels)
    frame, seg = conv_train.frame_variables(params), tail_train.segment_variables(params)
    bessel = {s.kernel: np.ndim(weights[s.kernel]) == 4 for s in tuple(frame) + tuple(seg)}
    stack = TorchStack(frame, seg, weights, bessel)
    variables = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items() if "moving" not in k}
    losses = []
    for batch in head_train.plan_train_batches(data, spklist, params, params["seed"], 0)[:steps]:
        feats, offsets = native_batch(mats, batch, DIM)
        out, grads, _ = stack.run(variables, feats, offsets, batch.labels, batch_stats)
        logits = out @ variables["softmax/output/kernel"] + variables["softmax/output/bias"]
        logits -= logits.max(axis=1, keepdims=True)
        logp = logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))
        losses.append(float(-logp[np.arange(len(batch.labels)), batch.labels].mean()))
        for k in variables:
            variables[k] = variables[k] - rate * grads[k]
    return losses


def learn_params():
    from tf_kaldi_speaker_amd import synth
    return dict(synth.TDNN_STAT_PARAMS, **dict(BATCH, optimizer="sgd", learning_rate=LEARN_RATE, weight_l2_regularizer=0.0,
                                               num_steps_per_epoch=LEARN_STEPS, num_epochs=1, show_training_progress=0,
                                               num_nodes_pooling_layer=LEARN_POOL, num_nodes_last_layer=LEARN_LAST))


def test_it_learns(world):
    """40 steps of plain sgd at the fixed rate 0.05, batch norm in training mode, on the directory of every test here: speaker s
    has the mean 4.0 on axis s (unit noise).  The values were chosen on the torch float64 model of the same stack
    (tests/test_gpu_bn_train.TorchStack) on the same batches, on the CPU.  At the widths of the other tests (8 channels, pooling
    24, last layer 16) that model stalls: with three speakers in a batch, what batch norm subtracts depends on the other two, and
    8 channels cannot sort that out in 40 steps (mean loss of the first 5 steps 1.8756, of the last 5 1.0658, a factor of 1.76;
    no rate from 0.02 to 0.8 and no offset from 0.3 to 16 gave 2).  At 32 channels, pooling 64 and a last layer of 32, the widths
    of this test, it falls from 1.6882 to 0.6132, a factor of 2.75 (2.33 at an offset of 2.0; 1.87 at the rate 0.2, not taken).
    The device must fall as well, and its first 3 losses must be the torch model's within 1e-4, the bound
    tests/test_gpu_bn_train.py holds the same trainers to.  (On an MI355X: 1.6882 to 0.6320, the first three losses within 6e-7
    of torch's.)"""
    params = learn_params()
    got = []
    world.run("learn", params, channels=LEARN_CHANNELS, on_step=lambda step, res: got.append(res.loss))
    want = torch_losses(params, world.data, world.spklist, world.mats, LEARN_STEPS, LEARN_RATE, LEARN_CHANNELS)
    print("torch: first 5 %.4f last 5 %.4f; device: first 5 %.4f last 5 %.4f" % (np.mean(want[:5]), np.mean(want[-5:]),
                                                                                 np.mean(got[:5]), np.mean(got[-5:])))
    assert len(got) == LEARN_STEPS and np.mean(want[-5:]) <= 0.5 * np.mean(want[:5])           # the margin comes from the reference
    for t in range(3):
        print("step %d: device %.6f torch %.6f" % (t, got[t], want[t]))
        assert abs(got[t] - want[t]) <= 1e-4 * abs(want[t]), (t, got[t], want[t])
    assert np.mean(got[-5:]) < np.mean(got[:5])
