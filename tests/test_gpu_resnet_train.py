"""GPU: one step of resnet_train.ResNetTrainer against a torch float64 model of the same stack
(tests/helpers/ref_resnet_train.py: per-utterance F.pad + conv2d, the batch norm's mode as a switch), in the scheme of
tests/test_gpu_bn_train.py and tests/test_gpu_att_train.py.

The model is small (width 4, resnet_blocks [2, 1, 1, 1], pooling 24, last layer 16; three utterances of 9, 14 and 11 frames) and
whole: every gradient, every updated variable, every moved statistic and the inference forward() are judged by the project's
parity requirement, 1e-4 relative L2 per tensor; no element and no tensor is left out.  The bias in front of a batch norm in
training mode has the exact gradient zero (the mean is subtracted): it is judged against the column sums of |gz|, the size of the
terms that cancel, as in those two files.  The seeds keep every activation input away from zero (ref_resnet_train.CASES; the
condition is asserted on the CPU in tests/test_resnet_train_host.py).

Then forward() against Trainer.predict in exact fp32 on the same weights, and a checkpoint written by
train_head(conv_layers=True) on a synthetic data directory."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_loss_grad as rlg                                         # noqa: E402
import ref_resnet_train as rr                                       # noqa: E402
from valid_data import make_data_dir                                # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
CLASSES = 3
HEAD_K, HEAD_B = rr.HEAD_K, rr.HEAD_B
RATES = {"sgd": 0.05, "momentum": 0.05, "adam": 0.002}
KINDS = {"sgd": rlg.SGD, "momentum": rlg.MOMENTUM, "adam": rlg.ADAM}


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def device_grads(trainer):
    """name -> the gradient the last step left on the device, in TensorFlow shapes."""
    from tf_kaldi_speaker_amd import conv_train
    shapes = {spec.kernel: (layer, getattr(layer, "shape", (layer.in_dim, layer.out_dim))) for spec, layer in zip(trainer.specs, trainer.layers)}
    out = {}
    for name, _, g, _ in trainer.tensors():
        g = g.cpu().numpy()
        if name in shapes:
            layer, shape = shapes[name]
            g = conv_train.rows_to_kernel(g[:, :layer.in_dim], shape)
        elif name == HEAD_K:
            g = g[:, :trainer.embed_dim].T
        out[name] = g
    return out


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_one_step_against_torch(name):
    import torch
    from tf_kaldi_speaker_amd import resnet_train
    from tf_kaldi_speaker_amd.params import Params
    mode, extra, seed, _ = rr.CASES[name]
    params, weights, feats, offsets = rr.small_model(seed, **extra)
    metric = params["loss_func"] != "softmax"
    labels = np.array([0, 0, 1] if metric else [0, 1, 2], dtype=np.int32)
    batch = mode == "batch"
    trainer = resnet_train.ResNetTrainer(Params(**params), weights, CLASSES, device=0, seed=3, batch_norm=mode, metric=metric)
    names = [n for n, _, _, _ in trainer.tensors()]
    assert names == (resnet_train.metric_trained_names(params) if metric else resnet_train.trained_names(params))
    assert set(trainer.l2) == set(names)
    bessel = {spec.kernel: layer.bessel for spec, layer in zip(trainer.specs, trainer.layers)}
    assert bessel == {spec.kernel: batch and np.ndim(weights[spec.kernel]) == 4 for spec in trainer.specs}    # conv5 true, dense false
    before = {k: v for k, v in trainer.variables().items() if "moving" not in k}
    assert set(before) == set(names)
    for k, v in before.items():                                      # the kernels come back in the checkpoint's shape and bits
        assert v.shape == np.shape(weights[k]) if k in weights else True, k
        assert k not in weights or v.tobytes() == np.asarray(weights[k], np.float32).tobytes(), k
    stack = rr.TorchResNet(params, weights, params.get("batchnorm_momentum", 0.99))
    loss = None
    if metric:
        from test_metric_grad_host import torch_loss_of
        loss = lambda rows, lab: torch_loss_of("all", rows, lab.numpy(), loss_type=params["loss_type"], margin=params["margin"])   # noqa: E731
    ref = stack.run(before, feats, np.diff(offsets), labels, batch, loss)
    grads, gz_sums = ref["grads"], ref["gz_sums"]
    dev = torch.from_numpy(feats).cuda()
    rate = RATES[params["optimizer"]]
    res = trainer.step(dev, offsets, labels, rate, global_step=0)
    worst = dict(loss=abs(res.loss - ref["loss"]) / abs(ref["loss"]))
    assert np.isnan(res.accuracy) == metric
    got = device_grads(trainer)
    assert set(got) == set(grads)
    for k in sorted(grads):
        assert got[k].shape == grads[k].shape, k
        zero = batch and k in gz_sums and any(s.bias == k and s.bn for s in trainer.specs)
        if zero:                                                      # the exact gradient is zero: judged against |gz|
            worst["grad " + k] = float(np.linalg.norm(got[k] - grads[k]) / np.linalg.norm(gz_sums[k]))
        else:
            worst["grad " + k] = rel(got[k], grads[k])
    after = trainer.variables()
    clip = float(params.get("clip_gradient_norm", 0.0)) if params.get("clip_gradient") else 0.0
    for k, w0 in before.items():                                      # the first step from zero slots, by the optimizer's float32 rule
        zeros = np.zeros_like(w0)
        want = rlg.opt_step(KINDS[params["optimizer"]], w0, np.asarray(grads[k], dtype=np.float32), zeros, zeros, lr=rate, l2=trainer.l2[k],
                            clip_norm=clip, momentum=params.get("momentum", 0.9), use_nesterov=bool(params.get("use_nesterov")), step=1)[0]
        worst["var " + k] = rel(after[k], want)
        assert after[k].tobytes() != w0.tobytes() or not np.any(grads[k]), k
    moving = [k for k in after if "moving" in k]
    assert len(moving) == (2 * sum(1 for s in trainer.specs if s.bn) if batch else 0)
    for k in moving:
        worst["stat " + k] = rel(after[k], stack.R[k].numpy())
        assert rel(after[k], weights[k]) > 100 * TOL, k
    if not batch:                                                     # the moving statistics stay where they were, bit for bit
        for spec, layer in zip(trainer.specs, trainer.layers):
            if spec.bn:
                for i, s in ((2, "moving_mean"), (3, "moving_variance")):
                    assert layer.bn[i].cpu().numpy().tobytes() == np.asarray(weights[spec.bn + "/" + s], np.float32).tobytes()
    final = {k: v for k, v in after.items() if "moving" not in k}
    want = stack.run(final, feats, np.diff(offsets), None, False)["out"]
    fwd = trainer.forward(dev, offsets).cpu().numpy()
    worst["forward"] = float((np.linalg.norm(fwd - want, axis=1) / np.linalg.norm(want, axis=1)).max())
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("%s: %d tensors, largest relative L2 " % (name, len(names)) + ", ".join("%s %.2e" % kv for kv in top))
    assert all(v <= TOL for v in worst.values()), {k: v for k, v in worst.items() if not v <= TOL}


def test_forward_is_the_extractors_output():
    """ResNetTrainer.forward() on the checkpoint's weights against Trainer.predict in exact fp32, node `output`."""
    import torch
    from tf_kaldi_speaker_amd import resnet_train
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights, feats, offsets = rr.small_model(5, **rr.NESTEROV)
    trainer = resnet_train.ResNetTrainer(Params(**params), weights, CLASSES, device=0, seed=3)
    got = trainer.forward(torch.from_numpy(feats).cuda(), offsets).cpu().numpy()
    tr = Trainer(Params(**params), None, rr.DIM, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights)
    tr.embeddings = "output"
    want = np.concatenate([tr.predict(feats[offsets[u]:offsets[u + 1]][None]) for u in range(len(rr.LENS))])
    tr.close()
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    print("forward() against Trainer.predict f32: relative L2 per row, largest %.3e" % float(err.max()))
    assert got.shape == want.shape == (len(rr.LENS), rr.LAST) and err.max() <= TOL


def _train(tmp_path, name, params, weights, pre, data, spklist, batch_norm="moving"):
    from tf_kaldi_speaker_amd import head_train, model_io
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    tr = Trainer(Params(**params), pre, rr.DIM, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    out = str(tmp_path / name)
    hist = head_train.train_head(tr, data, spklist, data, spklist, out, weights=weights, seed=5, precision="f32", conv_layers=True,
                                 batch_norm=batch_norm)
    tr.close()
    return hist, model_io.load_weights(os.path.join(out, "nnet"))[0], out


def test_train_head_writes_a_resnet_checkpoint(tmp_path):
    """train_head(conv_layers=True) on a synthetic data directory, one epoch of two steps: the checkpoint loads in Trainer, holds
    every trained kernel in its checkpoint shape, leaves every moving statistic byte-identical, and two runs with one seed write
    the same bits."""
    from tf_kaldi_speaker_amd import model_io, resnet_train, synth
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    extra = dict(num_speakers_per_batch=3, num_segments_per_speaker=2, min_segment_len=8, max_segment_len=12, valid_max_iterations=100,
                 num_steps_per_epoch=2, num_epochs=1, learning_rate=0.05, reduce_lr_epochs=2, **rr.NESTEROV)
    params, weights, _, _ = rr.small_model(5, **extra)
    pre = str(tmp_path / "pretrain")
    model_io.save_model(pre, params, rr.DIM, weights, step=77)
    rs = np.random.RandomState(21)
    spk_utts = [("spk%d" % s, ["spk%d-u%d" % (s, u) for u in range(3)]) for s in (3, 0, 1, 2)]
    lens = {u: int(t) for (_, us) in spk_utts for u, t in zip(us, rs.randint(14, 23, 12))}
    data, spklist, _ = make_data_dir(tmp_path, spk_utts, lens, dim=rr.DIM, spklist=[("spk%d" % s, s) for s in range(4)], seed=22)
    hist, saved, out = _train(tmp_path, "a", params, weights, pre, data, spklist)
    assert len(hist) == 1 and hist[0][1] == 2 and np.isfinite(hist[0][2])
    names = set(resnet_train.trained_names(params))
    assert set(saved) == set(weights) | {HEAD_K, HEAD_B}
    for k, v in saved.items():
        if k in weights:
            assert v.shape == np.shape(weights[k]), k                  # conv5 [1, 5, C, N], the convolutions HWIO
            changed = v.tobytes() != np.asarray(weights[k], np.float32).tobytes()
            assert changed == (k in names), k                          # every trained tensor moved; every moving statistic is as it was
    judge = Trainer(Params(**params), out, rr.DIM, single_cpu=True, device=0, precision="f32")
    judge.build("predict")
    emb = judge.predict(np.random.RandomState(3).standard_normal((1, 17, rr.DIM)).astype(np.float32))
    judge.close()
    assert np.all(np.isfinite(emb))
    _, again, _ = _train(tmp_path, "b", params, weights, pre, data, spklist)
    assert set(again) == set(saved) and all(again[k].tobytes() == saved[k].tobytes() for k in saved)
