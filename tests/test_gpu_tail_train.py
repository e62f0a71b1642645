"""GPU: training the two segment-level layers with the head (tf_kaldi_speaker_amd/tail_train.py) on a synth.py model of the
smallest widths: steps against the replay of tests/helpers/ref_seg_grad.py, the saved checkpoint through Trainer.predict, what
stays frozen, train_head with and without the keyword, and a separable toy set.

The replay of step t starts from the parameters and optimizer slots the device held before step t: the float64 rule
(ref_seg_grad.tail_grads) gives the gradients, rounded to float32, and ref_loss_grad.opt_step applies the update in the
kernel's float32 order.  What the device holds after the step must lie within ref_seg_grad.update_bound of it, with the
gradient's bound composed stage by stage in ref_seg_grad.tail_grad_bounds; this is asserted after each of the three steps, so
the parameters after step 3 carry the bounds of all three."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_loss_grad as rg                                          # noqa: E402
import ref_seg_grad as rs                                           # noqa: E402
import seg_grad_cases as sc                                         # noqa: E402
from test_gpu_head_train import run_train, train_setup              # noqa: E402

pytestmark = pytest.mark.gpu

DIM, CHANNELS, POOL, LAST, CLASSES = 30, 8, 24, 16, 3
DATA_SEED = 2       # with this seed every h of both layers keeps 64 bounds from zero over the three steps of all three optimizers:
#                     found on the CPU with the float64 rule as the device; the test asserts it again on what the device holds


def f32(a):
    return np.asarray(a, dtype=np.float32)


def small_model(seed=4, **extra):
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.TDNN_STAT_PARAMS, num_nodes_pooling_layer=POOL, num_nodes_last_layer=LAST, **extra)
    return params, synth.synth_weights(params, DIM, seed=seed, channels=CHANNELS)


OPTIMIZERS = [
    dict(optimizer="sgd", weight_l2_regularizer=1e-2, clip_gradient=True, clip_gradient_norm=0.5),
    dict(optimizer="momentum", momentum=0.9, use_nesterov=True, weight_l2_regularizer=1e-3),
    dict(optimizer="adam", weight_l2_regularizer=0.0),
]


def state_of(tt):
    """name -> (parameter, slots) as float32 numpy, kernels in the rows layout without the padding."""
    out = {}
    for name, w, _, slots in tt.tensors():
        cut = (lambda a: a[:, :tt.pool_dim]) if name == tt.specs[0].kernel else (
            (lambda a: a[:, :tt.layers[1].in_dim]) if name == tt.specs[1].kernel else (
                (lambda a: a[:, :tt.embed_dim]) if name == "softmax/output/kernel" else (lambda a: a)))
        out[name] = (cut(w.cpu().numpy()).copy(), [cut(s.cpu().numpy()).copy() for s in slots])
    return out


def replay_layers(tt, st, weights):
    layers = []
    for spec in tt.specs:
        bn = None
        if spec.bn:
            bn = [st[spec.bn + "/gamma"][0], st[spec.bn + "/beta"][0], weights[spec.bn + "/moving_mean"], weights[spec.bn + "/moving_variance"]]
        layers.append(rs.Layer(st[spec.kernel][0], st[spec.bias][0], bn, spec.act))
    return layers


@pytest.mark.parametrize("extra", OPTIMIZERS, ids=[o["optimizer"] for o in OPTIMIZERS])
def test_three_steps_against_the_replay(extra):
    from tf_kaldi_speaker_amd import head_train, tail_train
    from tf_kaldi_speaker_amd.params import Params
    params, weights = small_model(**extra)
    x, labels = sc.separable_pooled(DATA_SEED, CLASSES, 2, 2 * POOL)
    tt = tail_train.TailTrainer(Params(**params), weights, CLASSES, device=0, seed=3)
    kind, mom, nest, _, clip = head_train.optimizer_config(params)
    l2 = tail_train.l2_assignment(params)
    lr = 0.05
    worst = 0.0
    for t in range(1, 4):
        before = state_of(tt)
        res = tt.step(x, labels, lr, global_step=t)
        after = state_of(tt)
        layers = replay_layers(tt, before, weights)
        hw, hb = before["softmax/output/kernel"][0], before["softmax/output/bias"][0]
        f1, f2, hd, b1, b2 = rs.tail_grads(layers, hw.T, hb, x, labels)
        # the masks of the step are certain: every h keeps 64 bounds from zero, the error of layer 2's input included
        sc.precondition(dict(act=tt.specs[0].act, name="layer 1"), f1)
        in2 = rs.bounds(f1)["y"] @ np.abs(f2["w"]).T
        sc.precondition(dict(act=tt.specs[1].act, name="layer 2"), f2, extra_h=np.abs(f2["bn"][0] * f2["r"])[None, :] * in2)
        assert abs(res.loss - float(np.mean(hd["loss"]))) <= 1e-4 * max(1.0, abs(res.loss))
        o1, o2, hk, hbb = rs.tail_grad_bounds(f1, f2, hd, b1, b2, LAST, CLASSES)
        grads = {tt.specs[0].kernel: (b1["gw"], o1["w"]), tt.specs[0].bias: (b1["gbias"], o1["b"]),
                 tt.specs[0].bn + "/gamma": (b1["ggamma"], o1["gamma"]), tt.specs[0].bn + "/beta": (b1["gbeta"], o1["beta"]),
                 tt.specs[1].kernel: (b2["gw"], o2["w"]), tt.specs[1].bias: (b2["gbias"], o2["b"]),
                 tt.specs[1].bn + "/gamma": (b2["ggamma"], o2["gamma"]), tt.specs[1].bn + "/beta": (b2["gbeta"], o2["beta"]),
                 "softmax/output/kernel": (hd["grad_kernel"].T, hk.T), "softmax/output/bias": (hd["grad_bias"], hbb)}
        assert set(grads) == set(before)
        for name, (g, dg) in grads.items():
            w0, slots = before[name]
            s0 = slots[0] if slots else None
            s1 = slots[1] if len(slots) > 1 else None
            want = rg.opt_step(kind, w0, f32(g), s0, s1, lr=lr, l2=l2[name], clip_norm=clip, momentum=mom, use_nesterov=nest, step=t)[0]
            bound = rs.update_bound(kind, g, dg + rs.U * np.abs(g), s0, s1, lr, clip, mom, nest, t, w0, l2[name])
            err = np.abs(after[name][0].astype(np.float64) - want)
            ratio = float(np.max(err / (bound + 1e-300)))
            worst = max(worst, ratio)
            moved = float(np.max(np.abs(after[name][0] - w0)))
            print("%s step %d %s: error/bound %.3f, largest update %.3e, largest bound %.3e" % (extra["optimizer"], t, name, ratio, moved,
                                                                                              float(np.max(bound))))
            assert ratio <= 1.0, (name, t, ratio)
            assert np.median(bound) <= 0.1 * moved, (name, "the bound is no blanket: it stays far below the update it judges")
    print("%s: largest error / bound over the three steps %.3f" % (extra["optimizer"], worst))


def test_saved_checkpoint_is_what_was_trained(tmp_path):
    from tf_kaldi_speaker_amd import model_io, synth, tail_train
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights = small_model(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=1e-3)
    tr = Trainer(Params(**params), None, DIM, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    feats = np.stack(synth.synth_features(6, 40, DIM, seed=9))
    tr.embeddings = "pooling"
    pooled = f32(tr.predict(feats))
    tr.close()
    labels = np.arange(6, dtype=np.int32) % 3
    tt = tail_train.TailTrainer(Params(**params), weights, 3, device=0, seed=3)
    for t in range(3):
        tt.step(pooled, labels, 0.05, global_step=t)
    trained = tt.variables()
    out = dict(weights)
    out.update(trained)
    model_io.save_model(str(tmp_path / "m"), params, DIM, out, step=3)
    saved, step = model_io.load_weights(str(tmp_path / "m" / "nnet"))
    assert step == 3 and set(saved) == set(weights) | {"softmax/output/kernel", "softmax/output/bias"}
    names = set(tail_train.trained_names(params))
    for k, v in weights.items():
        if k in names:
            assert saved[k].tobytes() != f32(v).tobytes(), k                   # trained ...
            assert saved[k].tobytes() == trained[k].tobytes(), k
        else:
            assert saved[k].tobytes() == f32(v).tobytes(), k                   # ... or byte-identical, the moving statistics included
    for spec in tt.specs:
        for s in ("moving_mean", "moving_variance"):
            assert saved[spec.bn + "/" + s].tobytes() == f32(weights[spec.bn + "/" + s]).tobytes()
    # the library's own forward of the saved model = TailTrainer's forward, each within its bound of the float64 oracle
    judge = Trainer(Params(**params), str(tmp_path / "m"), DIM, single_cpu=True, device=0, precision="f32")
    judge.build("predict")
    judge.load_weights(saved, 0)
    judge.embeddings = "output"
    got = judge.predict(feats)
    judge.close()
    mine = tt.forward(pooled).cpu().numpy()
    layers = []
    for spec in tt.specs:
        layers.append(rs.Layer(saved[spec.kernel].T, saved[spec.bias], [saved[spec.bn + "/" + s] for s in ("gamma", "beta", "moving_mean",
                                                                                                            "moving_variance")], spec.act))
    f1 = rs.forward(pooled, layers[0].w, layers[0].b, layers[0].bn, layers[0].act, rs.SLOPE)
    f2 = rs.forward(f1["y"], layers[1].w, layers[1].b, layers[1].bn, layers[1].act, rs.SLOPE)
    e1, e2 = rs.bounds(f1), rs.bounds(f2)
    total = e2["y"] + np.abs(f2["bn"][0] * f2["r"])[None, :] * (e1["y"] @ np.abs(f2["w"]).T)      # both forward bounds
    diff = np.abs(got.astype(np.float64) - mine)
    print("predict against TailTrainer.forward: largest difference / bound %.3f" % float(np.max(diff / (2.0 * total + 1e-300))))
    assert np.all(np.abs(mine - f2["y"]) <= total)
    assert np.all(diff <= 2.0 * total)


def test_the_keyword_left_out_changes_no_bit(tmp_path):
    from tf_kaldi_speaker_amd import head_train, model_io
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights, pre, data, spklist = train_setup(tmp_path)
    out_a, hist_a = run_train(tmp_path, "without", params, weights, pre, data, spklist)
    tr = Trainer(Params(**params), pre, 30, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    out_b = str(tmp_path / "with_false")
    hist_b = head_train.train_head(tr, data, spklist, data, spklist, out_b, weights=weights, seed=5, precision="f32", segment_layers=False)
    tr.close()
    assert hist_a == hist_b
    a, _ = model_io.load_weights(os.path.join(out_a, "nnet"))
    b, _ = model_io.load_weights(os.path.join(out_b, "nnet"))
    assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_train_head_with_segment_layers(tmp_path):
    from tf_kaldi_speaker_amd import head_train, model_io, tail_train
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights, pre, data, spklist = train_setup(tmp_path)
    tr = Trainer(Params(**params), pre, 30, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    endpoint = tr.embeddings
    out = str(tmp_path / "tail")
    hist = head_train.train_head(tr, data, spklist, data, spklist, out, weights=weights, seed=5, precision="f32", segment_layers=True)
    assert tr.embeddings == endpoint
    tr.close()
    assert len(hist) == 1 and hist[0][1] == 4 and np.isfinite(hist[0][2])
    saved, step = model_io.load_weights(os.path.join(out, "nnet"))
    names = set(tail_train.trained_names(params))
    assert step == 4 and set(saved) == set(weights) and saved["softmax/output/kernel"].shape == (16, 6)
    for k, v in weights.items():
        if k in names:
            assert saved[k].tobytes() != f32(v).tobytes(), k
        else:
            assert saved[k].tobytes() == f32(v).tobytes(), k


def test_separable_toy_set_is_learned():
    from tf_kaldi_speaker_amd import tail_train
    from tf_kaldi_speaker_amd.params import Params
    params, weights = small_model(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=0.0)
    x, labels = sc.separable_pooled(2, 8, 4, 2 * POOL)
    tt = tail_train.TailTrainer(Params(**params), weights, 8, device=0, seed=0)
    losses = [tt.step(x, labels, 0.1, global_step=t).loss for t in range(20)]
    print("separable toy set: mean loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
