"""GPU: training the trailing 1-tap frame layers, through statistics pooling, with the segment-level layers and the head
(tf_kaldi_speaker_amd/frame_train.py) on a synth.py model of the smallest widths: steps against the replay of
tests/helpers/ref_pool_grad.py, the saved checkpoint through Trainer.predict, what stays frozen, train_head with and without
the keyword, a separable toy set, and the extended TDNN's three-layer chain.

The replay of step t starts from the parameters and optimizer slots the device held before step t: the float64 rule
(ref_pool_grad.frame_grads) gives the gradients, rounded to float32, and ref_loss_grad.opt_step applies the update in the
kernel's float32 order.  What the device holds after the step must lie within ref_seg_grad.update_bound of it, with the gradient's
bound composed stage by stage in ref_pool_grad.frame_grad_bounds; this is asserted after each of the three steps.

Precondition, asserted on what the device holds before every step: every h of every layer keeps 64 of its bounds from zero (the
error its input hands on included), every pooled variance lies outside 1e-12 +- its bound, every live std is at least 64 times
its bound.  The data seeds were found on the CPU with the float64 rule standing in for the device (host_replay below)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pool_grad_cases as pc                                        # noqa: E402
import ref_loss_grad as rg                                          # noqa: E402
import ref_pool_grad as rpg                                         # noqa: E402
import ref_seg_grad as rs                                           # noqa: E402
import seg_grad_cases as sc                                         # noqa: E402
from test_gpu_head_train import run_train, train_setup              # noqa: E402

pytestmark = pytest.mark.gpu

DIM, CHANNELS, POOL, LAST, CLASSES = 30, 8, 24, 16, 3
LENGTHS = (16, 19, 23, 26, 17, 21)        # what 30- to 40-frame segments leave behind tdnn3_relu (context 14)
DATA_SEED = {"tdnn": 20, "extended_tdnn": 12}      # with these seeds the precondition holds on all three steps of every optimizer below
BN = ("gamma", "beta", "moving_mean", "moving_variance")
HEAD_K, HEAD_B = "softmax/output/kernel", "softmax/output/bias"


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


def toy_batch(network_type="tdnn"):
    return pc.separable_frames(DATA_SEED[network_type], CLASSES, 2, CHANNELS, LENGTHS)


def state_of(ft):
    """name -> (parameter, slots) as float32 numpy, kernels in the rows layout without the padding."""
    widths = {spec.kernel: layer.in_dim for spec, layer in zip(ft.specs, ft.layers)}
    widths[HEAD_K] = ft.embed_dim
    out = {}
    for name, w, _, slots in ft.tensors():
        cut = (lambda a, k=widths[name]: a[:, :k]) if name in widths else (lambda a: a)
        out[name] = (cut(w.cpu().numpy()).copy(), [cut(s.cpu().numpy()).copy() for s in slots])
    return out


def replay_layers(specs, st, weights):
    layers = []
    for spec in specs:
        bn = [st[spec.bn + "/gamma"][0], st[spec.bn + "/beta"][0], weights[spec.bn + "/moving_mean"], weights[spec.bn + "/moving_variance"]]
        layers.append(rs.Layer(st[spec.kernel][0], st[spec.bias][0], bn, spec.act))
    return layers


def oracle_step(frame_specs, seg_specs, st, weights, frames, offsets, labels):
    """The float64 step at the state `st`, its composed bounds, the precondition asserted -> (res, bounds, name -> (g, dg))."""
    fl, sl = replay_layers(frame_specs, st, weights), replay_layers(seg_specs, st, weights)
    res = rpg.frame_grads(fl, sl, st[HEAD_K][0].T, st[HEAD_B][0], frames, offsets, labels)
    bnd = rpg.frame_grad_bounds(res, LAST, CLASSES)
    fwds = res["frame_fwd"] + res["seg_fwd"]
    for i, (spec, fwd, eh) in enumerate(zip(tuple(frame_specs) + tuple(seg_specs), fwds, bnd["extra_h"])):
        sc.precondition(dict(act=spec.act, name=spec.kernel), fwd, extra_h=eh)
    rpg.pool_precondition(bnd["pool"])
    grads = {}
    for spec, bwd, o in zip(tuple(frame_specs) + tuple(seg_specs), res["frame_bwd"] + res["seg_bwd"], bnd["frame"] + bnd["seg"]):
        grads[spec.kernel] = (bwd["gw"], o["w"])
        grads[spec.bias] = (bwd["gbias"], o["b"])
        grads[spec.bn + "/gamma"] = (bwd["ggamma"], o["gamma"])
        grads[spec.bn + "/beta"] = (bwd["gbeta"], o["beta"])
    grads[HEAD_K] = (res["head"]["grad_kernel"].T, bnd["head_kernel"].T)
    grads[HEAD_B] = (res["head"]["grad_bias"], bnd["head_bias"])
    return res, bnd, grads


def replay_update(params, l2, name, st, g, lr, t):
    from tf_kaldi_speaker_amd import head_train
    kind, mom, nest, _, clip = head_train.optimizer_config(params)
    w0, slots = st[name]
    s0 = slots[0] if slots else None
    s1 = slots[1] if len(slots) > 1 else None
    return rg.opt_step(kind, w0, f32(g), s0, s1, lr=lr, l2=l2[name], clip_norm=clip, momentum=mom, use_nesterov=nest, step=t)


def host_replay(params, weights, frames, offsets, labels, head_seed=3, lr=0.05, steps=3):
    """The three steps with the float64 rule standing in for the device (no GPU): raises AssertionError when a precondition
    fails on a step.  This is how DATA_SEED was found."""
    from tf_kaldi_speaker_amd import frame_train, head_train, tail_train
    fs, ss = frame_train.frame_variables(params), tail_train.segment_variables(params)
    kind = head_train.optimizer_config(params)[0]
    nslots = {rg.SGD: 0, rg.MOMENTUM: 1, rg.ADAM: 2}[kind]
    st = {}
    for spec in tuple(fs) + tuple(ss):
        for name, v in ((spec.kernel, f32(weights[spec.kernel]).T), (spec.bias, f32(weights[spec.bias])),
                        (spec.bn + "/gamma", f32(weights[spec.bn + "/gamma"])), (spec.bn + "/beta", f32(weights[spec.bn + "/beta"]))):
            st[name] = (v.copy(), [np.zeros_like(v) for _ in range(nslots)])
    hk = head_train.xavier_uniform(LAST, CLASSES, head_seed).T.copy()
    st[HEAD_K] = (hk, [np.zeros_like(hk) for _ in range(nslots)])
    st[HEAD_B] = (np.zeros(CLASSES, dtype=np.float32), [np.zeros(CLASSES, dtype=np.float32) for _ in range(nslots)])
    l2 = frame_train.l2_assignment(params)
    for t in range(1, steps + 1):
        _, _, grads = oracle_step(fs, ss, st, weights, frames, offsets, labels)
        new = {}
        for name, (g, _) in grads.items():
            w, m, v = replay_update(params, l2, name, st, g, lr, t)
            new[name] = (f32(w), [f32(s) for s in (m, v) if s is not None][:nslots])
        st = new
    return st


def three_steps(network_type, extra):
    from tf_kaldi_speaker_amd import frame_train, head_train
    from tf_kaldi_speaker_amd.params import Params
    import torch
    params, weights = small_model(network_type=network_type, **extra)
    frames, offsets, labels = toy_batch(network_type)
    ft = frame_train.FrameTrainer(Params(**params), weights, CLASSES, device=0, seed=3)
    kind = head_train.optimizer_config(params)[0]
    _, mom, nest, _, clip = head_train.optimizer_config(params)
    l2 = frame_train.l2_assignment(params)
    frames_dev = torch.from_numpy(frames).cuda()
    lr, worst = 0.05, 0.0
    for t in range(1, 4):
        before = state_of(ft)
        res_dev = ft.step(frames_dev, offsets, labels, lr, global_step=t)
        after = state_of(ft)
        res, _, grads = oracle_step(ft.frame_specs, ft.tail.specs, before, weights, frames, offsets, labels)
        assert abs(res_dev.loss - float(np.mean(res["head"]["loss"]))) <= 1e-4 * max(1.0, abs(res_dev.loss))
        assert set(grads) == set(before) == set(frame_train.trained_names(params))
        for name, (g, dg) in grads.items():
            w0, slots = before[name]
            s0 = slots[0] if slots else None
            s1 = slots[1] if len(slots) > 1 else None
            want = replay_update(params, l2, name, before, g, lr, t)[0]
            bound = rs.update_bound(kind, g, dg + rs.U * np.abs(g), s0, s1, lr, clip, mom, nest, t, w0, l2[name])
            err = np.abs(after[name][0].astype(np.float64) - want)
            ratio = float(np.max(err / (bound + 1e-300)))
            worst = max(worst, ratio)
            moved = float(np.max(np.abs(after[name][0] - w0)))
            print("%s %s step %d %s: error/bound %.3f, largest update %.3e, largest bound %.3e"
                  % (network_type, extra["optimizer"], t, name, ratio, moved, float(np.max(bound))))
            assert ratio <= 1.0, (name, t, ratio)
            assert np.median(bound) <= 0.1 * moved, (name, "the bound is no blanket: it stays far below the update it judges")
    print("%s %s: largest error / bound over the three steps %.3f" % (network_type, extra["optimizer"], worst))


@pytest.mark.parametrize("extra", OPTIMIZERS, ids=[o["optimizer"] for o in OPTIMIZERS])
def test_three_steps_against_the_replay(extra):
    three_steps("tdnn", extra)


def test_extended_tdnn_three_layer_chain():
    three_steps("extended_tdnn", OPTIMIZERS[1])


def frozen_frames(params, weights, feats):
    """The packed rows of the frozen node for feats [B, T, DIM], on the device, and their offsets."""
    import torch
    from tf_kaldi_speaker_amd import frame_train
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    tr = Trainer(Params(**params), None, DIM, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    b, t, _ = feats.shape
    dev = torch.from_numpy(np.ascontiguousarray(feats.reshape(b * t, -1), dtype=np.float32)).cuda()
    frames = tr.predict_packed(dev, np.arange(b + 1, dtype=np.int32) * t, frame_train.frozen_node(params)).clone()
    torch.cuda.synchronize()
    tr.close()
    per = int(frames.shape[0]) // b
    assert per * b == int(frames.shape[0]) and per == t - 14
    return frames, np.arange(b + 1, dtype=np.int64) * per


def test_saved_checkpoint_is_what_was_trained(tmp_path):
    from tf_kaldi_speaker_amd import frame_train, model_io, synth
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights = small_model(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=1e-3)
    feats = np.stack(synth.synth_features(6, 40, DIM, seed=9))
    frames, offsets = frozen_frames(params, weights, feats)
    labels = np.arange(6, dtype=np.int32) % 3
    ft = frame_train.FrameTrainer(Params(**params), weights, 3, device=0, seed=3)
    for t in range(3):
        ft.step(frames, offsets, labels, 0.05, global_step=t)
    trained = ft.variables()
    out = dict(weights)
    out.update(trained)
    model_io.save_model(str(tmp_path / "m"), params, DIM, out, step=3)
    saved, step = model_io.load_weights(str(tmp_path / "m" / "nnet"))
    assert step == 3 and set(saved) == set(weights) | {HEAD_K, HEAD_B}
    names = set(frame_train.trained_names(params))
    assert set(trained) == names
    for k, v in weights.items():
        if k in names:
            assert saved[k].tobytes() != f32(v).tobytes(), k                   # trained ...
            assert saved[k].tobytes() == trained[k].tobytes(), k
        else:
            assert saved[k].tobytes() == f32(v).tobytes(), k                   # ... or byte-identical, the moving statistics included
    for spec in ft.specs:
        for s in ("moving_mean", "moving_variance"):
            assert saved[spec.bn + "/" + s].tobytes() == f32(weights[spec.bn + "/" + s]).tobytes()
    # the library's own forward of the saved model = FrameTrainer's forward, each within the composed bound of the float64 oracle
    judge = Trainer(Params(**params), str(tmp_path / "m"), DIM, single_cpu=True, device=0, precision="f32")
    judge.build("predict")
    judge.load_weights(saved, 0)
    judge.embeddings = "output"
    got = judge.predict(feats)
    judge.close()
    mine = ft.forward(frames, offsets).cpu().numpy()
    layers = [rs.Layer(saved[spec.kernel].T, saved[spec.bias], [saved[spec.bn + "/" + s] for s in BN], spec.act) for spec in ft.specs]
    res = rpg.frame_grads(layers[:-2], layers[-2:], saved[HEAD_K], saved[HEAD_B], frames.cpu().numpy(), offsets, labels)
    total = rpg.frame_grad_bounds(res, LAST, 3)["forward_output"]
    want = res["seg_fwd"][1]["y"]
    diff = np.abs(got.astype(np.float64) - mine)
    print("FrameTrainer.forward against the oracle: largest error / bound %.3f; predict against it: largest difference / bound %.3f"
          % (float(np.max(np.abs(mine - want) / (total + 1e-300))), float(np.max(diff / (2.0 * total + 1e-300)))))
    assert np.all(np.abs(mine - want) <= total)
    assert np.all(diff <= 2.0 * total)
    assert np.max(total) <= 1e-3 * np.max(np.abs(want))                         # the bound is no blanket


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
    hist_b = head_train.train_head(tr, data, spklist, data, spklist, out_b, weights=weights, seed=5, precision="f32", frame_layers=False)
    tr.close()
    assert hist_a == hist_b
    a, _ = model_io.load_weights(os.path.join(out_a, "nnet"))
    b, _ = model_io.load_weights(os.path.join(out_b, "nnet"))
    assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_train_head_with_frame_layers(tmp_path):
    from tf_kaldi_speaker_amd import frame_train, head_train, model_io
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights, pre, data, spklist = train_setup(tmp_path)
    tr = Trainer(Params(**params), pre, 30, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    endpoint = tr.embeddings
    out = str(tmp_path / "frames")
    hist = head_train.train_head(tr, data, spklist, data, spklist, out, weights=weights, seed=5, precision="f32", frame_layers=True)
    assert tr.embeddings == endpoint
    tr.close()
    assert len(hist) == 1 and hist[0][1] == 4 and np.isfinite(hist[0][2])
    saved, step = model_io.load_weights(os.path.join(out, "nnet"))
    names = set(frame_train.trained_names(params))
    assert step == 4 and set(saved) == set(weights) and saved[HEAD_K].shape == (16, 6)
    assert {"tdnn/tdnn4_dense/kernel", "tdnn/tdnn5_bn/gamma", "tdnn/tdnn6_dense/kernel"} <= names
    for k, v in weights.items():
        if k in names:
            assert saved[k].tobytes() != f32(v).tobytes(), k
        else:
            assert saved[k].tobytes() == f32(v).tobytes(), k


def test_separable_toy_set_is_learned():
    import torch
    from tf_kaldi_speaker_amd import frame_train
    from tf_kaldi_speaker_amd.params import Params
    params, weights = small_model(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=0.0)
    frames, offsets, labels = pc.separable_frames(2, 8, 4, CHANNELS, LENGTHS)
    ft = frame_train.FrameTrainer(Params(**params), weights, 8, device=0, seed=0)
    dev = torch.from_numpy(frames).cuda()
    # the same two steps with a `mark` callback on a twin: the same bits, and every stage named once, in the documented order
    twin, seen, losses = frame_train.FrameTrainer(Params(**params), weights, 8, device=0, seed=0), [], []
    for t in range(2):
        losses.append(ft.step(dev, offsets, labels, 0.1, global_step=t).loss)
        assert twin.step(dev, offsets, labels, 0.1, global_step=t, mark=seen.append).loss == losses[-1]
        a, b = ft.variables(), twin.variables()
        assert list(a) == list(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
    n = len(ft.frame_layers)
    assert seen == 2 * (["start"] + ["frame_forward/%d" % i for i in range(n)]
                        + ["frame_forward", "pool_forward", "segment_forward", "head", "segment_backward", "pool_backward"]
                        + ["frame_backward/%d" % i for i in range(n - 1, -1, -1)] + ["frame_backward", "optimizer"])
    losses += [ft.step(dev, offsets, labels, 0.1, global_step=t).loss for t in range(2, 20)]
    print("separable toy set: mean loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
