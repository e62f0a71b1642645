"""GPU: training every frame-level layer, the multi-tap convolutions included, with the pooling, the segment-level layers and
the head (tf_kaldi_speaker_amd/conv_train.py) on a synth.py model of the smallest widths: steps against the replay of
tests/helpers/ref_conv_train.py, the saved checkpoint through Trainer.predict, what stays untouched, train_head with and
without the keyword, a separable toy set, and the extended TDNN.

The scheme is that of tests/test_gpu_frame_train.py, three steps of each optimizer replayed in float64 and the update judged
through ref_seg_grad.update_bound, with one change.  There the gradient's bound is composed stage by stage from the input to the
head.  That composition is a worst case: every layer multiplies what it is handed by sum_k |w_jk|, 2 to 8 at these widths, while
the signal keeps its size.  Behind seven layers, a first one of K = 150 among them, the composed bound of the output is 1 % of
the output and the composed bound of the first kernel's gradient is 75 times that gradient (measured on the CPU on these
shapes): it judges nothing, and no |h| is certain of its sign under it.  So every stage is judged where its bound is tight: ON
THE INPUT THE DEVICE HANDED IT.  Tap records what each layer, the pooling and the head were handed and gave back in the step;
check_stages holds each against its own float64 rule on exactly those float32 inputs, within its own per-element bound
(ref_tconv.bounds, ref_seg_grad.bounds, the bars of ref_pool_grad, ref_loss_grad.bounds), every element, and checks that each
stage was handed the very bits the stage before gave.  A wrong value anywhere in the chain fails the stage that made it.  The
gradients of the parameters are outputs of these stages; the replay of the update starts from the parameters and slots the
device held before the step and applies ref_loss_grad.opt_step in the kernel's float32 order to the float64 gradient, and the
device's new parameters must lie within update_bound of it.

Precondition, asserted for every layer on the input the device handed it, before every step: every h keeps 64 of its bounds from
zero.  The first layer's bound is 1e-4 of a typical h and it has 1 500 activations, so its frames are drawn clear of it
(toy_segments); the seeds, one per optimizer, were found on the CPU with the float64 rule standing in for the device
(host_replay below).  The pooling needs none: its rule is judged at the float32 mean, std and variance the device kept."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_conv_train as rc                                         # noqa: E402
import ref_loss_grad as rg                                          # noqa: E402
import ref_pool_grad as rpg                                         # noqa: E402
import ref_seg_grad as rs                                           # noqa: E402
import ref_tconv as rt                                              # noqa: E402
from test_gpu_head_train import run_train, train_setup              # noqa: E402

pytestmark = pytest.mark.gpu

DIM, CHANNELS, POOL, LAST, CLASSES = 30, 8, 24, 16, 3
LENGTHS = {"tdnn": (30, 33, 37, 40, 31, 35), "extended_tdnn": (34, 37, 41, 44, 35, 39)}      # context 14 and 22
NOISE = 0.5
MARGIN = 64.0
# with these seeds the precondition holds on all three steps, with a margin of 72 or more on the CPU (host_replay)
DATA_SEED = {("tdnn", "sgd"): 31, ("tdnn", "momentum"): 141, ("tdnn", "adam"): 92, ("extended_tdnn", "momentum"): 32}
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
# Adam moves every weight by about its rate per step whatever the gradient: at 0.05 three steps would move the 150-input sums of
# the first layer across zero
RATE = {"sgd": 0.05, "momentum": 0.05, "adam": 3e-4}


def toy_segments(seed, speakers, segments, lengths, noise=NOISE, first=None, margin=16.0 * MARGIN):
    """Packed features of a separable toy set: a centre per speaker plus a per-frame spread -> (feats [rows, DIM] float32,
    offsets int64, labels int32).  With `first` (the first layer, a ref_conv_train.Layer) the frames of a segment are drawn in
    order and frame s is redrawn until the output row it completes, s - (taps - 1), keeps `margin` bounds from zero in every
    channel, as tests/helpers/tconv_cases.py does: 150 inputs per output put the first layer's bound at 1e-4 of a typical h,
    and no seed clears its 1 500 activations by chance.  The margin is sixteen times the test's: three steps move the weights."""
    r = np.random.RandomState(seed)
    centres = r.standard_normal((speakers, DIM))
    labels = np.repeat(np.arange(speakers), segments)
    lens = [int(lengths[i % len(lengths)]) for i in range(labels.size)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    feats = np.zeros((int(off[-1]), DIM), dtype=np.float32)
    for u, (l, n) in enumerate(zip(labels, lens)):
        for s in range(int(off[u]), int(off[u + 1])):
            for _ in range(1000):
                feats[s] = (centres[l] + noise * r.standard_normal(DIM)).astype(np.float32)
                t = s - (first.taps - 1) if first is not None else -1
                if t < off[u]:
                    break
                fwd = rs.forward(feats[t:s + 1].reshape(1, -1), first.w, first.b, first.bn, first.act, rs.SLOPE)
                if np.all(np.abs(fwd["h"]) >= margin * rs.bounds(fwd)["h"]):
                    break
            else:
                raise AssertionError("no clear frame found")
    return feats, off, labels.astype(np.int32)


def first_layer(network_type):
    """The first frame layer of small_model (the optimizer does not enter the weights)."""
    from tf_kaldi_speaker_amd import conv_train
    params, weights = small_model(network_type=network_type)
    spec = conv_train.frame_variables(params)[0]
    rows, taps, _ = conv_train.kernel_to_rows(weights[spec.kernel])
    return rc.Layer(rows, weights[spec.bias], [weights[spec.bn + "/" + k] for k in BN], spec.act, taps)


def toy_batch(network_type, optimizer):
    return toy_segments(DATA_SEED[network_type, optimizer], CLASSES, 2, LENGTHS[network_type], first=first_layer(network_type))


def state_of(ct):
    """name -> (parameter, slots) as float32 numpy, kernels in the rows layout without the padding."""
    widths = {spec.kernel: layer.in_dim for spec, layer in zip(ct.specs, ct.layers)}
    widths[HEAD_K] = ct.embed_dim
    out = {}
    for name, w, _, slots in ct.tensors():
        cut = (lambda a, k=widths[name]: a[:, :k]) if name in widths else (lambda a: a)
        out[name] = (cut(w.cpu().numpy()).copy(), [cut(s.cpu().numpy()).copy() for s in slots])
    return out


def layer_of(spec, st, weights):
    bn = [st[spec.bn + "/gamma"][0], st[spec.bn + "/beta"][0], weights[spec.bn + "/moving_mean"], weights[spec.bn + "/moving_variance"]]
    return rc.Layer(st[spec.kernel][0], st[spec.bias][0], bn, spec.act, getattr(spec, "taps", 1))


def replay_layers(specs, st, weights):
    return [layer_of(spec, st, weights) for spec in specs]


def precondition(spec, fwd, margin=MARGIN):
    """Every h of the layer keeps `margin` of its bounds (ref_seg_grad.bounds on the input the layer saw) from zero -> the
    smallest |h| / bound."""
    if spec.act == rs.NONE:
        return float("inf")
    ratio = np.abs(fwd["h"]) / rs.bounds(fwd)["h"]
    assert np.all(ratio >= margin), ("an h of %s lies within %g bounds of zero" % (spec.kernel, margin), int((ratio < margin).sum()))
    return float(ratio.min())


class Tap(object):
    """Records what every stage of a ConvTrainer was handed and what it gave back, forward and backward, as numpy."""

    def __init__(self, ct):
        self.frame = [dict() for _ in ct.frame_layers]
        self.seg = [dict() for _ in ct.tail.layers]
        self.pool = dict()
        host = lambda t: None if t is None else t.detach().cpu().numpy().copy()          # noqa: E731
        for rec, layer in zip(self.frame, ct.frame_layers):
            def fwd(x, off, _f=layer.forward, _r=rec):
                y, oo = _f(x, off)
                _r.update(x=host(x), off=np.asarray(off, dtype=np.int64).copy(), y=host(y))
                return y, oo

            def bwd(gy, want, _b=layer.backward, _r=rec):
                gx = _b(gy, want)
                _r.update(gy=host(gy), gx=host(gx))
                return gx
            layer.forward, layer.backward = fwd, bwd
        for rec, layer in zip(self.seg, ct.tail.layers):
            def fwd(x, _f=layer.forward, _r=rec):
                y = _f(x)
                _r.update(x=host(x), y=host(y))
                return y

            def bwd(gy, want, _b=layer.backward, _r=rec):
                gx = _b(gy, want)
                _r.update(gy=host(gy), gx=host(gx))
                return gx
            layer.forward, layer.backward = fwd, bwd
        pool = ct.pool

        def pfwd(x, off, _f=pool.forward, _r=self.pool):
            pooled = _f(x, off)
            _r.update(x=host(x), off=[int(o) for o in off], pooled=host(pooled), var=host(pool._var)[:pooled.shape[0]])
            return pooled

        def pbwd(g, _b=pool.backward, _r=self.pool):
            gx = _b(g)
            _r.update(gp=host(g), gx=host(gx))
            return gx
        pool.forward, pool.backward = pfwd, pbwd


def within(got, want, bound, what, worst):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    ratio = float(np.max(err / (bound + 1e-300))) if np.any(err > 0) else 0.0
    worst[what] = max(worst.get(what, 0.0), ratio)
    assert ratio <= 1.0, (what, ratio)


def check_stages(tap, frame_specs, seg_specs, st, weights, labels, worst):
    """Every stage of the step against its float64 rule ON THE INPUT THE DEVICE HANDED IT, within the stage's own bound, every
    element; the precondition asserted on every layer -> (name -> (oracle gradient, its bound), the oracle's mean loss)."""
    grads = {}
    for spec, rec in zip(frame_specs, tap.frame):
        l = layer_of(spec, st, weights)
        fwd = rt.forward(rec["x"], rec["off"], l.taps, l.w, l.b, l.bn, l.act)
        precondition(spec, fwd)
        bwd = rt.backward(fwd, rec["gy"])
        bnd = rt.bounds(fwd, bwd)
        within(rec["y"], fwd["y"], bnd["y"], spec.kernel + " y", worst)
        if rec["gx"] is not None:
            within(rec["gx"], bwd["gx"], bnd["gx"], spec.kernel + " gx", worst)
        grads.update({spec.kernel: (bwd["gw"], bnd["gw"]), spec.bias: (bwd["gbias"], bnd["gbias"]),
                      spec.bn + "/gamma": (bwd["ggamma"], bnd["ggamma"]), spec.bn + "/beta": (bwd["gbeta"], bnd["gbeta"])})
    assert tap.frame[0]["gx"] is None                                   # the first layer's input gradient is never formed
    # statistics pooling of the last frame layer's rows: the bars of ref_pool_grad, at the float32 m, std, v the device kept
    p = tap.pool
    C = p["x"].shape[1]
    assert np.array_equal(p["x"], tap.frame[-1]["y"]) and np.array_equal(p["gx"], tap.frame[-1]["gy"])
    for u in range(len(p["off"]) - 1):
        xu = p["x"][p["off"][u]:p["off"][u + 1]]
        m, sd, v = p["pooled"][u, :C], p["pooled"][u, C:], p["var"][u]
        for r, what in zip(rpg.forward_ratios(xu, m, v, sd), ("pool mean", "pool variance", "pool std")):
            worst[what] = max(worst.get(what, 0.0), float(np.max(r)))
            assert np.all(r <= 1.0), (what, u, float(np.max(r)))
        within(p["gx"][p["off"][u]:p["off"][u + 1]], rpg.backward(xu, m, sd, v, p["gp"][u]), rpg.backward_bound(xu, m, sd, v, p["gp"][u]),
               "pool gx", worst)
    assert np.array_equal(tap.seg[0]["x"], p["pooled"]) and np.array_equal(tap.seg[0]["gx"], p["gp"])
    for spec, rec in zip(seg_specs, tap.seg):
        l = layer_of(spec, st, weights)
        fwd = rs.forward(rec["x"], l.w, l.b, l.bn, l.act, rs.SLOPE)
        precondition(spec, fwd)
        bwd = rs.backward(fwd, rec["gy"], rs.SLOPE)
        bnd = rs.bounds(fwd, bwd)
        within(rec["y"], fwd["y"], bnd["y"], spec.kernel + " y", worst)
        within(rec["gx"], bwd["gx"], bnd["gx"], spec.kernel + " gx", worst)
        grads.update({spec.kernel: (bwd["gw"], bnd["gw"]), spec.bias: (bwd["gbias"], bnd["gbias"]),
                      spec.bn + "/gamma": (bwd["ggamma"], bnd["ggamma"]), spec.bn + "/beta": (bwd["gbeta"], bnd["gbeta"])})
    assert np.array_equal(tap.seg[1]["x"], tap.seg[0]["y"]) and np.array_equal(tap.seg[1]["gx"], tap.seg[0]["gy"])
    hd = rg.classifier_grad(tap.seg[1]["y"], labels, st[HEAD_K][0].T.astype(np.float64), st[HEAD_B][0], "softmax", 0.0, 0.0)
    bx, bk, bb = rg.bounds(hd, LAST, CLASSES)
    within(tap.seg[1]["gy"], hd["grad_x"], bx, "head grad_x", worst)
    grads[HEAD_K] = (hd["grad_kernel"].T, bk.T)
    grads[HEAD_B] = (hd["grad_bias"], bb)
    return grads, float(np.mean(hd["loss"]))


def replay_update(params, l2, name, st, g, lr, t):
    from tf_kaldi_speaker_amd import head_train
    kind, mom, nest, _, clip = head_train.optimizer_config(params)
    w0, slots = st[name]
    s0 = slots[0] if slots else None
    s1 = slots[1] if len(slots) > 1 else None
    return rg.opt_step(kind, w0, f32(g), s0, s1, lr=lr, l2=l2[name], clip_norm=clip, momentum=mom, use_nesterov=nest, step=t)


def host_replay(params, weights, feats, offsets, labels, head_seed=3, steps=3, margin=72.0):
    """The three steps with the float64 rule standing in for the device (no GPU): raises AssertionError when a layer's
    precondition fails on a step, with a margin of 72, since the device's activations differ from the stand-in's by their
    rounding, a few bounds at the most.  This is how DATA_SEED was found.  -> the smallest |h| / bound met."""
    from tf_kaldi_speaker_amd import conv_train, head_train, tail_train
    fs, ss = conv_train.frame_variables(params), tail_train.segment_variables(params)
    kind = head_train.optimizer_config(params)[0]
    nslots = {rg.SGD: 0, rg.MOMENTUM: 1, rg.ADAM: 2}[kind]
    st = {}
    for spec in tuple(fs) + tuple(ss):
        for name, v in ((spec.kernel, conv_train.kernel_to_rows(weights[spec.kernel])[0]), (spec.bias, f32(weights[spec.bias])),
                        (spec.bn + "/gamma", f32(weights[spec.bn + "/gamma"])), (spec.bn + "/beta", f32(weights[spec.bn + "/beta"]))):
            st[name] = (v.copy(), [np.zeros_like(v) for _ in range(nslots)])
    hk = head_train.xavier_uniform(LAST, CLASSES, head_seed).T.copy()
    st[HEAD_K] = (hk, [np.zeros_like(hk) for _ in range(nslots)])
    st[HEAD_B] = (np.zeros(CLASSES, dtype=np.float32), [np.zeros(CLASSES, dtype=np.float32) for _ in range(nslots)])
    l2 = conv_train.l2_assignment(params)
    lr, least = RATE[params["optimizer"]], float("inf")
    for t in range(1, steps + 1):
        res = rc.conv_grads(replay_layers(fs, st, weights), replay_layers(ss, st, weights), st[HEAD_K][0].T, st[HEAD_B][0], feats,
                            offsets, labels)
        grads = {}
        for spec, fwd, bwd in zip(tuple(fs) + tuple(ss), res["frame_fwd"] + res["seg_fwd"], res["frame_bwd"] + res["seg_bwd"]):
            least = min(least, precondition(spec, fwd, margin))
            grads.update({spec.kernel: bwd["gw"], spec.bias: bwd["gbias"], spec.bn + "/gamma": bwd["ggamma"], spec.bn + "/beta": bwd["gbeta"]})
        grads[HEAD_K], grads[HEAD_B] = res["head"]["grad_kernel"].T, res["head"]["grad_bias"]
        new = {}
        for name, g in grads.items():
            w, m, v = replay_update(params, l2, name, st, g, lr, t)
            new[name] = (f32(w), [f32(s) for s in (m, v) if s is not None][:nslots])
        st = new
    return least


def three_steps(network_type, extra):
    from tf_kaldi_speaker_amd import conv_train, head_train
    from tf_kaldi_speaker_amd.params import Params
    import torch
    params, weights = small_model(network_type=network_type, **extra)
    feats, offsets, labels = toy_batch(network_type, extra["optimizer"])
    ct = conv_train.ConvTrainer(Params(**params), weights, CLASSES, device=0, seed=3)
    tap = Tap(ct)
    kind, mom, nest, _, clip = head_train.optimizer_config(params)
    l2 = conv_train.l2_assignment(params)
    feats_dev = torch.from_numpy(feats).cuda()
    lr, worst, stage_worst = RATE[extra["optimizer"]], 0.0, {}
    for t in range(1, 4):
        before = state_of(ct)
        res_dev = ct.step(feats_dev, offsets, labels, lr, global_step=t)
        after = state_of(ct)
        assert np.array_equal(tap.frame[0]["x"], feats)
        grads, loss = check_stages(tap, ct.frame_specs, ct.tail.specs, before, weights, labels, stage_worst)
        assert abs(res_dev.loss - loss) <= 1e-6 * max(1.0, abs(loss))
        assert set(grads) == set(before) == set(conv_train.trained_names(params))
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
    print("%s %s: largest error / bound over the three steps: updates %.3f, stages %s"
          % (network_type, extra["optimizer"], worst, " ".join("%s %.3f" % kv for kv in sorted(stage_worst.items()))))


@pytest.mark.parametrize("extra", OPTIMIZERS, ids=[o["optimizer"] for o in OPTIMIZERS])
def test_three_steps_against_the_replay(extra):
    three_steps("tdnn", extra)


def test_extended_tdnn_with_momentum():
    three_steps("extended_tdnn", OPTIMIZERS[1])


def test_saved_checkpoint_is_what_was_trained(tmp_path):
    import torch
    from tf_kaldi_speaker_amd import conv_train, model_io
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights = small_model(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=1e-3)
    feats, offsets, labels = toy_segments(9, 3, 2, (40,))                      # six segments of 40 frames: Trainer.predict takes [B, T, dim]
    ct = conv_train.ConvTrainer(Params(**params), weights, 3, device=0, seed=3)
    dev = torch.from_numpy(feats).cuda()
    for t in range(3):
        ct.step(dev, offsets, labels, 0.05, global_step=t)
    trained = ct.variables()
    out = dict(weights)
    out.update(trained)
    model_io.save_model(str(tmp_path / "m"), params, DIM, out, step=3)
    saved, step = model_io.load_weights(str(tmp_path / "m" / "nnet"))
    assert step == 3 and set(saved) == set(weights) | {HEAD_K, HEAD_B}
    names = set(conv_train.trained_names(params))
    assert set(trained) == names
    for k, v in weights.items():
        assert saved[k].shape == np.shape(v), k                                # the convolutions keep the checkpoint's rank
        if k in names:
            assert saved[k].tobytes() != f32(v).tobytes(), k                   # trained ...
            assert saved[k].tobytes() == trained[k].tobytes(), k
        else:
            assert saved[k].tobytes() == f32(v).tobytes(), k                   # ... or byte-identical, the moving statistics included
    assert saved["tdnn/tdnn1_conv/kernel"].ndim == 4 and saved["tdnn/tdnn3_conv/kernel"].shape == (1, 7, CHANNELS, CHANNELS)
    for spec in ct.specs:
        for s in ("moving_mean", "moving_variance"):
            assert saved[spec.bn + "/" + s].tobytes() == f32(weights[spec.bn + "/" + s]).tobytes()
    # the library's own forward of the saved model = ConvTrainer's forward, each within the composed bound of the float64 oracle
    judge = Trainer(Params(**params), str(tmp_path / "m"), DIM, single_cpu=True, device=0, precision="f32")
    judge.build("predict")
    judge.load_weights(saved, 0)
    judge.embeddings = "output"
    got = judge.predict(feats.reshape(6, 40, DIM))
    judge.close()
    mine = ct.forward(dev, offsets).cpu().numpy()
    st = {k: (conv_train.kernel_to_rows(saved[k])[0] if k.endswith("/kernel") else saved[k], []) for k in names}
    layers = replay_layers(ct.frame_specs, st, saved) + replay_layers(ct.tail.specs, st, saved)
    res = rc.conv_grads(layers[:-2], layers[-2:], saved[HEAD_K], saved[HEAD_B], feats, offsets, labels)
    total = rc.conv_grad_bounds(res, LAST, 3)["forward_output"]
    want = res["seg_fwd"][1]["y"]
    diff = np.abs(got.astype(np.float64) - mine)
    print("ConvTrainer.forward against the oracle: largest error / bound %.3f; predict against it: largest difference / bound %.3f"
          % (float(np.max(np.abs(mine - want) / (total + 1e-300))), float(np.max(diff / (2.0 * total + 1e-300)))))
    assert np.all(np.abs(mine - want) <= total)
    assert np.all(diff <= 2.0 * total)
    # the composed bound is a worst case through seven layers (the module docstring), about 1 % of the output: the cap that
    # judges is the project's parity requirement, 1e-4 relative L2 per embedding, for both forwards against the oracle
    for what, emb in (("ConvTrainer.forward", mine), ("Trainer.predict", got)):
        rel = np.linalg.norm(emb - want, axis=1) / np.linalg.norm(want, axis=1)
        print("%s: relative L2 against the oracle, largest %.3e" % (what, float(rel.max())))
        assert rel.max() <= 1e-4, (what, float(rel.max()))


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
    hist_b = head_train.train_head(tr, data, spklist, data, spklist, out_b, weights=weights, seed=5, precision="f32", conv_layers=False)
    tr.close()
    assert hist_a == hist_b
    a, _ = model_io.load_weights(os.path.join(out_a, "nnet"))
    b, _ = model_io.load_weights(os.path.join(out_b, "nnet"))
    assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_train_head_with_conv_layers(tmp_path):
    from tf_kaldi_speaker_amd import conv_train, head_train, model_io
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights, pre, data, spklist = train_setup(tmp_path)
    tr = Trainer(Params(**params), pre, 30, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    endpoint = tr.embeddings
    out = str(tmp_path / "convs")
    lines = []
    hist = head_train.train_head(tr, data, spklist, data, spklist, out, weights=weights, seed=5, precision="f32", conv_layers=True,
                                 log=lines.append)
    assert tr.embeddings == endpoint
    tr.close()
    assert len(hist) == 1 and hist[0][1] == 4 and np.isfinite(hist[0][2])
    assert sum(1 for l in lines if " step " in l and " loss " in l and "valid" not in l) == 4
    saved, step = model_io.load_weights(os.path.join(out, "nnet"))
    names = set(conv_train.trained_names(params))
    assert step == 4 and set(saved) == set(weights) and saved[HEAD_K].shape == (16, 6)
    assert {"tdnn/tdnn1_conv/kernel", "tdnn/tdnn3_bn/gamma", "tdnn/tdnn4_dense/kernel", "tdnn/tdnn6_dense/kernel"} <= names
    for k, v in weights.items():
        assert k.startswith("softmax/") or saved[k].shape == np.shape(v), k      # the head is new: another speaker list
        if k in names:
            assert saved[k].tobytes() != f32(v).tobytes(), k
        else:
            assert saved[k].tobytes() == f32(v).tobytes(), k


def test_separable_toy_set_is_learned():
    import torch
    from tf_kaldi_speaker_amd import conv_train
    from tf_kaldi_speaker_amd.params import Params
    params, weights = small_model(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=0.0)
    feats, offsets, labels = toy_segments(2, 8, 4, LENGTHS["tdnn"], noise=0.5)
    ct = conv_train.ConvTrainer(Params(**params), weights, 8, device=0, seed=0)
    dev = torch.from_numpy(feats).cuda()
    # the same two steps with a `mark` callback on a twin: the same bits, and every stage named once, in the documented order
    twin, seen, losses = conv_train.ConvTrainer(Params(**params), weights, 8, device=0, seed=0), [], []
    for t in range(2):
        losses.append(ct.step(dev, offsets, labels, 0.1, global_step=t).loss)
        assert twin.step(dev, offsets, labels, 0.1, global_step=t, mark=seen.append).loss == losses[-1]
        a, b = ct.variables(), twin.variables()
        assert list(a) == list(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
    n = len(ct.frame_layers)
    assert seen == 2 * (["start"] + ["frame_forward/%d" % i for i in range(n)]
                        + ["frame_forward", "pool_forward", "segment_forward", "head", "segment_backward", "pool_backward"]
                        + ["frame_backward/%d" % i for i in range(n - 1, -1, -1)] + ["frame_backward", "optimizer"])
    losses += [ct.step(dev, offsets, labels, 0.1, global_step=t).loss for t in range(2, 20)]
    print("separable toy set: mean loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
