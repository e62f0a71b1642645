"""Host: the rule of xv_stat_pool_forward / xv_stat_pool_backward (tests/helpers/ref_pool_grad.py) against torch.autograd in
float64 on a restatement of model/pooling.py:41-50, the float64 step of the whole frame-level chain (frame_grads) against
autograd of that chain, the float32 emulations of both kernels inside the bars and the bound on every case of
tests/helpers/pool_grad_cases.py, and five mutants that each leave one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pool_grad_cases as pc                                        # noqa: E402
import ref_pool_grad as rpg                                         # noqa: E402
import ref_seg_grad as rs                                           # noqa: E402


def torch_pool(xt):
    """model/pooling.py:41-50 on [n, C]: the mask is computed from the variance and enters as a constant factor."""
    import torch
    mean = xt.mean(dim=0, keepdim=True)
    variance = ((xt - mean) ** 2).mean(dim=0, keepdim=True)
    mask = (variance <= 1e-12).to(torch.float64).detach()               # tf.to_float(tf.less_equal(...)): no gradient
    variance = (1.0 - mask) * variance + mask * 1e-12
    return torch.cat([mean.squeeze(0), torch.sqrt(variance).squeeze(0)])


@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_rule_is_torch_autograd(n):
    import torch
    r = np.random.RandomState(50 + n)
    C = 5
    x = r.standard_normal((n, C))
    x[:, 2] = 0.75                                                      # a constant channel: floored
    gp = r.standard_normal(2 * C)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    pooled = torch_pool(xt)
    pooled.backward(torch.tensor(gp))
    m, v, std = rpg.forward(x)
    want = pooled.detach().numpy()
    assert np.max(np.abs(np.concatenate([m, std]) - want)) <= 1e-12 * np.max(np.abs(want))
    gx = rpg.backward(x, m, std, v, gp)
    ref = xt.grad.numpy()
    rel = np.max(np.abs(gx - ref)) / np.max(np.abs(ref))
    print("n = %d: the rule against autograd, relative difference %.2e" % (n, rel))
    assert rel <= 1e-12
    assert np.all(v[2] <= 1e-12) and np.array_equal(gx[:, 2], np.full(n, gp[2] / n))       # floored: gx = a, nothing from std
    if n == 1:
        assert np.all(v == 0) and np.array_equal(gx[0], gp[:C])                             # one frame: every channel is floored


def test_no_frames():
    m, v, std = rpg.forward(np.zeros((0, 3)))
    assert np.all(m == 0) and np.all(v == 0) and np.allclose(std, 1e-6)
    em, ev, es = rpg.emu_forward(np.zeros((0, 3), dtype=np.float32))
    assert np.all(em == 0) and np.all(ev == 0) and np.all(es == np.sqrt(np.float32(1e-12)))


def chain_layers(r, dims, act):
    layers = []
    for k, n in zip(dims[:-1], dims[1:]):
        bn = [r.uniform(0.5, 1.5, n), 0.3 * r.standard_normal(n), 0.1 * r.standard_normal(n), r.uniform(0.5, 1.5, n)]
        layers.append(rs.Layer(r.standard_normal((n, k)) / np.sqrt(k), 0.1 * r.standard_normal(n), bn, act))
    return layers


@pytest.mark.parametrize("act,depth", [(rs.RELU, 2), (rs.LRELU, 3)])
def test_frame_grads_is_autograd_of_the_chain(act, depth):
    import torch
    import torch.nn.functional as fn
    r = np.random.RandomState(3 + depth)
    dims = [6] * depth + [7]
    frame = chain_layers(r, dims, act)
    seg = chain_layers(r, [14, 5, 4], act)
    classes = 3
    hw, hb = r.standard_normal((4, classes)).astype(np.float32), r.standard_normal(classes).astype(np.float32)
    lens = [5, 1, 9, 3]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    frames = np.abs(r.standard_normal((offsets[-1], 6))).astype(np.float32)
    frames[offsets[2]:offsets[3], :] = frames[offsets[2]]               # an utterance of identical frames: every channel floored
    labels = np.array([0, 2, 1, 2], dtype=np.int32)
    res = rpg.frame_grads(frame, seg, hw, hb, frames, offsets, labels)

    leaves = []

    def t(a, grad=True):
        v = torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)
        if grad:
            leaves.append(v)
        return v

    def layer(x, l):
        w, b, g, be = t(l.w), t(l.b), t(l.bn[0]), t(l.bn[1])
        h = fn.batch_norm(fn.linear(x, w, b), t(l.bn[2], False), t(l.bn[3], False), g, be, training=False, eps=1e-3)
        return fn.relu(h) if l.act == rs.RELU else fn.leaky_relu(h, rs.SLOPE)

    x = t(frames, False)
    for l in frame:
        x = layer(x, l)
    pooled = torch.stack([torch_pool(x[offsets[u]:offsets[u + 1]]) for u in range(len(lens))])
    y = layer(layer(pooled, seg[0]), seg[1])
    kw, kb = t(hw), t(hb)
    loss = fn.cross_entropy(y @ kw + kb, torch.tensor(labels, dtype=torch.long))
    loss.backward()
    got = []
    for bwd in res["frame_bwd"] + res["seg_bwd"]:
        got += [bwd["gw"], bwd["gbias"], bwd["ggamma"], bwd["gbeta"]]
    got += [res["head"]["grad_kernel"], res["head"]["grad_bias"]]
    assert len(got) == len(leaves)
    worst = 0.0
    for g, leaf in zip(got, leaves):
        want = leaf.grad.numpy()
        worst = max(worst, float(np.max(np.abs(g - want)) / max(np.max(np.abs(want)), 1e-30)))
    print("frame_grads against autograd of the whole chain: largest relative difference %.2e" % worst)
    assert worst <= 1e-10
    assert abs(float(np.mean(res["head"]["loss"])) - float(loss.detach())) <= 1e-12
    assert np.any(res["pool"]["var"] <= 1e-12) and np.any(res["pool"]["var"] > 1e-12)


@pytest.mark.parametrize("C", pc.CHANNELS)
def test_emulations_stay_inside_the_bars_and_the_bound(C):
    case = pc.make(C)
    again = pc.make(C)
    assert np.array_equal(case["x"][pc.LEAD:], again["x"][pc.LEAD:]) and np.array_equal(case["gp"], again["gp"])      # fixed seeds
    worst = dict(mean=0.0, var=0.0, std=0.0, gx=0.0)
    for u, n in enumerate(pc.LENGTHS):
        x = pc.utterance(case, u)
        assert x.shape == (n, C) and np.all(np.isfinite(x))
        mean, var, std = rpg.emu_forward(x)
        rm, rv, rsd = rpg.forward_ratios(x, mean, var, std)
        gx = rpg.emu_backward(x, mean, std, var, case["gp"][u])
        ref = rpg.backward(x, mean, std, var, case["gp"][u])
        rg_ = np.abs(gx.astype(np.float64) - ref) / rpg.backward_bound(x, mean, std, var, case["gp"][u])
        for k, rat in (("mean", rm), ("var", rv), ("std", rsd), ("gx", rg_)):
            worst[k] = max(worst[k], float(np.max(rat)))
        if case["const"] is not None:
            j = case["const"]
            assert mean[j] == pc.CONST_VALUE and var[j] == 0 and std[j] == np.sqrt(np.float32(1e-12))
            assert np.all(gx[:, j] == np.float32(case["gp"][u, j]) / np.float32(n))         # gx = a bit for bit
    print("C = %d: emulation error / bar " % C + " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def _worst_backward(C, **mutant):
    case = pc.make(C)
    worst = 0.0
    for u, n in enumerate(pc.LENGTHS):
        if n < 2:
            continue
        x = pc.utterance(case, u)
        mean, var, std = rpg.emu_forward(x)
        gx = rpg.emu_backward(x, mean, std, var, case["gp"][u], **mutant)
        with np.errstate(invalid="ignore"):
            rat = np.abs(gx.astype(np.float64) - rpg.backward(x, mean, std, var, case["gp"][u])) / rpg.backward_bound(
                x, mean, std, var, case["gp"][u])
        worst = max(worst, float(np.max(np.where(np.isfinite(rat), rat, np.inf))))
    return worst


@pytest.mark.parametrize("mutant", ["n_minus_1", "no_mask", "drop_a", "flip_b"])
def test_backward_mutants_leave_the_bound(mutant):
    assert _worst_backward(65) <= 1.0
    worst = _worst_backward(65, **{mutant: True})
    print("%s: error / bound %.3g" % (mutant, worst))
    assert worst > 1.0


def test_one_pass_variance_leaves_the_bar():
    case = pc.make(65)
    worst_good, worst_bad = 0.0, 0.0
    for u, n in enumerate(pc.LENGTHS):
        x = pc.utterance(case, u)
        for one_pass in (False, True):
            mean, var, std = rpg.emu_forward(x, one_pass=one_pass)
            _, rv, rsd = rpg.forward_ratios(x, mean, var, std)
            w = float(max(np.max(rv), np.max(rsd)))
            if one_pass:
                worst_bad = max(worst_bad, w)
            else:
                worst_good = max(worst_good, w)
    print("two sweeps: variance error / bar %.3f; E[x^2] - m^2: %.3g" % (worst_good, worst_bad))
    assert worst_good <= 1.0 < worst_bad
