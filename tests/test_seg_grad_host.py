"""Host: the rule of xv_seg_forward / xv_seg_backward (tests/helpers/ref_seg_grad.py) against torch.autograd in float64, the
condition tests/helpers/seg_grad_cases.py puts on the GPU tests' inputs, and the host side of tf_kaldi_speaker_amd/tail_train.py:
variable names, refusals, the l2 assignment."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_loss_grad as rg                                          # noqa: E402
import ref_seg_grad as rs                                           # noqa: E402
import seg_grad_cases as sc                                         # noqa: E402


@pytest.mark.parametrize("has_bn", [False, True])
@pytest.mark.parametrize("act", [rs.NONE, rs.RELU, rs.LRELU])
def test_rule_is_torch_autograd(has_bn, act):
    import torch
    import torch.nn.functional as fn
    r = np.random.RandomState(7 + act + 10 * has_bn)
    n, K, N = 9, 6, 5
    x, w, b, gy = r.standard_normal((n, K)), r.standard_normal((N, K)), r.standard_normal(N), r.standard_normal((n, N))
    bn = [r.uniform(0.5, 1.5, N), r.standard_normal(N), r.standard_normal(N), r.uniform(0.5, 1.5, N)] if has_bn else None
    fwd = rs.forward(x, w, b, bn, act)
    bwd = rs.backward(fwd, gy)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)      # noqa: E731
    xt, wt, bt = t(x), t(w), t(b)
    h = fn.linear(xt, wt, bt)
    z = h
    if has_bn:
        gt, bet = t(bn[0]), t(bn[1])
        h = fn.batch_norm(h, torch.tensor(bn[2]), torch.tensor(bn[3]), gt, bet, training=False, eps=1e-3)
    y = h if act == rs.NONE else (fn.relu(h) if act == rs.RELU else fn.leaky_relu(h, 0.2))
    y.backward(torch.tensor(gy))

    def close(got, want, what):
        want = want.detach().numpy()
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), what

    close(fwd["z"], z, "z")
    close(fwd["y"], y, "y")
    close(bwd["gx"], xt.grad, "gx")
    close(bwd["gw"], wt.grad, "gw")
    close(bwd["gbias"], bt.grad, "gbias")
    if has_bn:
        close(bwd["ggamma"], gt.grad, "ggamma")
        close(bwd["gbeta"], bet.grad, "gbeta")
    else:
        assert bwd["ggamma"] is None and bwd["gbeta"] is None


def test_zero_belongs_to_the_lower_branch():
    fwd = rs.forward(np.zeros((1, 1)), np.ones((1, 1)), np.zeros(1), None, rs.LRELU)
    assert rs.backward(fwd, np.ones((1, 1)))["a"][0, 0] == 0.2
    fwd = rs.forward(np.zeros((1, 1)), np.ones((1, 1)), np.zeros(1), None, rs.RELU)
    assert rs.backward(fwd, np.ones((1, 1)))["a"][0, 0] == 0.0


@pytest.mark.parametrize("name", [c[0] for c in sc.CASES])
def test_no_element_of_a_case_sits_on_the_discontinuity(name):
    c = sc.make(name)
    again = sc.make(name)
    assert all(np.array_equal(c[k], again[k]) for k in ("x", "w", "b", "gy"))       # fixed seeds
    zero, exact, far = sc.precondition(c)
    n, N = c["gy"].shape
    print("%s: %d elements zero by construction, %d of exact sign, %d at least 64 bounds from zero" % (name, zero, exact, far))
    assert zero + exact + far == n * N or c["act"] == rs.NONE
    if c["zero_col"] is not None:
        assert zero == n
    if c["family"] == "dyadic" and c["bn"] is None:
        assert np.any(rs.forward(c["x"], c["w"], c["b"], None, c["act"])["h"] == 0)   # the zero branch is exercised
    # every value of the issue's shape list appears
    assert {k[1] for k in sc.CASES} == {1, 31, 33, 70} and {k[2] for k in sc.CASES} == {1, 35, 100}
    assert {k[3] for k in sc.CASES} == {1, 33, 65, 130}


def test_the_bound_is_far_below_the_values():
    """A bound that is a sizeable fraction of the tensor could hide a failure: its largest element stays below 1e-3 of the
    tensor's largest value for every output of every case (the GPU test caps the error itself at 1e-4 relative L2)."""
    for name in [c[0] for c in sc.CASES]:
        c = sc.make(name)
        fwd = rs.forward(c["x"], c["w"], c["b"], c["bn"], c["act"], rs.SLOPE)
        bwd = rs.backward(fwd, c["gy"], rs.SLOPE)
        bnd = rs.bounds(fwd, bwd)
        ref = dict(fwd, **{k: v for k, v in bwd.items() if v is not None})
        for k, v in bnd.items():
            top = np.max(np.abs(ref[k]))
            if top > 0:
                assert np.max(v) < 1e-3 * top, (name, k, np.max(v) / top)


def test_variable_names_of_the_three_networks():
    from tf_kaldi_speaker_amd import _lib, synth, tail_train
    p = dict(synth.TDNN_STAT_PARAMS)
    a, b = tail_train.segment_variables(p)
    assert a == ("tdnn/tdnn6_dense/kernel", "tdnn/tdnn6_dense/bias", "tdnn/tdnn6_bn", _lib.XV_SEG_ACT_RELU)
    assert b == ("tdnn/tdnn7_dense/kernel", "tdnn/tdnn7_dense/bias", "tdnn/tdnn7_bn", _lib.XV_SEG_ACT_RELU)
    w = synth.synth_weights(dict(p, num_nodes_pooling_layer=8, num_nodes_last_layer=4), 30, seed=0, channels=8)
    assert set(tail_train.trained_names(p)) - {"softmax/output/kernel", "softmax/output/bias"} <= set(w)
    e = dict(p, network_type="extended_tdnn", network_relu_type="lrelu", last_layer_linear=True, last_layer_no_bn=True)
    a, b = tail_train.segment_variables(e)
    assert a == ("etdnn/tdnn12_dense/kernel", "etdnn/tdnn12_dense/bias", "etdnn/tdnn12_bn", _lib.XV_SEG_ACT_LRELU)
    assert b == ("etdnn/tdnn13_dense/kernel", "etdnn/tdnn13_dense/bias", None, _lib.XV_SEG_ACT_NONE)
    w = synth.synth_weights(dict(e, num_nodes_pooling_layer=8, num_nodes_last_layer=4), 30, seed=0, channels=8)
    assert set(tail_train.trained_names(e)) - {"softmax/output/kernel", "softmax/output/bias"} <= set(w)
    assert "etdnn/tdnn13_bn/gamma" not in tail_train.trained_names(e)
    r = dict(synth.RESNET_PARAMS)
    a, b = tail_train.segment_variables(r)
    assert a.kernel == "resnet_18/tdnn6_dense/kernel" and a.bn == "resnet_18/tdnn6_bn"
    assert b.kernel == "resnet_18/tdnn7_dense/kernel" and b.bn == "resnet_18/tdnn7_bn"
    w = synth.synth_resnet_weights(dict(r, num_nodes_pooling_layer=8, num_nodes_last_layer=4), seed=0, width=4)
    assert set(tail_train.trained_names(r)) - {"softmax/output/kernel", "softmax/output/bias"} <= set(w)
    assert tail_train.trained_names(dict(p, loss_func="additive_margin_softmax"))[-1] == "softmax/output/kernel"


def test_refusals():
    from tf_kaldi_speaker_amd import synth, tail_train
    p = dict(synth.TDNN_STAT_PARAMS, optimizer="sgd")
    tail_train.check_supported(p)
    for extra, word in ((dict(network_relu_type="prelu"), "prelu"), (dict(feature_norm=True), "feature_norm"),
                        (dict(loss_func="semihard_triplet_loss"), "softmax family"), (dict(aux_loss_func=["ring_loss"]), "aux_loss_func"),
                        (dict(sample_with_prob=True), "sample_with_prob"), (dict(loss_func="asoftmax", asoftmax_m=3), "m=3")):
        with pytest.raises(NotImplementedError) as info:
            tail_train.check_supported(dict(p, **extra))
        assert word in str(info.value), (extra, str(info.value))
        with pytest.raises(NotImplementedError):                       # the constructor refuses before it touches a device
            tail_train.TailTrainer(dict(p, **extra), {}, 4)
    with pytest.raises(ValueError):
        tail_train.check_supported(dict(p, optimizer="rmsprop"))


def test_l2_goes_on_the_kernels_only():
    from tf_kaldi_speaker_amd import synth, tail_train
    p = dict(synth.TDNN_STAT_PARAMS, optimizer="sgd", weight_l2_regularizer=1e-2)
    l2 = tail_train.l2_assignment(p)
    assert set(l2) == set(tail_train.trained_names(p))
    kernels = {"tdnn/tdnn6_dense/kernel", "tdnn/tdnn7_dense/kernel", "softmax/output/kernel"}
    assert all(l2[k] == (1e-2 if k in kernels else 0.0) for k in l2)
    l2 = tail_train.l2_assignment(dict(p, output_weight_l2_regularizer=5e-3))
    assert l2["softmax/output/kernel"] == 5e-3 and l2["tdnn/tdnn6_dense/kernel"] == 1e-2 and l2["tdnn/tdnn7_dense/kernel"] == 1e-2
    assert l2["tdnn/tdnn6_bn/gamma"] == 0.0 and l2["tdnn/tdnn7_bn/beta"] == 0.0 and l2["tdnn/tdnn6_dense/bias"] == 0.0


def test_update_bound_covers_a_perturbed_gradient():
    """ref_seg_grad.update_bound against two float32 runs of the optimizer rule whose gradients differ by a known amount."""
    r = np.random.RandomState(3)
    w, g = rs.f32(r.standard_normal(200)), r.standard_normal(200)
    dg = 1e-6 * np.abs(r.standard_normal(200))
    s0, s1 = rs.f32(0.1 * r.standard_normal(200)), rs.f32(0.01 * r.uniform(0, 1, 200))
    for kind, nest, clip in ((rg.SGD, False, 0.0), (rg.SGD, False, 3.0), (rg.MOMENTUM, False, 0.0), (rg.MOMENTUM, True, 3.0),
                             (rg.ADAM, False, 0.0)):
        a = rg.opt_step(kind, w, rs.f32(g), s0, s1, lr=0.05, l2=1e-3, clip_norm=clip, momentum=0.9, use_nesterov=nest, step=2)[0]
        b = rg.opt_step(kind, w, rs.f32(g + dg * np.sign(r.standard_normal(200))), s0, s1, lr=0.05, l2=1e-3, clip_norm=clip,
                        momentum=0.9, use_nesterov=nest, step=2)[0]
        bound = rs.update_bound(kind, g, dg + rs.U * np.abs(g), s0, s1, 0.05, clip, 0.9, nest, 2, w, 1e-3)
        assert np.all(np.abs(a.astype(np.float64) - b) <= bound), (kind, nest, clip)
        assert np.max(bound) < 1e-5                                    # and it is no blanket
