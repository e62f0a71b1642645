"""CPU: the rule of xv_bn_batch_forward / xv_bn_batch_backward as tests/helpers/ref_bn_batch.py states it, against
torch.autograd in float64; the condition tests/helpers/bn_batch_cases.py puts on the GPU test's inputs; and the host logic of the
trainers' batch_norm switch (tail_train.batch_stats_options, layer_variables, the refusals)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bn_batch_cases as bc                                         # noqa: E402
import ref_bn_batch as rb                                           # noqa: E402
import ref_tconv as rt                                              # noqa: E402

torch = pytest.importorskip("torch")
F = np.float32
RTOL = 1e-10


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    assert err <= RTOL, "%s: relative error %.3e" % (what, err)


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


def torch_act(h, act):
    if act == rb.RELU:
        return torch.relu(h)
    if act == rb.LRELU:
        return torch.nn.functional.leaky_relu(h, rb.SLOPE)
    return h


# ---------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", bc.NAMES)
def test_every_case_meets_the_precondition(name):
    c = bc.make(name)
    counts = bc.precondition(c)
    assert counts["clear"] + counts["exact_zero"] == c["n"] * c["N"]                 # the cap on skipped elements is zero
    if c["zero_col"] is not None:
        assert counts["exact_zero"] == c["n"]
    assert c["z"].dtype == F and c["gy"].dtype == F
    if c["const_col"] is not None:
        fwd = rb.forward(c["z"], c["gamma"], c["beta"], c["act"])
        assert fwd["v"][c["const_col"]] == 0.0 and fwd["r"][c["const_col"]] == 1.0 / np.sqrt(rb.EPS)
    if c["family"] == "dyadic":
        assert np.all(c["z"] * 8 == np.round(c["z"] * 8)) and c["n"] & (c["n"] - 1) == 0
        mu = c["z"].astype(np.float64).mean(axis=0)
        assert np.all(mu.astype(F).astype(np.float64) == mu)                         # the mean is exact in float32


def test_the_cases_are_deterministic_and_cover_the_table():
    assert {(c[1], c[2], c[3]) for c in bc.CASES if c[4] == "random"} == {(n, N, a) for n in (1, 2, 63, 64, 65, 1025)
                                                                          for N in (1, 31, 33, 68) for a in (0, 1, 2)}
    a, b = bc.make("n65_N33_lrelu"), bc.make("n65_N33_lrelu")
    assert all(np.array_equal(a[k], b[k]) for k in ("z", "gy", "gamma", "beta", "mm", "mv"))
    assert set(bc.LAYOUTS) == {"contiguous", "padded", "offset"}


def test_a_one_sweep_variance_would_fail_the_offset_column():
    """Column 1 (mean 1000, standard deviation 0.01): E[z^2] - mu^2 in float32 is off by more than the bound of v by orders of
    magnitude, the two-sweep rule about the float32-rounded mean is within it."""
    c = bc.make("n1025_N33_relu")
    fwd = rb.forward(c["z"], c["gamma"], c["beta"], c["act"])
    bv = rb.bounds(fwd)["v"][1]
    z = c["z"][:, 1]
    one_sweep = float(np.mean(z * z, dtype=F) - np.mean(z, dtype=F) ** 2)
    mu32 = F(np.mean(z.astype(np.float64)))
    two_sweep = float(F(np.mean((z.astype(np.float64) - float(mu32)) ** 2)))
    assert abs(two_sweep - fwd["v"][1]) <= bv
    assert abs(one_sweep - fwd["v"][1]) > 100.0 * bv


# ---------------------------------------------------------------------------------------------- the rule against torch
@pytest.mark.parametrize("act", bc.ACTS)
@pytest.mark.parametrize("n,N", [(2, 3), (3, 1), (65, 33), (300, 7)])        # torch refuses one row in training mode
def test_rule_equals_torch_autograd(n, N, act):
    r = np.random.RandomState(7 * n + N + act)
    z, gy = r.standard_normal((n, N)) * 2.0 + 0.5, r.standard_normal((n, N))
    gamma, beta = r.standard_normal(N), r.standard_normal(N)
    fwd = rb.forward(z, gamma, beta, act)
    bwd = rb.backward(fwd, gy)
    zt, gt, bt = t64(z, True), t64(gamma, True), t64(beta, True)
    rm, rv = torch.zeros(N, dtype=torch.float64), torch.ones(N, dtype=torch.float64)
    y = torch_act(torch.nn.functional.batch_norm(zt, rm, rv, gt, bt, training=True, momentum=0.1, eps=rb.EPS), act)
    y.backward(t64(gy))
    close(fwd["y"], y.detach().numpy(), "y")
    close(bwd["gz"], zt.grad.numpy(), "gz")
    close(bwd["ggamma"], gt.grad.numpy(), "ggamma")
    close(bwd["gbeta"], bt.grad.numpy(), "gbeta")
    assert all(np.all(np.isfinite(v)) for v in (fwd["y"], bwd["gz"], bwd["ggamma"], bwd["gbeta"]))


@pytest.mark.parametrize("act", (rb.RELU, rb.LRELU))
def test_conv_stack_equals_torch_autograd(act):
    """conv1d -> batch norm -> activation -> conv1d -> batch norm on packed utterances, composed as the trainers compose it:
    ref_tconv without batch norm and with no activation for z, the new rule on z, and backwards ref_tconv's pass-through of gz
    (gbias = sum_i gz_ij, gw, gx)."""
    r = np.random.RandomState(11 + act)
    lengths, C, N1, N2, W1, W2 = [9, 12, 7], 4, 6, 5, 3, 2
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    x = r.standard_normal((int(off[-1]), C))
    w1, b1 = r.standard_normal((N1, W1 * C)) / 3.0, r.standard_normal(N1)
    w2, b2 = r.standard_normal((N2, W2 * N1)) / 3.0, r.standard_normal(N2)
    g1, be1, g2, be2 = (r.standard_normal(k) for k in (N1, N1, N2, N2))
    f1 = rt.forward(x, off, W1, w1, b1, None, rt.NONE)
    n1 = rb.forward(f1["z"], g1, be1, act)
    off1 = rt.out_offsets(off, W1)
    f2 = rt.forward(n1["y"], off1, W2, w2, b2, None, rt.NONE)
    n2 = rb.forward(f2["z"], g2, be2, rb.NONE)
    G = r.standard_normal(n2["y"].shape)
    m2 = rb.backward(n2, G)
    t2 = rt.backward(f2, m2["gz"])
    m1 = rb.backward(n1, t2["gx"])
    t1 = rt.backward(f1, m1["gz"])

    P = [t64(v, True) for v in (x, w1, b1, g1, be1, w2, b2, g2, be2)]
    xt, w1t, b1t, g1t, be1t, w2t, b2t, g2t, be2t = P

    def conv(inp, offsets, w, b, taps):                              # rows [N, taps C] with k = tau C + c -> conv1d weight [N, C, taps]
        cin = inp.shape[1]
        k = w.reshape(w.shape[0], taps, cin).permute(0, 2, 1)
        outs = [torch.nn.functional.conv1d(inp[offsets[u]:offsets[u + 1]].t()[None], k, b)[0].t() for u in range(len(offsets) - 1)]
        return torch.cat(outs, dim=0)

    def bn(v, g, b):
        return torch.nn.functional.batch_norm(v, None, None, g, b, training=True, eps=rb.EPS)

    y1 = torch_act(bn(conv(xt, off, w1t, b1t, W1), g1t, be1t), act)
    y2 = bn(conv(y1, off1, w2t, b2t, W2), g2t, be2t)
    (y2 * t64(G)).sum().backward()
    close(n2["y"], y2.detach().numpy(), "y")
    for got, want, what in ((t1["gx"], xt, "gx"), (t1["gw"], w1t, "gw1"), (t1["gbias"], b1t, "gbias1"), (m1["ggamma"], g1t, "ggamma1"),
                            (m1["gbeta"], be1t, "gbeta1"), (t2["gw"], w2t, "gw2"), (t2["gbias"], b2t, "gbias2"),
                            (m2["ggamma"], g2t, "ggamma2"), (m2["gbeta"], be2t, "gbeta2")):
        if what.startswith("gbias"):                                 # the exact gradient is zero: batch norm removes the mean
            assert np.abs(got).max() <= 1e-10 * np.abs(G).sum() and np.abs(want.grad.numpy()).max() <= 1e-10 * np.abs(G).sum(), what
        else:
            close(got, want.grad.numpy(), what)


# ---------------------------------------------------------------------------------------------- the moving update
@pytest.mark.parametrize("bessel", (True, False))
@pytest.mark.parametrize("n", (2, 65, 300))
def test_moving_update_equals_torch_running_statistics(n, bessel):
    r = np.random.RandomState(n)
    N, momentum = 9, 0.99
    z = (r.standard_normal((n, N)) * 1.5 + 0.3).astype(F)
    mm, mv = r.standard_normal(N).astype(F), (0.5 + r.rand(N)).astype(F)
    fwd = rb.forward(z, np.ones(N), np.zeros(N))
    got_m, got_v = rb.moving_f32(mm, mv, fwd["mu"].astype(F), fwd["v"].astype(F), n, momentum, bessel)
    rm, rv = torch.tensor(mm.copy()), torch.tensor(mv.copy())
    torch.nn.functional.batch_norm(torch.tensor(z), rm, rv, None, None, training=True, momentum=1.0 - momentum, eps=rb.EPS)
    want_m = rm.numpy().astype(np.float64)
    want_v = rv.numpy().astype(np.float64)                           # torch feeds the Bessel-corrected variance
    if not bessel:                                                   # the same update fed the biased variance
        want_v = mv.astype(np.float64) * momentum + fwd["v"] * (1.0 - momentum)
    tol = 8 * rb.U                                                   # a few float32 roundings on each side
    assert np.all(np.abs(got_m - want_m) <= tol * np.maximum(np.abs(want_m), np.abs(mm)))
    assert np.all(np.abs(got_v - want_v) <= tol * np.maximum(np.abs(want_v), np.abs(mv)))
    m64, v64, _ = rb.moving(mm, mv, fwd["mu"], fwd["v"], n, momentum, bessel)
    b = rb.bounds(fwd, mm=mm, mv=mv, momentum=momentum, bessel=bessel)
    assert np.all(np.abs(got_m - m64) <= b["moving_mean"]) and np.all(np.abs(got_v - v64) <= b["moving_variance"])


def test_one_row_is_finite():
    N = 4
    z = np.array([[0.5, -1.0, 2.0, 0.0]])
    fwd = rb.forward(z, np.ones(N), np.full(N, 0.25), rb.LRELU)
    bwd = rb.backward(fwd, np.ones((1, N)))
    assert rb.bessel_factor(1) == 1.0 and rb.bessel_factor(2) == 2.0
    assert np.all(fwd["v"] == 0.0) and np.all(fwd["y"] == 0.25) and np.all(bwd["gz"] == 0.0)
    m, v, vb = rb.moving(np.zeros(N), np.ones(N), fwd["mu"], fwd["v"], 1, 0.99, True)
    m32, v32 = rb.moving_f32(np.zeros(N), np.ones(N), fwd["mu"], fwd["v"], 1, 0.99, True)
    for a in (m, v, vb, m32, v32, bwd["ggamma"], bwd["gbeta"]) + tuple(rb.bounds(fwd, bwd, mm=np.zeros(N), mv=np.ones(N)).values()):
        assert np.all(np.isfinite(a))


# ---------------------------------------------------------------------------------------------- host logic of the trainers
def _params(network_type, **extra):
    d = dict(network_type=network_type, loss_func="softmax", optimizer="momentum", momentum=0.9, use_nesterov=False,
             weight_l2_regularizer=1e-2, network_relu_type="relu")
    d.update(extra)
    return d


def test_bessel_follows_the_rank_of_the_layers_own_kernel():
    from tf_kaldi_speaker_amd import tail_train
    p = _params("tdnn", batchnorm_momentum=0.95)
    opt = tail_train.batch_stats_options
    assert opt(p, "moving") == {} and opt(p, "moving", np.zeros((1, 5, 3, 4))) == {}
    # tdnn: conv2d kernels [1, W, C, N] -> the batch norm sees [b, 1, l, N], the fused kernel, Bessel
    assert opt(p, "batch", np.zeros((1, 5, 3, 4))) == dict(batch_stats=True, momentum=0.95, bessel=True)
    # its dense frame layers come behind tf.squeeze (model/tdnn.py:94): rank 3, no Bessel; so do conv1d kernels and segment layers
    assert opt(p, "batch", np.zeros((3, 4)))["bessel"] is False
    assert opt(p, "batch", np.zeros((5, 3, 4)))["bessel"] is False
    assert opt(p, "batch")["bessel"] is False
    assert opt(_params("extended_tdnn"), "batch", np.zeros((5, 3, 4))) == dict(batch_stats=True, momentum=0.99, bessel=False)
    with pytest.raises(ValueError):
        opt(p, "renorm")


def test_variables_hold_the_moving_statistics_of_batch_layers_only():
    from tf_kaldi_speaker_amd import tail_train

    class Vec(object):
        def __init__(self, v):
            self.v = np.full(3, v, dtype=F)

        def cpu(self):
            return self

        def numpy(self):
            return self.v

    class FakeLayer(object):
        def __init__(self, batch_stats, bn=True):
            self.batch_stats, self.b = batch_stats, Vec(0)
            self.bn = [Vec(1), Vec(2), Vec(3), Vec(4)] if bn else None

        def kernel(self):
            return np.zeros((2, 3), dtype=F)

    specs = (tail_train.SegSpec("s/a/kernel", "s/a/bias", "s/a_bn", 1), tail_train.SegSpec("s/b/kernel", "s/b/bias", None, 0))
    moving = tail_train.layer_variables(specs, [FakeLayer(False), FakeLayer(False, bn=False)])
    assert list(moving) == ["s/a/kernel", "s/a/bias", "s/a_bn/gamma", "s/a_bn/beta", "s/b/kernel", "s/b/bias"]
    batch = tail_train.layer_variables(specs, [FakeLayer(True), FakeLayer(False, bn=False)])
    assert list(batch) == ["s/a/kernel", "s/a/bias", "s/a_bn/gamma", "s/a_bn/beta", "s/a_bn/moving_mean", "s/a_bn/moving_variance",
                           "s/b/kernel", "s/b/bias"]
    assert batch["s/a_bn/moving_mean"][0] == 3 and batch["s/a_bn/moving_variance"][0] == 4


def test_trained_names_and_l2_do_not_know_the_mode():
    """The moving statistics are no optimizer tensors: the names and l2 factors are functions of params alone, as before."""
    import inspect
    from tf_kaldi_speaker_amd import conv_train, frame_train, tail_train
    p = _params("tdnn")
    for mod in (tail_train, frame_train, conv_train):
        assert list(inspect.signature(mod.trained_names).parameters) == ["params"]
        assert list(inspect.signature(mod.l2_assignment).parameters) == ["params"]
        names = mod.trained_names(p)
        assert not [n for n in names if "moving" in n] and set(mod.l2_assignment(p)) == set(names)
    assert tail_train.trained_names(p) == ["tdnn/tdnn6_dense/kernel", "tdnn/tdnn6_dense/bias", "tdnn/tdnn6_bn/gamma", "tdnn/tdnn6_bn/beta",
                                           "tdnn/tdnn7_dense/kernel", "tdnn/tdnn7_dense/bias", "tdnn/tdnn7_bn/gamma", "tdnn/tdnn7_bn/beta",
                                           "softmax/output/kernel", "softmax/output/bias"]
    for cls in (tail_train.TailTrainer, frame_train.StackedTrainer, conv_train.ConvTrainer):
        assert inspect.signature(cls.__init__).parameters["batch_norm"].default == "moving"
    assert inspect.signature(tail_train.Layer.__init__).parameters["batch_stats"].default is False


def test_batch_norm_batch_alone_is_refused(capsys):
    from tf_kaldi_speaker_amd import head_train, train_head
    with pytest.raises(ValueError, match="the head has no batch norm"):
        head_train.train_head(None, "train", "spk", "valid", "spk", "out", weights={}, batch_norm="batch")
    with pytest.raises(ValueError):
        head_train.train_head(None, "train", "spk", "valid", "spk", "out", weights={}, segment_layers=True, batch_norm="renorm")
    with pytest.raises(SystemExit) as e:
        train_head.main(["--batch-norm", "batch", "pre", "train", "spk", "valid", "spk", "out"])
    assert e.value.code == 2 and "the head has no batch norm" in capsys.readouterr().err
    args = train_head.build_parser().parse_args(["pre", "train", "spk", "valid", "spk", "out"])
    assert args.batch_norm == "moving"
    assert inspect_default(head_train.train_head, "batch_norm") == "moving"


def test_the_operator_is_built_declared_and_bound(repo_root):
    import __graft_entry__ as g
    assert "bn_batch.hip" in g.SOURCES and os.path.isfile(os.path.join(g.CSRC, "bn_batch.hip"))
    header = open(os.path.join(repo_root, "include", "xvec_hip.h")).read()
    assert "**Parity unpinned**" in header and "bessel" in header
    source = open(os.path.join(g.CSRC, "bn_batch.hip")).read()
    assert "atomic" not in source.replace("no floating-point atomics", "") and '#include "layer_lines.h"' in source


def inspect_default(fn, name):
    import inspect
    return inspect.signature(fn).parameters[name].default
