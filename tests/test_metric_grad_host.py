"""The gradient rule of the triplet heads (include/xvec_hip.h, xv_metric_loss_grad) without a GPU: the numpy oracle
tests/helpers/ref_metric_grad.py against torch.autograd in float64 on a dense restatement of the three losses written from the
rule; the rule's choices on ties and degenerate rows; the refusals of the C ABI on the built library (none reaches a HIP call);
and the Python surface."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_metric_grad as rg                                        # noqa: E402
import ref_metric_loss as rm                                        # noqa: E402

from tf_kaldi_speaker_amd import metric_losses as ml                # noqa: E402
from tf_kaldi_speaker_amd.params import Params                      # noqa: E402

ARC = "additive_angular_margin_softmax"
AM = "additive_margin_softmax"
CASES = [("semihard", dict(margin=0.2, squared=False, normalize=True)),
         ("semihard", dict(margin=0.2, squared=True, normalize=True)),
         ("semihard", dict(margin=1.5, squared=False, normalize=False)),
         ("semihard", dict(margin=6.0, squared=True, normalize=False)),
         ("all", dict(loss_type="asoftmax", margin=1)),
         ("all", dict(loss_type="asoftmax", margin=2)),
         ("all", dict(loss_type="asoftmax", margin=4)),
         ("all", dict(loss_type=AM, margin=0.2)),
         ("all", dict(loss_type=ARC, margin=0.3)),
         ("hard", dict(loss_type="asoftmax", margin=1)),
         ("hard", dict(loss_type="asoftmax", margin=2)),
         ("hard", dict(loss_type="asoftmax", margin=4)),
         ("hard", dict(loss_type=AM, margin=0.2)),
         ("hard", dict(loss_type=ARC, margin=0.3))]


def rows_and_labels(seed, b, d, classes):
    rs = np.random.RandomState(seed)
    cls = np.concatenate([np.arange(classes), rs.randint(0, classes, b - classes)])
    rs.shuffle(cls)
    x = rs.standard_normal((classes, d))[cls] * 0.8 + rs.standard_normal((b, d))
    return x.astype(np.float32), (cls * 7 - 3).astype(np.int32)


def torch_pos(c, head, margin):
    if head == "asoftmax":
        if margin == 1:
            return c
        s0 = torch.sign(c).detach()
        if margin == 2:
            return 2.0 * s0 * c * c - 1.0
        s3 = (torch.sign(2.0 * c * c - 1.0) * s0).detach()
        return s3 * (8.0 * c ** 4 - 8.0 * c * c + 1.0) + (2.0 * s0 + s3 - 3.0)
    if head == AM:
        return c - margin
    t = c * np.cos(margin) - torch.sqrt(1.0 - c * c) * np.sin(margin)
    return torch.where(c <= np.cos(np.pi - margin), -t - 2.0, t)


def torch_loss(kind, x, labels, **o):
    """torch_loss_of on numpy rows -> (loss, its gradient by autograd)."""
    x = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    loss = torch_loss_of(kind, x, labels, **o)
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def torch_loss_of(kind, x, labels, **o):
    """The three losses, dense ([B, B, B] where the rule ranges over triplets), on a torch float64 tensor -> the loss tensor."""
    lab = torch.as_tensor(np.asarray(labels, dtype=np.int64))
    B = x.shape[0]
    eye = torch.eye(B, dtype=torch.bool)
    same = lab[:, None] == lab[None, :]
    pos, neg = same & ~eye, ~same
    normalize = True if kind != "semihard" else o.get("normalize", True)
    v = x / torch.sqrt(torch.clamp((x * x).sum(dim=1, keepdim=True), min=1e-12)) if normalize else x
    G = v @ v.T
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    if kind == "semihard":
        n = (v * v).sum(dim=1)
        d2 = torch.clamp(n[:, None] - 2.0 * G + n[None, :], min=0.0)
        dist = d2 if o.get("squared", False) else torch.sqrt(torch.where(eye, torch.ones_like(d2), d2))
        dist = torch.where(eye, torch.zeros_like(dist), dist)
        dik = dist[:, None, :].expand(B, B, B)                       # [i, j, k] = d(i, k)
        ok = neg[:, None, :] & (dik > dist[:, :, None])
        least = torch.where(ok, dik, inf).min(dim=2).values
        largest = torch.where(neg[:, None, :], dik, -inf).max(dim=2).values
        z = torch.where(torch.isfinite(least), least, largest)
        use = pos & neg.any(dim=1)[:, None]
        terms = torch.relu(o.get("margin", 0.2) + dist - torch.where(use, z, torch.zeros_like(z)))
        loss = torch.where(use, terms, torch.zeros_like(terms)).sum() / max(float(use.sum()), 1e-16)
    else:
        head, margin = o["loss_type"], o["margin"]
        c = torch.clamp(G, -1.0, 1.0)
        # the pair (i, i) is the constant c(i, i); off the diagonal pos is differentiated
        pv = torch.where(eye, torch_pos(c.detach(), head, margin), torch_pos(torch.where(eye, torch.full_like(c, 0.5), c), head, margin))
        if kind == "all":
            t = c[:, None, :] - pv[:, :, None]                       # [i, j, k]
            use = pos[:, :, None] & neg[:, None, :]
            active = float((use & (t > 1e-12)).sum())
            loss = torch.where(use, torch.relu(t), torch.zeros_like(t)).sum() / (active + 1e-16)
        else:
            hp = torch.where(same, pv, inf).min(dim=1).values
            hn = torch.where(neg, c, -inf).max(dim=1).values
            has = neg.any(dim=1)
            rows = torch.relu(torch.where(has, hn, torch.zeros_like(hn)) - torch.where(has, hp, torch.zeros_like(hp)))
            loss = torch.where(has, rows, torch.zeros_like(rows)).sum() / B
    return loss


@pytest.mark.parametrize("b,classes,seed", [(24, 5, 1), (32, 6, 2)])
@pytest.mark.parametrize("kind,o", CASES, ids=["%s-%s" % (k, "-".join(str(v) for v in o.values())) for k, o in CASES])
def test_oracle_agrees_with_autograd(kind, o, b, classes, seed):
    x, labels = rows_and_labels(seed, b, 16, classes)
    out = rg.grad(kind, x, labels, **o)
    m = rg.margins(out)
    assert min(m.values()) > 1e-9, "the inputs hold a near-tie: %s" % (m,)
    want_loss, want = torch_loss(kind, np.asarray(x, dtype=np.float64), labels, **o)
    assert out["res"]["loss"] == rm.evaluate(kind, x, labels, **o)["loss"]
    assert abs(out["res"]["loss"] - want_loss) <= 1e-12 * max(1.0, abs(want_loss))
    scale = np.abs(want).max()
    err = np.abs(out["grad"] - want).max()
    print("%s %s B=%d: max |oracle - autograd| / max |g| = %.3g (max |g| %.3g)" % (kind, o, b, err / scale, scale))
    assert scale > 0 and np.all(np.isfinite(out["grad"]))
    assert err <= 1e-10 * scale
    # grad_scale is a plain factor
    np.testing.assert_allclose(rg.grad(kind, x, labels, grad_scale=0.5, **o)["grad"], 0.5 * out["grad"], rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------ the rule's choices
def degenerate_cases():
    """(name, kind, options, x, labels): the ties and degenerate rows the rule fixes a choice for."""
    rs = np.random.RandomState(5)
    x, labels = rows_and_labels(11, 12, 8, 3)
    cases = []
    dup = x.copy()
    j = np.nonzero(labels == labels[0])[0][1]
    dup[j] = dup[0]                                                   # two bitwise-equal rows of one class: D2 == 0
    cases.append(("duplicate_rows", "semihard", dict(margin=0.2, squared=False, normalize=True), dup, labels))
    cases.append(("duplicate_rows_sq", "semihard", dict(margin=0.2, squared=True, normalize=False), dup, labels))
    tie = x.copy()
    k = np.nonzero(labels != labels[0])[0][:2]
    tie[k[1]] = tie[k[0]]                                             # two negatives at the same distance: the lowest column
    cases.append(("equal_negatives", "semihard", dict(margin=0.2, squared=False, normalize=True), tie, labels))
    cases.append(("equal_negatives_hard", "hard", dict(loss_type=AM, margin=0.2), tie, labels))
    zero = x.copy()
    zero[3] = 0.0                                                     # sum x^2 <= 1e-12
    cases.append(("zero_row", "semihard", dict(margin=0.2, squared=False, normalize=True), zero, labels))
    cases.append(("zero_row_all", "all", dict(loss_type="asoftmax", margin=2), zero, labels))
    cases.append(("zero_row_hard", "hard", dict(loss_type=AM, margin=0.2), zero, labels))
    lone = labels.copy()
    lone[5] = 1 << 20                                                 # a class of one row: hp is the pair (i, i)
    near = x.copy()
    near[5] = near[6] + 0.05 * near[7]                                # ... and a negative inside the margin, so the row is active
    cases.append(("one_row_class", "hard", dict(loss_type=ARC, margin=0.3), near, lone))
    par = x.copy()
    far = np.nonzero(labels != labels[0])[0][0]
    par[[0, j, far]] = 0.0                                            # one component, powers of two: u = +-e_1 and |c| = 1 exactly
    par[0, 0], par[j, 0], par[far, 0] = 2.0, 4.0, -8.0
    cases.append(("unit_cosine", "all", dict(loss_type=ARC, margin=0.3), par, labels))
    cases.append(("unit_cosine_hard", "hard", dict(loss_type="asoftmax", margin=4), par, labels))
    cases.append(("no_negative", "semihard", dict(margin=0.2, squared=False, normalize=True), x, np.full(12, 4, np.int32)))
    cases.append(("no_negative_all", "all", dict(loss_type=AM, margin=0.2), x, np.full(12, 4, np.int32)))
    cases.append(("no_negative_hard", "hard", dict(loss_type=ARC, margin=0.3), x, np.full(12, 4, np.int32)))
    del rs
    return cases


@pytest.mark.parametrize("case", degenerate_cases(), ids=lambda c: c[0])
def test_rule_cases_are_finite_and_as_stated(case):
    name, kind, o, x, labels = case
    out = rg.grad(kind, x, labels, **o)
    g, W = out["grad"], out["W"]
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(W))
    if name.startswith("duplicate_rows"):
        j = np.nonzero(labels == labels[0])[0][1]
        assert out["res"]["dist"][0, j] == 0.0 and W[0, j] == 0.0 and W[j, 0] == 0.0          # no gradient through D2 == 0
    if name == "equal_negatives":
        k = np.nonzero(labels != labels[0])[0][:2]
        assert out["res"]["dist"][0, k[0]] == out["res"]["dist"][0, k[1]]
        assert W[0, k[1]] == 0.0 or W[0, k[0]] != 0.0                                        # never the higher column alone
        assert np.all((W[:, k[1]] == 0.0) | (labels == labels[k[1]]) | (W[:, k[0]] != 0.0))
    if name == "equal_negatives_hard":
        k = np.nonzero(labels != labels[0])[0][:2]
        rows = np.nonzero(labels != labels[k[0]])[0]
        assert np.all(W[rows, k[1]] == 0.0)                                                  # hn never takes the higher of the twins
    if name.startswith("zero_row"):
        assert out["s"][3] == 1e6
    if name == "one_row_class":
        assert np.count_nonzero(W[5]) == 1 and W[5, 5] == 0.0                                # the negative alone: (i, i) is a constant
    if name.startswith("unit_cosine"):
        c = out["res"]["cos"]
        off = ~np.eye(12, dtype=bool)
        assert (np.abs(c[off]) == 1.0).any() and np.all(W[np.abs(c) == 1.0] == 0.0)
    if name.startswith("no_negative"):
        assert not g.any() and out["res"]["loss"] == 0.0


# ------------------------------------------------------------------------------------------------ the C ABI, no device needed
def test_abi_workspace_and_refusals(repo_root):
    import __graft_entry__ as g
    from tf_kaldi_speaker_amd import _lib
    assert "metric_loss_grad.hip" in g.SOURCES and os.path.isfile(os.path.join(g.CSRC, "metric_loss_grad.hip"))
    g.build()
    lib = _lib.load()
    off = np.array([0, 640, 1280], dtype=np.int64)
    ptr = off.ctypes.data_as(ctypes.c_void_p)
    r256 = lambda v: (v + 255) // 256 * 256                          # noqa: E731
    # tables (3 offsets, 160 panels of 8 anchors), three doubles per row, one slot: dL/dM [B, B] and its product [B, d]
    want = r256(8 * 3) + r256(8 * 160) + 3 * r256(8 * 1280) + r256(8 * 640 * (640 + 512))
    for kind in (0, 1, 2):
        assert lib.xv_metric_loss_grad_workspace(2, ptr, 512, kind) == want
    assert lib.xv_metric_loss_grad_workspace(0, None, 512, 0) == 0
    for kind in (3, 4):
        assert lib.xv_metric_loss_grad_workspace(2, ptr, 512, kind) == _lib.XV_ERR_UNSUPPORTED
    for args in ((2, ptr, 0, 0), (2, ptr, 4097, 0), (2, ptr, 512, 5), (2, ptr, 512, -1), (-1, ptr, 512, 0)):
        assert lib.xv_metric_loss_grad_workspace(*args) == _lib.XV_ERR_INVALID, args
    big = np.array([0, 1025], dtype=np.int64)
    assert lib.xv_metric_loss_grad_workspace(1, big.ctypes.data_as(ctypes.c_void_p), 8, 0) == _lib.XV_ERR_UNSUPPORTED
    full = np.array([0, 1024], dtype=np.int64)
    assert lib.xv_metric_loss_grad_workspace(1, full.ctypes.data_as(ctypes.c_void_p), 8, 0) > 0

    # the call itself: host buffers stand in for device memory, since every refusal comes before the first HIP call
    n, d = 6, 4
    x = np.zeros((n, d), np.float32)
    lab = np.zeros(n, np.int32)
    outs = [np.full(n, -7.0), np.full(n, -7, np.int64), np.full(1, -7.0), np.full(2, -7, np.int64), np.full((n, d), -7.0, np.float32)]
    ws = np.full(1 << 16, 0x5A, np.uint8)
    one = np.array([0, n], dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                 # noqa: E731

    def call(offsets=one, groups=1, dd=d, kind=0, head=0, margin=0.2, scale=1.0, ldx=d, ldg=d, ws_bytes=ws.size, x_=x, gx=outs[4]):
        return lib.xv_metric_loss_grad(0, None if x_ is None else p(x_), ldx, p(offsets), groups, dd, p(lab), kind, head, margin, 0, 1,
                                       scale, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None if gx is None else p(gx), ldg,
                                       p(ws), ws_bytes, None)

    U, I, Wk = _lib.XV_ERR_UNSUPPORTED, _lib.XV_ERR_INVALID, _lib.XV_ERR_WORKSPACE
    assert call(kind=3) == U and call(kind=4) == U and call(kind=5) == I and call(kind=-1) == I
    assert call(offsets=big, groups=1) == U
    assert call(ldg=d - 1) == I and call(ldx=d - 1) == I
    assert call(scale=float("inf")) == I and call(scale=float("nan")) == I and call(margin=float("nan")) == I
    assert call(kind=1, head=0) == I and call(kind=2, head=4) == I and call(kind=1, head=1, margin=3.0) == U
    assert call(x_=None) == I and call(gx=None) == I and call(dd=0) == I
    assert call(ws_bytes=64) == Wk
    assert call(groups=0) == 0
    assert all(np.all(o == -7) for o in outs) and np.all(ws == 0x5A)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_metric_head_takes_the_training_options():
    h = ml.MetricHead(Params(loss_func="semihard_triplet_loss", margin=0.35, triplet_loss_squared=True))
    assert (h.kind, h.margin, h.squared, h.normalize, h.pos_head) == (0, 0.35, True, True, 0)
    h = ml.MetricHead(Params(loss_func="angular_triplet_loss", margin=0.2, triplet_type="hard", loss_type=AM))
    assert (h.kind, h.pos_head, h.margin) == (2, 2, 0.2)
    h = ml.MetricHead(Params(loss_func="angular_triplet_loss", margin=4, triplet_type="all", loss_type="asoftmax"))
    assert (h.kind, h.pos_head, h.margin) == (1, 1, 4.0)
    with pytest.raises(NotImplementedError, match="m=3 is not unsupported"):
        ml.MetricHead(Params(loss_func="angular_triplet_loss", margin=3, triplet_type="all", loss_type="asoftmax"))
    for func in ("generalized_angular_triplet_loss", "ge2e", "softmax", "asoftmax", "nonsense"):
        with pytest.raises(NotImplementedError):
            ml.MetricHead(Params(loss_func=func))
    x = np.zeros((6, 4), np.float32)
    labels = np.array([0, 0, 1, 1, 2, 2])
    h = ml.MetricHead(Params(loss_func="semihard_triplet_loss", margin=0.2, triplet_loss_squared=False))
    with pytest.raises(ValueError, match="at most 1024"):
        h.loss_and_grad(np.zeros((1025, 2), np.float32), np.arange(1025))
    with pytest.raises(ValueError, match="grad_scale"):
        h.loss_and_grad(x, labels, grad_scale=float("nan"))
    with pytest.raises(ValueError, match="labels"):
        h.loss_and_grad(x, labels[:5])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            h.loss_and_grad(x, labels)


def test_the_metric_door_of_the_trainers():
    from tf_kaldi_speaker_amd import att_train, conv_train, frame_train, synth, tail_train
    semi = dict(synth.TDNN_STAT_PARAMS, loss_func="semihard_triplet_loss", margin=0.2, triplet_loss_squared=False)
    ang = dict(synth.TDNN_STAT_PARAMS, loss_func="angular_triplet_loss", margin=0.2, triplet_type="all", loss_type=AM)
    for module in (tail_train, frame_train, conv_train):
        for p in (semi, ang):
            module.check_supported(Params(**p), metric=True)
            with pytest.raises(NotImplementedError, match="softmax family"):           # the default door, in today's words
                module.check_supported(Params(**p))
            names = module.metric_trained_names(Params(**p))
            assert names and not any(n.startswith("softmax/") for n in names)
            assert names + ["softmax/output/kernel"] == module.trained_names(Params(**p))
            l2 = module.metric_l2_assignment(Params(**p))
            assert set(l2) == set(names)
        with pytest.raises(NotImplementedError, match="metric door"):
            module.check_supported(Params(**synth.TDNN_STAT_PARAMS), metric=True)
        for bad in (dict(feature_norm=True), dict(network_relu_type="prelu"), dict(aux_loss_func=["ring_loss"]),
                    dict(sample_with_prob=True), dict(loss_func="generalized_angular_triplet_loss"), dict(loss_func="ge2e")):
            with pytest.raises(NotImplementedError):
                module.check_supported(Params(**dict(semi, **bad)), metric=True)
        with pytest.raises(NotImplementedError, match="m=3 is not unsupported"):
            module.check_supported(Params(**dict(ang, loss_type="asoftmax", margin=3)), metric=True)
    import test_gpu_att_train as att_cases                                  # its models are plain dictionaries
    net, keys = att_cases.MODELS["front-h1"]
    p = dict(synth.TDNN_STAT_PARAMS, network_type=net, **dict(att_cases.EXTRA, **dict(keys, **{k: ang[k] for k in ("loss_func", "margin", "triplet_type", "loss_type")})))
    for conv in (False, True):
        att_train.check_supported(Params(**p), conv, metric=True)
        with pytest.raises(NotImplementedError, match="softmax family"):
            att_train.check_supported(Params(**p), conv)
        names = att_train.trained_names(Params(**p), conv, metric=True)
        assert not any(n.startswith("softmax/") for n in names) and set(att_train.l2_assignment(Params(**p), conv, metric=True)) == set(names)
    with pytest.raises(NotImplementedError, match="softmax family"):
        tail_train.TailTrainer(Params(**semi), {}, 3)
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, KeyError)):
            tail_train.TailTrainer(Params(**semi), {}, 3, metric=True)


def test_train_head_refuses_what_the_triplet_losses_cannot_train(tmp_path):
    import types
    from tf_kaldi_speaker_amd import head_train, synth, train_head
    base = dict(synth.TDNN_STAT_PARAMS, loss_func="angular_triplet_loss", margin=0.2, triplet_type="all", loss_type=AM,
                num_speakers_per_batch=4, num_segments_per_speaker=2)
    stub = lambda **kw: types.SimpleNamespace(params=Params(**dict(base, **kw)))        # noqa: E731
    with pytest.raises(ValueError, match="there is no head to train"):
        head_train.train_head(stub(), "t", "ts", "v", "vs", str(tmp_path))
    with pytest.raises(ValueError, match="num_segments_per_speaker >= 2"):
        head_train.train_head(stub(num_segments_per_speaker=1), "t", "ts", "v", "vs", str(tmp_path), segment_layers=True)
    with pytest.raises(ValueError, match="num_speakers_per_batch >= 2"):
        head_train.train_head(stub(num_speakers_per_batch=1), "t", "ts", "v", "vs", str(tmp_path), conv_layers=True)
    # the command says the same before it loads anything
    import json
    nnet = tmp_path / "pre" / "nnet"
    nnet.mkdir(parents=True)
    (nnet / "config.json").write_text(json.dumps(base))
    (nnet / "feature_dim").write_text("30\n")
    with pytest.raises(SystemExit):
        train_head.main([str(tmp_path / "pre"), "t", "ts", "v", "vs", str(tmp_path / "out")])
