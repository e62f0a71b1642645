"""Host: the gradient rule of xv_loss_classifier_grad (tests/helpers/ref_loss_grad.py) against torch.autograd in float64 on a
torch transcription of ref_loss.classifier_loss; the optimizer oracle against closed forms; the inputs of the GPU test against
the gate the issue puts on them; plan_train_batches, the learning-rate rule, HeadTrainer's refusals and the initialisation."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import loss_grad_cases as lc                                        # noqa: E402
import ref_loss                                                     # noqa: E402
import ref_loss_grad as rg                                          # noqa: E402
from valid_data import make_data_dir                                # noqa: E402


def torch_loss(x, labels, w, b, head, margin, fa):
    """ref_loss.classifier_loss line by line in torch float64 -> (loss [n], lse [n], target [n])."""
    import torch
    n = x.shape[0]
    rows = torch.arange(n)
    lab = torch.as_tensor(labels, dtype=torch.long)
    if head == "softmax":
        z = x @ w
        if b is not None:
            z = z + b[None, :]
        upd = z
    else:
        wh = w / torch.sqrt(torch.clamp(torch.sum(w * w, dim=0, keepdim=True), min=1e-12))        # tf.nn.l2_normalize
        z = x @ wh
        upd = z
        if not (head == "asoftmax" and int(margin) == 1):
            sel = z[rows, lab]
            fn = torch.clamp(torch.sqrt(torch.sum(x * x, dim=1)), min=1e-12)                      # tf.maximum(tf.norm, eps)
            c = torch.clamp(sel / fn, -1.0 + 1e-12, 1.0 - 1e-12)                                  # tf.clip_by_value
            if head == "asoftmax":
                s0 = torch.sign(c).detach()
                c2 = c * c
                if int(margin) == 2:
                    p = 2.0 * s0 * c2 - 1.0
                else:
                    s3 = (torch.sign(2.0 * c2 - 1.0) * s0).detach()
                    s4 = 2.0 * s0 + s3 - 3.0
                    p = s3 * (8.0 * c2 * c2 - 8.0 * c2 + 1.0) + s4
            elif head == "additive_margin_softmax":
                p = c - margin
            else:
                sn = torch.sqrt(torch.clamp(1.0 - c * c, min=1e-12))
                cpm = c * math.cos(margin) - sn * math.sin(margin)
                p = torch.where(c > math.cos(math.pi - margin), cpm, -cpm - 2.0)
            fs = 1.0 - fa
            onehot = torch.zeros_like(z)
            onehot[rows, lab] = 1.0
            upd = z * (1.0 - onehot) + onehot * (fs * sel + fa * (p * fn))[:, None]
    mx = upd.max(dim=1).values.detach()
    lse = mx + torch.log(torch.sum(torch.exp(upd - mx[:, None]), dim=1))
    tgt = upd[rows, lab]
    return lse - tgt, lse, tgt


def away_from_kinks(x, labels, w, head, margin):
    """Move rows whose target cosine lies within 1e-3 of a kink (0 and +-1/sqrt 2 for asoftmax, cos(pi - m) for the additive
    angle) by rescaling nothing: they are simply redrawn by the caller.  -> True when every row is clear."""
    wh = w / np.sqrt(np.maximum(np.sum(w * w, axis=0, keepdims=True), 1e-12))
    c = np.sum(x * wh[:, labels].T, axis=1) / np.maximum(np.linalg.norm(x, axis=1), 1e-12)
    kinks = {"asoftmax": [0.0, math.sqrt(0.5), -math.sqrt(0.5)], "additive_angular_margin_softmax": [math.cos(math.pi - margin)]}.get(head, [])
    return all(np.all(np.abs(c - k) >= 1e-3) for k in kinks)


CASES = [("softmax", 0.0, 0.0, True), ("softmax", 0.0, 0.0, False), ("asoftmax", 1, 0.0, False)]
for _fa in (1.0, 0.37):
    CASES += [("asoftmax", 2, _fa, False), ("asoftmax", 4, _fa, False), ("additive_margin_softmax", 0.25, _fa, False),
              ("additive_angular_margin_softmax", 0.3, _fa, False)]


@pytest.mark.parametrize("head,margin,fa,with_bias", CASES)
def test_rule_is_what_autograd_gives(head, margin, fa, with_bias):
    import torch
    n, e, c = 23, 9, 11
    seed = 0
    while True:
        rs = np.random.RandomState(1234 + seed)
        x = rs.standard_normal((n, e))
        w = rs.standard_normal((e, c))
        w[:, 4] *= 1e-8                                      # under the norm floor
        labels = rs.randint(0, c, n)
        labels[:3] = [4, 0, c - 1]
        if away_from_kinks(x, labels, w, head, margin):
            break
        seed += 1
    b = rs.standard_normal(c) if with_bias else None
    scale = 0.29
    ref = rg.classifier_grad(x, labels, w, b, head, margin, fa, scale)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = None if b is None else torch.tensor(b, dtype=torch.float64, requires_grad=True)
    loss, lse, tgt = torch_loss(xt, labels, wt, bt, head, margin, fa)
    want = ref_loss.classifier_loss(x, labels, w, b, head, margin, fa)
    for got, name in ((loss, "loss"), (lse, "lse"), (tgt, "target_logit")):
        assert np.max(np.abs(got.detach().numpy() - want[name])) <= 1e-12, name
    (scale * loss.sum()).backward()
    worst = 0.0
    for got, auto, name in ((ref["grad_x"], xt.grad, "grad_x"), (ref["grad_kernel"], wt.grad, "grad_kernel"),
                            (ref["grad_bias"], None if bt is None else bt.grad, "grad_bias")):
        if auto is None:
            assert got is None
            continue
        a = auto.numpy()
        rel = np.max(np.abs(got - a)) / np.max(np.abs(a))
        worst = max(worst, rel)
        assert rel <= 1e-10, (name, rel)
    print("%s m=%g fa=%.2f: largest relative difference to autograd %.1e" % (head, margin, fa, worst))


def test_gpu_cases_keep_the_bound_under_the_gate():
    """The condition on the inputs of tests/test_gpu_loss_grad.py: bound / largest |gradient| < 1e-4 for every tensor."""
    worst = 0.0
    for n, c, e in lc.SHAPES + [(129, 300, 33), (260, 128, 30)]:
        for same in ((False, True) if (n, c, e) in [(129, 300, 33), (260, 128, 30)] else (False,)):
            x, w, b, labels = lc.make_case(n, c, e, same)
            for head, m, fa, with_bias in lc.HEADS:
                ref, bnd = lc.reference(x, labels, w, b if with_bias else None, head, m, fa)
                for r in lc.gate_ratios(ref, bnd):
                    assert r is None or r < lc.GATE, (n, c, e, same, head, r)
                    worst = max(worst, r or 0.0)
    x, w, labels = lc.make_special()                              # the special rows of test_special_rows
    for head, m, fa in lc.SPECIAL_HEADS:
        ref, bnd = lc.reference(x, labels, w, None, head, m, fa)
        for r in lc.gate_ratios(ref, bnd):
            assert r is not None and r < lc.GATE, ("special rows", head, r)
            worst = max(worst, r)
    print("largest bound / largest |gradient|: %.2e" % worst)


# ---------------------------------------------------------------------------------------------- optimizer oracle
def test_optimizer_oracle_closed_forms():
    F = np.float32
    w, g = F([1.0, -2.0, 0.5]), F([0.5, 0.25, -1.0])
    out, _, _ = rg.opt_step(rg.SGD, w, g, lr=0.5)
    assert out.tobytes() == F([0.75, -2.125, 1.0]).tobytes()
    out, _, _ = rg.opt_step(rg.SGD, w, g, lr=0.5, l2=0.5)                       # g + 0.5 w = [1, -0.75, -0.75]
    assert out.tobytes() == F([0.5, -1.625, 0.875]).tobytes()
    out, a, _ = rg.opt_step(rg.MOMENTUM, w, g, F([1.0, 1.0, 1.0]), lr=0.5, momentum=0.5)     # a = 0.5 + g
    assert a.tobytes() == F([1.0, 0.75, -0.5]).tobytes() and out.tobytes() == F([0.5, -2.375, 0.75]).tobytes()
    out, a, _ = rg.opt_step(rg.MOMENTUM, w, g, F([1.0, 1.0, 1.0]), lr=0.5, momentum=0.5, use_nesterov=True)   # g + 0.5 a
    assert out.tobytes() == F([0.5, -2.3125, 1.125]).tobytes()
    g34 = F([3.0, 4.0, 0.0])                                                     # ||g|| = 5
    assert float(rg.grad_norm(g34)) == 5.0
    out, _, _ = rg.opt_step(rg.SGD, F([0, 0, 0]), g34, lr=1.0, clip_norm=2.5)   # halved
    assert out.tobytes() == F([-1.5, -2.0, 0.0]).tobytes()
    for clip in (5.0, 10.0):                                                     # at and above the norm: g c / c
        out, _, _ = rg.opt_step(rg.SGD, F([0, 0, 0]), g34, lr=1.0, clip_norm=clip)
        assert out.tobytes() == F([-3.0, -4.0, 0.0]).tobytes()
    # adam, first step from zero slots: m = 0.1 g, v = 0.001 g^2, lr_1 = lr sqrt(0.001) / 0.1: w - lr sign(g) up to eps
    out, m, v = rg.opt_step(rg.ADAM, w, g, F([0, 0, 0]), F([0, 0, 0]), lr=0.01, step=1)
    np.testing.assert_allclose(out, w - 0.01 * np.sign(g), rtol=0, atol=1e-6)
    np.testing.assert_allclose(m, 0.1 * g, rtol=1e-6)
    np.testing.assert_allclose(v, 0.001 * g * g, rtol=1e-6)
    assert abs(float(rg.adam_lr(0.01, 7)) - 0.01 * math.sqrt(1 - 0.999 ** 7) / (1 - 0.9 ** 7)) < 1e-9
    big = np.random.RandomState(0).standard_normal(70001).astype(F)
    assert abs(float(rg.grad_norm(big)) - math.sqrt(float(np.sum(big.astype(np.float64) ** 2)))) <= 1e-6 * 265


def test_separable_rows_seed_in_the_oracle_loop():
    """The seed of tests/test_gpu_head_train.py::test_separable_rows_are_learned, with the numpy oracle in the loop: the start
    loss lies within 0.5 of ln 8, the loss halves within 50 steps and top-1 reaches 1."""
    from tf_kaldi_speaker_amd import head_train
    rs = np.random.RandomState(0)
    centres = 3.0 * rs.standard_normal((8, 16))
    labels = np.arange(64) % 8
    x = np.asarray((centres[labels] + 0.3 * rs.standard_normal((64, 16))), dtype=np.float32)
    x = np.asarray(x / 12.0, dtype=np.float32)
    w = head_train.xavier_uniform(16, 8, 0)
    b = np.zeros(8, dtype=np.float32)
    aw, ab = np.zeros_like(w), np.zeros_like(b)
    first = None
    for t in range(50):
        ref = rg.classifier_grad(x, labels, w, b, "softmax")
        first = ref["loss"].mean() if first is None else first
        last, acc = ref["loss"].mean(), np.mean(ref["top1"] == labels)
        w, aw, _ = rg.opt_step(rg.MOMENTUM, w, ref["grad_kernel"], aw, lr=0.5, momentum=0.9)
        b, ab, _ = rg.opt_step(rg.MOMENTUM, b, ref["grad_bias"], ab, lr=0.5, momentum=0.9)
    assert abs(first - math.log(8.0)) <= 0.5 and last < 0.5 * first and acc == 1.0, (first, last, acc)


# ---------------------------------------------------------------------------------------------- batches
def data_dir(tmp_path):
    spk_utts = [("spk%d" % s, ["spk%d-u%d" % (s, u) for u in range(3)]) for s in range(5)]
    lens = {}
    for s, (_, us) in enumerate(spk_utts):
        for u, t in zip(us, (20 + 10 * s, 25 + 10 * s, 30 + 10 * s)):
            lens[u] = t
    return make_data_dir(tmp_path, spk_utts, lens, dim=4)[:2] + (lens,)


PLAN = dict(num_speakers_per_batch=3, num_segments_per_speaker=2, min_segment_len=20, max_segment_len=40, num_steps_per_epoch=6)


def test_plan_train_batches_is_deterministic_and_legal(tmp_path):
    from tf_kaldi_speaker_amd import head_train
    data, spklist, lens = data_dir(tmp_path)
    a = head_train.plan_train_batches(data, spklist, PLAN, seed=3, epoch=0)
    b = head_train.plan_train_batches(data, spklist, PLAN, seed=3, epoch=0)
    assert len(a) == 6
    for p, q in zip(a, b):
        assert p.keys == q.keys and p.starts == q.starts and p.length == q.length and np.array_equal(p.labels, q.labels)
    c = head_train.plan_train_batches(data, spklist, PLAN, seed=3, epoch=1)
    d = head_train.plan_train_batches(data, spklist, PLAN, seed=4, epoch=0)
    assert [p.keys for p in c] != [p.keys for p in a] and [p.keys for p in d] != [p.keys for p in a]
    for batch in a + c + d:
        assert 20 <= batch.length <= 40 and len(batch.keys) == 6 and batch.labels.dtype == np.int32
        assert len(set(batch.labels.tolist())) == 3                                    # distinct speakers
        assert list(batch.labels) == sorted(batch.labels, key=list(batch.labels).index)    # speaker-major
        for key, lab, start in zip(batch.keys, batch.labels, batch.starts):
            assert key.startswith("spk%d-" % lab) and lens[key] >= batch.length and 0 <= start <= lens[key] - batch.length
    feats = head_train.read_train_batch(a[0], 4)
    assert feats.shape == (6, a[0].length, 4) and feats.dtype == np.float32


def test_plan_train_batches_refusals(tmp_path):
    from tf_kaldi_speaker_amd import head_train
    data, spklist, _ = data_dir(tmp_path)
    with pytest.raises(ValueError, match="a batch needs 3"):                           # at 65 frames only spk4 qualifies
        head_train.plan_train_batches(data, spklist, dict(PLAN, min_segment_len=65, max_segment_len=65), 0, 0)
    with pytest.raises(ValueError):
        head_train.plan_train_batches(data, spklist, dict(PLAN, num_speakers_per_batch=0), 0, 0)
    with pytest.raises(ValueError):
        head_train.plan_train_batches(data, spklist, dict(PLAN, min_segment_len=41), 0, 0)
    with pytest.raises(NotImplementedError):
        head_train.plan_train_batches(data, spklist, dict(PLAN, sample_with_prob=True), 0, 0)
    # a speaker with nothing long enough is redrawn, not an error: at 45 frames spk0 and spk1 have none, three remain
    plan = head_train.plan_train_batches(data, spklist, dict(PLAN, min_segment_len=45, max_segment_len=45), 0, 0)
    assert all(set(b.labels.tolist()) == {2, 3, 4} for b in plan)


def test_learning_rate_rule_hand_worked():
    """finetune.py:154-172, 185-191 on the losses 5, 4, 4.5, 4.6, 4.7, 4.8 with reduce_lr_epochs = 2, factor 2, start 0.1:
    epoch 0, 1 improve; epoch 2: 2 - 1 < 2 keeps; epoch 3: 3 - 1 >= 2 halves, best epoch -> 2; epoch 4: 4 - 2 >= 2 halves,
    best epoch -> 3; epoch 5: 5 - 3 >= 2 halves, best epoch -> 4."""
    from tf_kaldi_speaker_amd import head_train
    rule = head_train.LearningRateRule(dict(reduce_lr_epochs=2), 0.1)
    got = [rule.after(e, v) for e, v in enumerate([5.0, 4.0, 4.5, 4.6, 4.7, 4.8])]
    assert [r for r, _ in got] == [0.1, 0.1, 0.1, 0.05, 0.025, 0.0125]
    assert [s for _, s in got] == [False] * 6 and rule.min_loss == 4.0
    # lr_start_decay_epoch holds the rate; early_stop_epochs then ends the run
    rule = head_train.LearningRateRule(dict(reduce_lr_epochs=1, lr_start_decay_epoch=10, early_stop_epochs=3), 0.1)
    got = [rule.after(e, v) for e, v in enumerate([1.0, 2.0, 2.0, 2.0])]
    assert [r for r, _ in got] == [0.1] * 4 and [s for _, s in got] == [False, False, False, True]
    # min_learning_rate stops once the next rate falls under it
    rule = head_train.LearningRateRule(dict(reduce_lr_epochs=1, min_learning_rate=0.04, learning_rate_reduce_factor=2), 0.1)
    got = [rule.after(e, v) for e, v in enumerate([1.0, 2.0, 2.0])]
    assert got == [(0.1, False), (0.05, False), (0.025, True)]
    # a learning-rate file: read off, never stops
    rule = head_train.LearningRateRule({}, 0.3, schedule=[0.3, 0.2, 0.1])
    assert rule.after(0, 9.0) == (0.2, False) and rule.after(1, 99.0) == (0.1, False) and rule.rate(1) == 0.2
    with pytest.raises(KeyError):
        head_train.LearningRateRule({}, 0.1)


def test_learning_rate_file(tmp_path):
    from tf_kaldi_speaker_amd import head_train
    path = tmp_path / "lr"
    path.write_text("0 0.10000000\n1 0.05000000\n0.025\n")
    assert head_train.read_learning_rate_file(str(path)) == [0.1, 0.05, 0.025]


def test_head_trainer_refusals_and_initialisation():
    from tf_kaldi_speaker_amd import head_train
    HT = head_train.HeadTrainer
    with pytest.raises(NotImplementedError, match="aux_loss_func"):
        HT(dict(loss_func="softmax", aux_loss_func=["ring_loss"]), 16, 8)
    with pytest.raises(NotImplementedError, match="only the softmax family"):
        HT(dict(loss_func="ge2e"), 16, 8)
    with pytest.raises(NotImplementedError, match="Not implement"):
        HT(dict(loss_func="nonsense"), 16, 8)
    with pytest.raises(NotImplementedError, match="m=3"):
        HT(dict(loss_func="asoftmax", asoftmax_m=3), 16, 8)
    with pytest.raises(ValueError, match="Optimizer rmsprop is not supported"):
        HT(dict(loss_func="softmax", optimizer="rmsprop"), 16, 8)
    with pytest.raises(ValueError, match="should not specify the momentum"):
        HT(dict(loss_func="softmax", optimizer="sgd", momentum=0.9), 16, 8)
    with pytest.raises(NotImplementedError, match="sample_with_prob"):
        HT(dict(loss_func="softmax", sample_with_prob=True), 16, 8)
    with pytest.raises(ValueError, match="kernel: expected"):
        HT(dict(loss_func="softmax"), 16, 8, kernel=np.zeros((8, 16), dtype=np.float32))
    with pytest.raises(ValueError):
        HT(dict(loss_func="softmax"), 4096, 8)
    assert head_train.optimizer_config(dict(optimizer="momentum", momentum=0.8, use_nesterov=True, weight_l2_regularizer=1e-2,
                                            output_weight_l2_regularizer=1e-3, clip_gradient=True, clip_gradient_norm=3.0)) \
        == (1, 0.8, True, 1e-3, 3.0)
    assert head_train.optimizer_config(dict(weight_l2_regularizer=1e-2, clip_gradient_norm=3.0)) == (0, 0.0, False, 1e-2, 0.0)
    k = head_train.xavier_uniform(512, 7323, seed=3)
    limit = math.sqrt(6.0 / (512 + 7323))
    assert k.shape == (512, 7323) and k.dtype == np.float32 and np.abs(k).max() <= limit and np.abs(k).max() > 0.99 * limit
    assert abs(float(k.std()) - limit / math.sqrt(3.0)) < 0.01 * limit and abs(float(k.mean())) < 0.01 * limit
    assert np.array_equal(k, head_train.xavier_uniform(512, 7323, seed=3)) and not np.array_equal(k, head_train.xavier_uniform(512, 7323, seed=4))


def test_new_entry_points_are_declared_listed_and_exported(repo_root):
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    # sizes are host arithmetic: the least workspace is a panel of 32 rows, the full one min(round32(n), 1024)
    n, c, e = 5000, 7323, 512
    per_row = 4 * ((c + 3) // 4 * 4 + c + e)
    assert lib.xv_loss_grad_workspace(n, c, e) - lib.xv_loss_grad_workspace_min(n, c, e) == (1024 - 32) * per_row
    assert lib.xv_loss_grad_workspace(0, c, e) == 0 and lib.xv_opt_workspace(4097) == 16 and lib.xv_opt_workspace(0) == 0
    fixed = lib.xv_loss_grad_workspace_min(n, c, e) - 32 * per_row - lib.xv_loss_workspace(n, c)
    assert fixed <= 4 * c * 512 + 4 * e * (c + 3) + 520 * c + 16 * n + 256 * 9        # O(C ldc) + the transpose + 16 n
