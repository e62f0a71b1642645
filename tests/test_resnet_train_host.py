"""CPU: the pure host side of tf_kaldi_speaker_amd/resnet_train.py -- the names and l2 factors of everything ResNetTrainer
updates, for resnet_blocks [2, 2, 2, 2] and [2, 1, 1, 1] with and without the time stride, against the names
synth.synth_resnet_weights gives its variables; every refusal and its word; the HWIO kernel round trip; the absent-bias paths of
the tail_train helpers (and that the with-bias paths return what they returned); where train_head sends a ResNet; and the seed
precondition of tests/test_gpu_resnet_train.py, with torch float32 standing in for the device."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_resnet_train as rr                                       # noqa: E402

from tf_kaldi_speaker_amd import conv_train, frame_train, resnet_train, synth, tail_train      # noqa: E402

BN = ("gamma", "beta", "moving_mean", "moving_variance")


def params_of(**extra):
    return dict(dict(synth.RESNET_PARAMS, optimizer="momentum", momentum=0.9), **extra)


@pytest.mark.parametrize("blocks", ([2, 2, 2, 2], [2, 1, 1, 1]))
@pytest.mark.parametrize("stride", (False, True))
def test_names_and_l2(blocks, stride):
    params = params_of(resnet_blocks=blocks, resnet_time_stride=stride)
    weights = synth.synth_resnet_weights(params, seed=1, width=4)
    names = resnet_train.trained_names(params)
    assert len(names) == len(set(names))
    # everything the checkpoint holds is trained, but the moving statistics; the head is added behind
    want = [k for k in weights if not k.endswith("moving_mean") and not k.endswith("moving_variance")]
    assert set(names) == set(want) | {"softmax/output/kernel", "softmax/output/bias"}
    grid = resnet_train.grid_variables(params)
    assert len(grid) == 1 + 2 * sum(blocks) + 4 and all(s.bias is None for s in grid)
    shorts = [s for s in grid if "_conv_short/" in s.kernel]
    assert [s.kernel for s in shorts] == ["resnet_18/conv%da_conv_short/kernel" % i for i in (1, 2, 3, 4)]
    st = 2 if stride else 1
    assert [s.window for s in shorts] == [(1, 1, 1, 1)] + [(1, 1, st, 2)] * 3
    for s in grid:                                                  # the kernel's window is the checkpoint's
        assert weights[s.kernel].shape[:2] == s.window[:2], s.kernel
        strided = s.kernel.split("/")[1] in ("conv%da_conv%s" % (i, t) for i in (2, 3, 4) for t in ("0", "_short"))
        assert s.window[2:] == ((st, 2) if strided else (1, 1)), s.kernel
    order = [s.kernel for s in resnet_train.frame_variables(params)]
    assert order[0] == "resnet_18/conv0_1/kernel" and order[1:4] == ["resnet_18/conv1a_conv%s/kernel" % t for t in ("0", "1", "_short")]
    assert order[-3:] == ["resnet_18/%s/kernel" % n for n in ("conv5", "dense1", "dense2")]
    assert names[-4:-2] == ["resnet_18/tdnn7_bn/gamma", "resnet_18/tdnn7_bn/beta"] and names[0] == order[0]
    l2 = resnet_train.l2_assignment(params)
    assert set(l2) == set(names)
    for k, v in l2.items():
        if k == "softmax/output/kernel":
            continue
        assert v == (1e-2 if k.endswith("/kernel") else 0.0), k
    metric = dict(params, loss_func="angular_triplet_loss")
    assert resnet_train.metric_trained_names(metric) == names[:-2]
    assert resnet_train.metric_l2_assignment(metric) == {k: v for k, v in l2.items() if not k.startswith("softmax/")}
    assert list(resnet_train.out_lens([9, 14, 11, 1, 0], 2)) == [5, 7, 6, 1, 0] and list(resnet_train.out_lens([9, 14], 1)) == [9, 14]


def test_refusals_and_their_words():
    ok = params_of()
    resnet_train.check_supported(ok)
    for extra, word in ((dict(resnet_maxpooling=True), "resnet_maxpooling"), (dict(network_relu_type="prelu"), "prelu"),
                        (dict(feature_norm=True), "feature_norm"), (dict(pooling_type="self_attention"), "statistics_pooling"),
                        (dict(network_type="tdnn"), "Not implement tdnn network"), (dict(sample_with_prob=True), "sample_with_prob"),
                        (dict(loss_func="generalized_angular_triplet_loss"), "loss")):
        with pytest.raises(NotImplementedError) as e:
            resnet_train.check_supported(params_of(**extra))
        assert word in str(e.value), (extra, str(e.value))
    with pytest.raises(ValueError) as e:                            # head_train.optimizer_config's word
        resnet_train.check_supported(params_of(optimizer="rmsprop"))
    assert "rmsprop" in str(e.value)
    with pytest.raises(NotImplementedError):
        resnet_train.check_supported(ok, metric=True)               # softmax behind the metric door
    resnet_train.check_supported(params_of(loss_func="angular_triplet_loss", margin=0.2, triplet_type="all",
                                           loss_type="additive_margin_softmax"), metric=True)
    with pytest.raises(ValueError):
        resnet_train.block_plan(params_of(resnet_blocks=[2, 0, 1, 1]))
    # the other stages keep refusing the ResNet in their own words
    for mod, word in ((frame_train, "resnet_18: no 1-tap frame layers"), (conv_train, "resnet_18: no 1-tap frame layers")):
        with pytest.raises(NotImplementedError) as e:
            mod.check_supported(ok)
        assert word in str(e.value)
    from tf_kaldi_speaker_amd import att_train
    with pytest.raises(NotImplementedError):
        att_train.check_supported(params_of(pooling_type="self_attention"), True, False)


def test_kernel_round_trip():
    r = np.random.RandomState(2)
    for shape in ((3, 3, 5, 7), (1, 1, 4, 6), (3, 3, 1, 4)):
        k = r.standard_normal(shape).astype(np.float32)
        rows, window, channels = resnet_train.kernel_to_rows(k)
        assert rows.shape == (shape[3], shape[0] * shape[1] * shape[2]) and window == shape[:2] and channels == shape[2]
        dl, df, c, j = shape[0] - 1, 0, shape[2] - 1, 2
        assert rows[j, (dl * shape[1] + df) * shape[2] + c] == k[dl, df, c, j]
        assert resnet_train.rows_to_kernel(rows, shape).tobytes() == k.tobytes()
    with pytest.raises(ValueError):
        resnet_train.kernel_to_rows(np.zeros((3, 4, 5), np.float32))
    # conv5's [1, 5, C, N] as [5 C, N] rows is the same order: k = f C + c
    k = r.standard_normal((1, 5, 3, 4)).astype(np.float32)
    rows, taps, channels = conv_train.kernel_to_rows(k.reshape(15, 4))
    assert taps == 1 and channels == 15 and rows[1, 2 * 3 + 1] == k[0, 2, 1, 1]
    assert conv_train.rows_to_kernel(rows, k.shape).tobytes() == k.tobytes()


def test_absent_bias_in_the_shared_helpers():
    Spec = resnet_train.GridSpec
    nob = Spec("s/conv/kernel", None, "s/bn", 1, (3, 3, 1, 1))
    withb = tail_train.SegSpec("s/dense/kernel", "s/dense/bias", "s/dbn", 1)
    w = {"s/conv/kernel": np.zeros((3, 3, 1, 2), np.float32), "s/dense/kernel": np.ones((2, 2), np.float32),
         "s/dense/bias": np.arange(2, dtype=np.float32)}
    for scope in ("s/bn", "s/dbn"):
        for i, s in enumerate(BN):
            w[scope + "/" + s] = np.full(2, float(i), np.float32)
    k, b, bn = tail_train.layer_weights(nob, w)
    assert k is w["s/conv/kernel"] and b is None and [float(v[0]) for v in bn] == [0.0, 1.0, 2.0, 3.0]
    k, b, bn = tail_train.layer_weights(withb, w)                    # what it returned before
    assert k is w["s/dense/kernel"] and b is w["s/dense/bias"] and len(bn) == 4
    with pytest.raises(KeyError) as e:
        tail_train.layer_weights(withb, {k: v for k, v in w.items() if k != "s/dense/bias"})
    assert str(e.value).strip("'\"") == "the checkpoint lacks s/dense/bias"
    with pytest.raises(KeyError) as e:
        tail_train.layer_weights(nob, {k: v for k, v in w.items() if k != "s/bn/beta"})
    assert "the checkpoint lacks s/bn/beta" in str(e.value)
    params = dict(synth.TDNN_STAT_PARAMS)
    assert frame_train.stacked_names((withb,), params)[:4] == ["s/dense/kernel", "s/dense/bias", "s/dbn/gamma", "s/dbn/beta"]
    assert frame_train.stacked_names((nob,), params)[:3] == ["s/conv/kernel", "s/bn/gamma", "s/bn/beta"]
    assert frame_train.stacked_l2((nob,), dict(params, weight_l2_regularizer=0.5))["s/conv/kernel"] == 0.5

    class Fake(object):                                               # what layer_tensors and layer_variables read of a layer
        def __init__(self, bias):
            self.b, self.bn, self.batch_stats = bias, [FakeT(i) for i in range(4)], False
            self.slots = collections.defaultdict(list)

        def trained(self):
            return [("kernel", "W", "GW")] + ([("bias", self.b, "GB")] if self.b is not None else []) + [("gamma", "G", "GG"),
                                                                                                        ("beta", "B", "GBE")]

        def kernel(self):
            return "K"

    class FakeT(object):
        def __init__(self, v):
            self.v = v

        def cpu(self):
            return self

        def numpy(self):
            return np.full(2, float(self.v), np.float32)

    assert [t[0] for t in tail_train.layer_tensors((nob, withb), (Fake(None), Fake(FakeT(7))))] == [
        "s/conv/kernel", "s/bn/gamma", "s/bn/beta", "s/dense/kernel", "s/dense/bias", "s/dbn/gamma", "s/dbn/beta"]
    out = tail_train.layer_variables((nob, withb), (Fake(None), Fake(FakeT(7))))
    assert list(out) == ["s/conv/kernel", "s/bn/gamma", "s/bn/beta", "s/dense/kernel", "s/dense/bias", "s/dbn/gamma", "s/dbn/beta"]
    assert float(out["s/dense/bias"][0]) == 7.0


def test_train_head_sends_a_resnet_to_its_trainer(monkeypatch):
    """conv_layers on a ResNet reaches resnet_train.check_supported before conv_train's refusal; frame_layers alone stays
    refused in frame_train's words."""
    from tf_kaldi_speaker_amd import head_train
    from tf_kaldi_speaker_amd.params import Params
    seen = []

    class Stop(Exception):
        pass

    def spy(params, metric=False):
        seen.append(metric)
        raise Stop()
    monkeypatch.setattr(resnet_train, "check_supported", spy)
    from tf_kaldi_speaker_amd import valid
    monkeypatch.setattr(valid, "read_speaker_info", lambda *a, **k: (None, 3))
    trainer = collections.namedtuple("T", "params embeddings model dim")(Params(**params_of(learning_rate=0.1, num_epochs=1, reduce_lr_epochs=2)), "x", None,
                                                                    40)
    with pytest.raises(Stop):
        head_train.train_head(trainer, "d", "s", "d", "s", "o", weights={}, conv_layers=True)
    assert seen == [False]

    class T(object):
        params, embeddings, model, dim = trainer.params, "x", None, 40
    with pytest.raises(NotImplementedError) as e:
        head_train.train_head(T(), "d", "s", "d", "s", "o", weights={}, frame_layers=True)
    assert "resnet_18: no 1-tap frame layers" in str(e.value) and T.embeddings == "x"


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_seed_precondition(name):
    """No activation input of the case changes sign between float64 and float32, and the smallest |h| keeps MARGIN times its
    layer's largest float32-to-float64 difference."""
    mode, extra, seed, measured = rr.CASES[name]
    params, weights, feats, off = rr.small_model(seed, **extra)
    ratio, count, flips, worst = rr.sign_margin(params, weights, feats, np.diff(off), mode == "batch")
    print("%s: seed %d, %d activation inputs, %d sign changes, smallest |h| / largest layer error %.1f (recorded %.1f), "
          "largest layer error %.1e of the layer's rms" % (name, seed, count, flips, ratio, measured, worst))
    assert flips == 0 and ratio >= rr.MARGIN
    assert count == (38752 if extra.get("resnet_time_stride") else 62976)
