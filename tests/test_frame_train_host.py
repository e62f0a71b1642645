"""Host: the host side of tf_kaldi_speaker_amd/frame_train.py: the variable names of the trailing 1-tap frame layers and the
frozen node for the TDNN and the extended TDNN, trained_names, the l2 assignment, every refusal of check_supported, and the
command line's new flag."""
import pytest

from tf_kaldi_speaker_amd import _lib, frame_train, synth, tail_train

TDNN = dict(synth.TDNN_STAT_PARAMS)
ETDNN = dict(synth.TDNN_STAT_PARAMS, network_type="extended_tdnn")


def test_frame_variables_and_frozen_node():
    specs = frame_train.frame_variables(TDNN)
    assert [s.kernel for s in specs] == ["tdnn/tdnn4_dense/kernel", "tdnn/tdnn5_dense/kernel"]
    assert [s.bias for s in specs] == ["tdnn/tdnn4_dense/bias", "tdnn/tdnn5_dense/bias"]
    assert [s.bn for s in specs] == ["tdnn/tdnn4_bn", "tdnn/tdnn5_bn"]
    assert all(s.act == _lib.XV_SEG_ACT_RELU for s in specs)
    assert frame_train.frozen_node(TDNN) == "tdnn3_relu"
    specs = frame_train.frame_variables(ETDNN)
    assert [s.kernel for s in specs] == ["etdnn/tdnn%d_dense/kernel" % i for i in (8, 9, 10)]
    assert [s.bn for s in specs] == ["etdnn/tdnn%d_bn" % i for i in (8, 9, 10)]
    assert frame_train.frozen_node(ETDNN) == "tdnn7_relu"
    assert all(s.act == _lib.XV_SEG_ACT_LRELU for s in frame_train.frame_variables(dict(TDNN, network_relu_type="lrelu")))
    # these are the 1-tap layers behind the last multi-tap one, by the widths the graph is built from
    for params in (TDNN, ETDNN):
        widths = synth.net_spec(params)[1]
        last_conv = max(i for i, w in enumerate(widths, start=1) if w > 1)
        names = ["%s/tdnn%d_dense/kernel" % (synth.net_spec(params)[0], i) for i in range(last_conv + 1, len(widths) + 1)]
        assert [s.kernel for s in frame_train.frame_variables(params)] == names
        assert frame_train.frozen_node(params) == "tdnn%d_relu" % last_conv
        weights = synth.synth_weights(params, 30, seed=0, channels=8)
        assert all(n in weights for n in frame_train.trained_names(params) if not n.startswith("softmax/"))


def test_trained_names():
    names = frame_train.trained_names(TDNN)
    frame = []
    for i in (4, 5):
        frame += ["tdnn/tdnn%d_dense/kernel" % i, "tdnn/tdnn%d_dense/bias" % i, "tdnn/tdnn%d_bn/gamma" % i, "tdnn/tdnn%d_bn/beta" % i]
    assert names == frame + tail_train.trained_names(TDNN)
    assert len(set(names)) == len(names) and not any("moving" in n for n in names)
    assert frame_train.trained_names(dict(ETDNN, loss_func="amsoftmax", amsoftmax_m=0.2))[-1] == "softmax/output/kernel"
    assert len(frame_train.trained_names(ETDNN)) == 3 * 4 + len(tail_train.trained_names(ETDNN))


def test_l2_assignment():
    params = dict(ETDNN, weight_l2_regularizer=1e-3, output_weight_l2_regularizer=5e-2)
    l2 = frame_train.l2_assignment(params)
    assert set(l2) == set(frame_train.trained_names(params))
    for name, v in l2.items():
        if name == "softmax/output/kernel":
            assert v == 5e-2                                          # the head keeps its own rule
        elif name.endswith("_dense/kernel"):
            assert v == 1e-3, name                                    # every dense kernel, the frame layers' included
        else:
            assert v == 0.0, name
    assert sum(1 for n in l2 if n.endswith("_dense/kernel")) == 5
    tail = tail_train.l2_assignment(params)
    assert all(l2[k] == v for k, v in tail.items())


@pytest.mark.parametrize("bad,word", [
    (dict(network_type="resnet_18"), "resnet_18"),
    (dict(pooling_type="self_attention"), "statistics_pooling"),
    (dict(pooling_type="lde"), "statistics_pooling"),
    (dict(network_relu_type="prelu"), "prelu"),
    (dict(feature_norm=True), "feature_norm"),
    (dict(network_type="ftdnn"), "ftdnn"),
    (dict(sample_with_prob=True), "sample_with_prob"),
    (dict(loss_func="ge2e"), ""),
])
def test_check_supported_refuses(bad, word):
    with pytest.raises(NotImplementedError) as e:
        frame_train.check_supported(dict(TDNN, **bad))
    assert word in str(e.value) and str(e.value)
    # everything tail_train refuses is refused here as well
    if "pooling_type" not in bad and bad.get("network_type") != "resnet_18":
        with pytest.raises(NotImplementedError):
            tail_train.check_supported(dict(TDNN, **bad))


def test_check_supported_accepts():
    frame_train.check_supported(TDNN)
    frame_train.check_supported(dict(ETDNN, network_relu_type="lrelu", optimizer="adam"))
    with pytest.raises(ValueError):
        frame_train.check_supported(dict(TDNN, optimizer="rmsprop"))


def test_command_line_flag():
    from tf_kaldi_speaker_amd import train_head
    args = train_head.build_parser().parse_args(["--frame-layers", "a", "b", "c", "d", "e", "f"])
    assert args.frame_layers and not args.segment_layers
    args = train_head.build_parser().parse_args(["a", "b", "c", "d", "e", "f"])
    assert not args.frame_layers
    assert "--frame-layers" in train_head.build_parser().format_help()
