"""Host: what tf_kaldi_speaker_amd/att_train.py decides without a device: check_supported's refusals with their words, the
variable names against synth.synth_weights of an attention config, trained_names and l2_assignment, and that the statistics
pooling trainers keep refusing self_attention with the message they have."""
import pytest

from tf_kaldi_speaker_amd import _lib, att_train, conv_train, frame_train, synth, tail_train

ATT = dict(synth.TDNN_ATT_PARAMS, loss_func="softmax", optimizer="momentum", momentum=0.9, use_nesterov=False,
           weight_l2_regularizer=1e-2, num_nodes_pooling_layer=24, num_nodes_last_layer=16,
           att_key_num_nodes=[12, 8], att_key_network_type=1, att_num_heads=2)


def refused(params, words, conv_layers=False):
    with pytest.raises(NotImplementedError) as e:
        att_train.check_supported(params, conv_layers)
    assert words in str(e.value), str(e.value)


def test_the_reference_config_is_supported():
    att_train.check_supported(ATT)
    att_train.check_supported(ATT, conv_layers=True)
    att_train.check_supported(dict(ATT, att_key_input="tdnn3_relu"))            # the frozen node itself may feed the key
    att_train.check_supported(dict(ATT, att_key_input="tdnn5_relu"))            # both on the same node
    att_train.check_supported(dict(ATT, network_type="extended_tdnn", att_key_input="tdnn9_relu", att_value_input="tdnn10_relu"))


def test_refusals_and_their_words():
    refused(dict(ATT, att_key_network_type=3), "att_key_network_type 3 (tanh): xv_seg_forward has no such activation")
    refused(dict(ATT, att_value_num_nodes=[8], att_value_network_type=3), "att_value_network_type 3 (tanh)")
    refused(dict(ATT, att_apply_nonlinear=True), "att_apply_nonlinear")
    refused(dict(ATT, att_penalty_term=0.1), "att_penalty_term > 0")
    refused(dict(ATT, att_key_num_nodes=[8] * (_lib.XV_MAX_ATT_LAYERS + 1)), "att_key_num_nodes needs 1 .. %d" % _lib.XV_MAX_ATT_LAYERS)
    refused(dict(ATT, att_value_num_nodes=[8] * (_lib.XV_MAX_ATT_LAYERS + 1)), "att_value_num_nodes at most")
    refused(dict(ATT, att_key_num_nodes=[]), "att_key_num_nodes needs 1")
    refused(dict(ATT, network_type="resnet_18"), "resnet_18")
    refused(dict(ATT, pooling_type="statistics_pooling"), "att_train trains self_attention models")
    refused(dict(ATT, att_value_input="tdnn4_relu"), "the last frame layer tdnn5 reaches the pooled vector through neither")
    refused(dict(ATT, att_key_input="tdnn2_relu"), "a multi-tap layer lies between them", conv_layers=True)
    refused(dict(ATT, att_key_input="tdnn2_relu"), "a multi-tap layer lies between them")
    refused(dict(ATT, network_type="extended_tdnn", att_key_input="tdnn6_relu", att_value_input="tdnn10_relu"), "multi-tap")
    refused(dict(ATT, att_key_input="tdnn4_bn"), "only the tdnn<i>_relu endpoints")
    refused(dict(ATT, att_key_input="tdnn6_relu"), "only the tdnn<i>_relu endpoints")
    # in front of the frozen node: the frame-layer variant alone
    etdnn = dict(ATT, network_type="extended_tdnn", att_key_input="tdnn6_relu", att_value_input="tdnn10_relu")
    front = dict(etdnn, att_key_input="tdnn5_relu")                              # tdnn6 has one tap: the lengths agree...
    refused(front, "multi-tap")                                                  # ...but tdnn7 between them has seven
    front = dict(ATT, network_type="extended_tdnn", att_key_input="tdnn8_relu", att_value_input="tdnn10_relu")
    att_train.check_supported(front)
    # everything tail_train refuses
    refused(dict(ATT, network_relu_type="prelu"), "prelu")
    refused(dict(ATT, feature_norm=True), "feature_norm")
    with pytest.raises(NotImplementedError):
        tail_train.check_supported(dict(ATT, network_relu_type="prelu"))


def test_an_input_in_front_of_the_frozen_node():
    # the extended TDNN's tdnn8 .. tdnn10 are trained behind tdnn7_relu; tdnn7 is a convolution, so an input in front of the frozen
    # node always has another length: build the case on a net whose frozen node is followed by 1-tap layers only
    p = dict(ATT, att_key_input="tdnn3_relu")
    att_train.check_supported(p)                                                 # the frozen node itself: its rows are the input
    for name in ("tdnn1_relu", "tdnn2_relu"):
        with pytest.raises(NotImplementedError) as e:
            att_train.check_supported(dict(ATT, att_key_input=name, att_value_input="tdnn5_relu"))
        assert "multi-tap" in str(e.value) or "in front of the frozen node" in str(e.value)
    # the message itself, on a table where the lengths agree: widths patched so that no multi-tap layer lies between
    nets = dict(conv_train._NETS)
    try:
        conv_train._NETS["tdnn"] = ("tdnn", (5, 1, 1, 1, 1))
        refused(dict(ATT, att_key_input="tdnn2_relu"), "att_key_input tdnn2_relu lies in front of the frozen node tdnn3_relu")
        att_train.check_supported(dict(ATT, att_key_input="tdnn2_relu"), conv_layers=True)
    finally:
        conv_train._NETS.clear()
        conv_train._NETS.update(nets)


def test_statistics_trainers_keep_refusing_attention():
    for mod in (frame_train, conv_train):
        with pytest.raises(NotImplementedError) as e:
            mod.check_supported(ATT)
        assert "only the gradient of statistics_pooling is implemented" in str(e.value)


@pytest.mark.parametrize("conv_layers", [False, True])
def test_names_against_the_synthetic_checkpoint(conv_layers):
    weights = synth.synth_weights(ATT, 30, seed=1, channels=20)
    names = att_train.trained_names(ATT, conv_layers)
    assert len(names) == len(set(names))
    missing = [n for n in names if n not in weights and not n.startswith("softmax/")]
    assert not missing, missing
    attention = [k for k in weights if "/attention/" in k and "moving" not in k]
    assert attention and all(k in names for k in attention)                     # every attention variable is trained
    key, value, query = att_train.attention_variables(ATT)
    assert [s.kernel for s in key] == ["tdnn/attention/att_key0/att_key0_dense/kernel", "tdnn/attention/att_key1/att_key1_dense/kernel"]
    assert key[0].bn == "tdnn/attention/att_key0/att_key0_bn" and key[1].bn is None and value == ()
    assert key[0].act == _lib.XV_SEG_ACT_RELU and key[1].act == _lib.XV_SEG_ACT_RELU and query == "tdnn/attention/query"
    assert weights[query].shape == (2, 4)                                       # att_split_key: 8 / 2 heads
    frame = (conv_train if conv_layers else frame_train).trained_names(dict(ATT, pooling_type="statistics_pooling"))
    tail = tail_train.trained_names(ATT)
    assert names[:len(frame) - len(tail)] == frame[:len(frame) - len(tail)] and names[-len(tail):] == tail
    assert names[len(frame) - len(tail)] == key[0].kernel and names[-len(tail) - 1] == query
    kinds = att_train.attention_variables(dict(ATT, att_key_network_type=0, att_value_num_nodes=[6, 4], att_value_network_type=2,
                                               network_relu_type="lrelu"))
    assert kinds[0][1].act == _lib.XV_SEG_ACT_NONE and kinds[0][1].bn is None
    assert [s.bn is not None for s in kinds[1]] == [True, True] and kinds[1][1].act == _lib.XV_SEG_ACT_LRELU


def test_l2_assignment():
    l2 = att_train.l2_assignment(ATT, True)
    assert set(l2) == set(att_train.trained_names(ATT, True))
    for name, factor in l2.items():
        if name.startswith("softmax/"):
            continue
        assert factor == (1e-2 if name.endswith("/kernel") else 0.0), name
    assert l2["tdnn/attention/query"] == 0.0 and l2["tdnn/attention/att_key1/att_key1_dense/kernel"] == 1e-2
    assert l2["softmax/output/kernel"] == tail_train.l2_assignment(ATT)["softmax/output/kernel"]
