"""No GPU: the host side of training from scratch (tf_kaldi_speaker_amd/train.py): fresh_weights against the variable sets of
synth.py, the rule rebuilt from the files of a run that stopped, the optimizer file -c insists on, and the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from valid_data import make_data_dir                                # noqa: E402

HEAD_K, HEAD_B = "softmax/output/kernel", "softmax/output/bias"
SPEAKERS = 7


def _configs():
    from tf_kaldi_speaker_amd import synth
    small = dict(num_nodes_pooling_layer=24, num_nodes_last_layer=16)
    att = dict(synth.TDNN_ATT_PARAMS, num_nodes_pooling_layer=24, num_nodes_last_layer=16, att_key_num_nodes=[12, 12])
    return {
        "tdnn": (dict(synth.TDNN_STAT_PARAMS, **small), 30),
        "attention": (att, 30),
        "attention_xavier": (dict(att, att_query_init="xavier_init", att_num_heads=2, att_split_key=False), 30),
        "etdnn": (dict(synth.TDNN_STAT_PARAMS, network_type="extended_tdnn", **small), 23),
        "resnet": (dict(synth.RESNET_PARAMS, **small), 40),
        "amsoftmax": (dict(synth.TDNN_STAT_PARAMS, loss_func="additive_margin_softmax", amsoftmax_m=0.2, amsoftmax_lambda_min=0,
                           amsoftmax_lambda_base=10, amsoftmax_lambda_gamma=1, amsoftmax_lambda_power=4, **small), 30),
        "triplet": (dict(synth.TDNN_STAT_PARAMS, loss_func="angular_triplet_loss", margin=0.2, triplet_type="all",
                         loss_type="additive_margin_softmax", num_speakers_per_batch=3, num_segments_per_speaker=2, **small), 30),
    }


def _synth(params, dim):
    from tf_kaldi_speaker_amd import synth
    if params["network_type"] == "resnet_18":
        return synth.synth_resnet_weights(params, 0, width=4)
    return synth.synth_weights(params, dim, 0, channels=8)


def _limit(shape):
    receptive = int(np.prod(shape[:-2]))
    return np.sqrt(6.0 / (receptive * (shape[-2] + shape[-1])))


@pytest.mark.parametrize("name", ["tdnn", "attention", "attention_xavier", "etdnn", "resnet", "amsoftmax", "triplet"])
def test_fresh_weights_are_the_synth_variable_set_with_tensorflows_defaults(name):
    from tf_kaldi_speaker_amd import train
    params, dim = _configs()[name]
    want = {k: v.shape for k, v in _synth(params, dim).items()}
    if name != "triplet":
        want[HEAD_K] = (16, SPEAKERS)
        if params["loss_func"] == "softmax":
            want[HEAD_B] = (SPEAKERS,)
    w = train.fresh_weights(params, dim, SPEAKERS, seed=3, channels=8, width=4)
    assert {k: v.shape for k, v in w.items()} == want and all(v.dtype == np.float32 for v in w.values())
    kernels = 0
    for k, v in w.items():
        leaf = k.rsplit("/", 1)[-1]
        if leaf == "kernel":
            kernels += 1
            assert np.abs(v).max() <= np.float32(_limit(v.shape)) and np.unique(v).size > 1, k
            if v.size >= 64:                                          # uniform up to the limit, not a narrower box
                assert np.abs(v).max() > 0.8 * _limit(v.shape), k
        elif leaf in ("bias", "beta", "moving_mean"):
            assert not v.any(), k
        elif leaf in ("gamma", "moving_variance"):
            assert np.all(v == 1.0), k
        else:
            assert leaf == "query"
            if params.get("att_query_init") == "xavier_init":
                assert np.abs(v).max() <= _limit(v.shape) and np.unique(v).size > 1
            else:
                assert np.abs(v).max() <= 0.2 and np.unique(v).size > 1    # truncated at two standard deviations of 0.1
    assert kernels >= 7
    again = train.fresh_weights(params, dim, SPEAKERS, seed=3, channels=8, width=4)
    other = train.fresh_weights(params, dim, SPEAKERS, seed=4, channels=8, width=4)
    assert all(w[k].tobytes() == again[k].tobytes() for k in w)
    assert all(w[k].tobytes() != other[k].tobytes() for k in w if k.endswith("kernel"))
    # every variable has its own stream: two kernels of one shape differ
    by_shape = {}
    for k in sorted(w):
        if k.endswith("kernel") and w[k].shape in by_shape:
            assert w[k].tobytes() != w[by_shape[w[k].shape]].tobytes()
        by_shape.setdefault(w[k].shape, k)


def test_the_full_size_defaults_are_the_references_widths():
    from tf_kaldi_speaker_amd import synth, train
    w = train.fresh_weights(dict(synth.TDNN_STAT_PARAMS), 30, 5, seed=0)
    assert w["tdnn/tdnn1_conv/kernel"].shape == (1, 5, 30, 512) and w["tdnn/tdnn5_dense/kernel"].shape == (512, 1500)
    assert w[HEAD_K].shape == (512, 5)


REFUSED = [
    (dict(network_relu_type="prelu"), "network_relu_type prelu"),
    (dict(feature_norm=True, feature_scaling_factor=10), "feature_norm"),
    (dict(aux_loss_func=["ring_loss"]), "aux_loss_func"),
    (dict(loss_func="generalized_angular_triplet_loss"), "generalized_angular_triplet_loss"),
]


@pytest.mark.parametrize("extra,word", REFUSED, ids=[w for _, w in REFUSED])
def test_what_the_trainers_refuse_stays_refused_before_anything_is_written(tmp_path, extra, word):
    import json
    from tf_kaldi_speaker_amd import conv_train, synth, train
    params = dict(synth.TDNN_STAT_PARAMS, **extra)
    with pytest.raises(NotImplementedError) as want:
        conv_train.check_supported(params)
    with pytest.raises(NotImplementedError) as got:
        train.fresh_weights(params, 30, 5, seed=0, channels=8)
    assert str(got.value) == str(want.value) and word in str(got.value)
    config = str(tmp_path / "config.json")
    with open(config, "w") as f:
        json.dump(params, f)
    model = str(tmp_path / "model")
    with pytest.raises(SystemExit) as e:
        train.main(["--config", config, "train", "spklist", "valid", "spklist", model])
    assert str(want.value) in str(e.value.code) and not os.path.exists(model)


def test_more_than_one_gpu_is_refused(tmp_path, capsys):
    from tf_kaldi_speaker_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["-n", "2", "--config", "x.json", "train", "spklist", "valid", "spklist", str(tmp_path / "model")])
    assert e.value.code == 2 and "more than one GPU" in capsys.readouterr().err
    with pytest.raises(NotImplementedError, match="more than one GPU"):
        train.train("train", "spklist", "valid", "spklist", str(tmp_path / "model"), config={}, num_gpus=2)
    assert not os.path.exists(str(tmp_path / "model"))


def test_trainer_build_train_still_raises():
    from tf_kaldi_speaker_amd import synth
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    tr = Trainer(Params(**dict(synth.TDNN_STAT_PARAMS)), None, 30, single_cpu=True)
    with pytest.raises(NotImplementedError, match=r"build\('train'\) is not implemented"):
        tr.build("train")


# ---------------------------------------------------------------------------------------------- continuing
RULE = dict(learning_rate=0.02, num_epochs=12, reduce_lr_epochs=2, min_learning_rate=1e-3)
LOSSES = [2.0, 1.5, 1.6, 1.7, 1.4, 1.45, 1.46, 1.47, 1.48, 1.49, 1.5, 1.51]


def _write_files(nnet, rule, epochs):
    """What head_train.finish_epoch writes for the epochs 0 .. epochs - 1 of an uninterrupted run -> [(next rate, stop)]."""
    os.makedirs(nnet, exist_ok=True)
    out = []
    for epoch in range(epochs):
        new_lr, stop = rule.after(epoch, LOSSES[epoch])
        with open(os.path.join(nnet, "learning_rate"), "a") as f:
            if epoch == 0:
                f.write("0 %.8f\n" % rule.rate(0))
            f.write("%d %.8f\n" % (epoch + 1, new_lr))
        with open(os.path.join(nnet, "valid_loss"), "a") as f:
            f.write("%d %f %f\n" % (epoch, LOSSES[epoch], 0.25))
        out.append((new_lr, stop))
    return out


def test_the_rule_of_the_training_script_stops_late():
    """early_stop_epochs defaults to 10 here (train.py:108-109), to 5 in fine-tuning: with the rate held up by
    lr_start_decay_epoch the same losses stop the two rules at different epochs."""
    from tf_kaldi_speaker_amd import head_train, train
    params = dict(RULE, lr_start_decay_epoch=100)
    rule, epochs = train.make_rule(params)
    assert epochs == 12 and rule.early_stop_epochs == 10
    stops = [rule.after(e, LOSSES[min(e, 11)] if e < 5 else 9.0)[1] for e in range(16)]
    assert stops.index(True) == 14                                           # the minimum is epoch 4
    fine = head_train.LearningRateRule(params, 0.02)
    assert [fine.after(e, LOSSES[min(e, 11)] if e < 5 else 9.0)[1] for e in range(16)].index(True) == 9


@pytest.mark.parametrize("stopped_after", range(1, 12))
def test_the_rebuilt_rule_goes_on_as_the_uninterrupted_one(tmp_path, stopped_after):
    from tf_kaldi_speaker_amd import train
    whole, _ = train.make_rule(RULE)
    want = _write_files(str(tmp_path / "whole"), whole, 12)
    assert any(stop for _, stop in want) and len({r for r, _ in want}) >= 3            # the rate falls and the rule stops
    nnet = str(tmp_path / "part")
    first, _ = train.make_rule(RULE)
    _write_files(nnet, first, stopped_after)
    rule, epochs = train.make_rule(RULE, nnet, stopped_after)
    assert epochs == 12 and rule.rate(stopped_after) == first.rate(stopped_after)
    assert (rule.min_loss, rule.min_loss_epoch) == (first.min_loss, first.min_loss_epoch)
    got = [rule.after(e, LOSSES[e]) for e in range(stopped_after, 12)]
    assert got == want[stopped_after:]


def test_a_rule_cannot_be_rebuilt_from_files_that_are_too_short(tmp_path):
    from tf_kaldi_speaker_amd import train
    nnet = str(tmp_path / "short")
    _write_files(nnet, train.make_rule(RULE)[0], 2)
    with pytest.raises(ValueError, match="valid_loss does not hold the epochs 0 .. 2"):
        train.make_rule(RULE, nnet, 3)


def test_continuing_without_the_optimizer_file_is_an_error_that_names_it(tmp_path):
    from tf_kaldi_speaker_amd import model_io, synth, train
    params = dict(synth.TDNN_STAT_PARAMS, num_nodes_pooling_layer=24, num_nodes_last_layer=16, num_steps_per_epoch=3, num_epochs=2,
                  learning_rate=0.05, reduce_lr_epochs=2, num_speakers_per_batch=2, num_segments_per_speaker=2, min_segment_len=20,
                  max_segment_len=24)
    spk_utts = [("s%d" % s, ["s%d-u%d" % (s, u) for u in range(2)]) for s in range(3)]
    data, spklist, _ = make_data_dir(tmp_path, spk_utts, {u: 30 for _, us in spk_utts for u in us}, dim=8)
    assert train.feature_dim(data, params) == 8 and train.feature_dim(data, dict(params, selected_dim=6)) == 6
    model = str(tmp_path / "model")
    with pytest.raises(RuntimeError, match="Cannot load checkpoint"):
        train.train(data, spklist, data, spklist, model, config=params, cont=True)
    model_io.save_model(model, params, 8, train.fresh_weights(params, 8, 3, seed=0, channels=8), step=3)
    with pytest.raises(FileNotFoundError) as e:
        train.train(data, spklist, data, spklist, model, cont=True)                     # the directory's own config.json
    assert os.path.join(model, "nnet", "optimizer-3.npz") in str(e.value) and "cold" in str(e.value)


def test_pruning_keeps_the_newest_pairs(tmp_path):
    from tf_kaldi_speaker_amd import train
    nnet = str(tmp_path)
    for step in (3, 6, 9, 12):
        np.savez(os.path.join(nnet, "model-%d.npz" % step), a=np.zeros(1))
        train.save_optimizer(nnet, step, {"num_steps": np.array(step)})
    train.prune_checkpoints(nnet, None)
    assert len(os.listdir(nnet)) == 8
    train.prune_checkpoints(nnet, 2)
    assert sorted(os.listdir(nnet)) == ["model-12.npz", "model-9.npz", "optimizer-12.npz", "optimizer-9.npz"]
    assert int(train.load_optimizer(nnet, 9)["num_steps"]) == 9
