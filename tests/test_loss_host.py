"""Host side of the validation path: the float64 oracle of the loss heads against the reference's numpy twins (fixtures
tests/golden/loss_*.npz, written by tests/golden/make_loss_golden.py), the batch planner on a fake data directory with the
expected batches written out by hand, the validation parameter set, Trainer.build("valid") and the command line."""
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_loss                                                     # noqa: E402
from valid_data import make_data_dir                                # noqa: E402
from tf_kaldi_speaker_amd import losses, model_io, synth, valid      # noqa: E402
from tf_kaldi_speaker_amd.params import Params                      # noqa: E402

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_*.npz")))


def golden_case(path):
    z = np.load(path)
    fa = ref_loss.annealing_fa(z["lambda_min"], z["lambda_base"], z["lambda_gamma"], z["lambda_power"], int(z["global_step"]))
    x = z["x"]
    if int(z["feature_norm"]):
        x = ref_loss.l2_scaling(x, float(z["feature_scaling_factor"]))
    return dict(x=x, labels=z["labels"], kernel=z["kernel"], head=str(z["head"]), margin=float(z["margin"]), fa=fa,
                loss=float(z["loss"]), z=z)


def test_fixtures_cover_the_issue():
    names = {os.path.basename(p)[5:-4] for p in GOLDEN}
    assert names == {"asoftmax_m1", "asoftmax_m2", "asoftmax_m4", "amsoftmax_m0", "amsoftmax_m02", "arcsoftmax_m0", "arcsoftmax_m03",
                     "amsoftmax_norm"}
    steps = {int(np.load(p)["global_step"]) for p in GOLDEN}
    assert len(steps - {0}) >= 2


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[5:-4] for p in GOLDEN])
def test_oracle_matches_reference_twins(path):
    c = golden_case(path)
    r = ref_loss.classifier_loss(c["x"], c["labels"], c["kernel"], None, c["head"], c["margin"], c["fa"])
    assert abs(r["loss"].mean() - c["loss"]) < 1e-9
    if not (c["head"] == "asoftmax" and c["margin"] == 1):
        assert 0.0 < c["fa"] < 1.0


def test_oracle_matches_brute_force_softmax():
    rs = np.random.RandomState(0)
    x, w, b = rs.standard_normal((9, 13)), rs.standard_normal((13, 7)), rs.standard_normal(7)
    labels = rs.randint(0, 7, 9)
    r = ref_loss.classifier_loss(x, labels, w, b, "softmax")
    z = x @ w + b
    p = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    np.testing.assert_allclose(r["loss"], -np.log(p[np.arange(9), labels]), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(r["top1"], np.argmax(z, axis=1))
    # asoftmax m = 1 is the plain cross-entropy on x . W^ whatever fa says
    wh = w / np.linalg.norm(w, axis=0, keepdims=True)
    r1 = ref_loss.classifier_loss(x, labels, w, None, "asoftmax", 1, 0.7)
    r0 = ref_loss.classifier_loss(x, labels, wh, None, "softmax")
    np.testing.assert_allclose(r1["loss"], r0["loss"], rtol=0, atol=1e-12)
    with pytest.raises(NotImplementedError):
        ref_loss.classifier_loss(x, labels, w, None, "asoftmax", 3, 0.5)


# ------------------------------------------------------------------------------------------------ planner
def keys_of(plan):
    return [b.keys for b in plan]


def test_planner_fewer_utterances_than_a_batch(tmp_path):
    data, spklist, _ = make_data_dir(tmp_path, [("s0", ["a", "b"]), ("s1", ["c"])], {"a": 40, "b": 50, "c": 60})
    plan = valid.plan_batches(data, spklist, batch_size=4, target_len=30)
    # 3 utterances: sub-lists [a] and [b, c]; each 0 // 4 + 1 = 1 batch of min(4, len) utterances
    assert keys_of(plan) == [["a"], ["b", "c"]]
    assert [list(b.labels) for b in plan] == [[0], [0, 1]]
    assert [b.length for b in plan] == [30, 30]


def test_planner_two_batches_and_three_with_odd_split(tmp_path):
    # N = 2 B + 3 = 7 with B = 2; speakers out of order in feats.scp and in spklist: ascending speaker INDEX decides
    spk_utts = [("sB", ["b0", "b1", "b2"]), ("sA", ["a0", "a1"]), ("sC", ["c0", "c1"])]
    lengths = {u: 100 for _, us in spk_utts for u in us}
    data, spklist, _ = make_data_dir(tmp_path, spk_utts, lengths, spklist=[("sA", 0), ("sC", 1), ("sB", 2)])
    plan = valid.plan_batches(data, spklist, batch_size=2, target_len=25)
    # list: a0 a1 c0 c1 b0 b1 b2; 7 // 2 = 3 -> [a0 a1 c0] and [c1 b0 b1 b2]
    # first: 3 // 2 + 1 = 2 batches of 2, wrapped: (a0 a1) (c0 a0); second: 4 // 2 + 1 = 3 batches: (c1 b0) (b1 b2) (c1 b0)
    assert keys_of(plan) == [["a0", "a1"], ["c0", "a0"], ["c1", "b0"], ["b1", "b2"], ["c1", "b0"]]
    assert [list(b.labels) for b in plan] == [[0, 0], [1, 0], [1, 2], [2, 2], [1, 2]]
    assert all(b.length == 25 for b in plan)
    # valid_max_iterations cuts the walk
    assert keys_of(valid.plan_batches(data, spklist, 2, 25, max_iterations=3)) == [["a0", "a1"], ["c0", "a0"], ["c1", "b0"]]
    p = Params(num_speakers_per_batch=1, num_segments_per_speaker=2, min_segment_len=20, max_segment_len=31, valid_max_iterations=4)
    plan4 = valid.plan_for_params(data, spklist, p)
    assert len(plan4) == 4 and all(b.length == 25 for b in plan4)                      # (20 + 31) // 2


def test_planner_short_utterance_absent_speaker_and_width(tmp_path):
    spk_utts = [("s0", ["a", "b"]), ("s2", ["c", "d"])]
    data, spklist, mats = make_data_dir(tmp_path, spk_utts, {"a": 50, "b": 17, "c": 40, "d": 45}, dim=5,
                                        spklist=[("s0", 0), ("s1", 1), ("s2", 2)])     # s1 has no data
    plan = valid.plan_batches(data, spklist, batch_size=2, target_len=30)
    # [a b] [c d]; each 2 // 2 + 1 = 2 batches: (a b) (a b) (c d) (c d); b has 17 frames
    assert keys_of(plan) == [["a", "b"], ["a", "b"], ["c", "d"], ["c", "d"]]
    assert [b.length for b in plan] == [17, 17, 30, 30]
    assert [list(b.labels) for b in plan] == [[0, 0], [0, 0], [2, 2], [2, 2]]
    feats = valid.read_batch(plan[0], 5)
    assert feats.shape == (2, 17, 5) and feats.dtype == np.float32
    np.testing.assert_array_equal(feats[0], mats["a"][:17])
    np.testing.assert_array_equal(feats[1], mats["b"][:17])
    np.testing.assert_array_equal(valid.read_batch(plan[2], 3)[1], mats["d"][:30, :3])       # wider features are truncated
    with pytest.raises(ValueError):
        valid.read_batch(plan[2], 6)                                                         # narrower ones are an error
    # a speaker of the data that spklist does not name
    with open(spklist, "w") as f:
        f.write("s0 0\n")
    with pytest.raises(KeyError):
        valid.plan_batches(data, spklist, 2, 30)


# ------------------------------------------------------------------------------------------------ parameters
ANGULAR = dict(asoftmax_lambda_min=0.0, asoftmax_lambda_base=10.0, asoftmax_lambda_gamma=0.5, asoftmax_lambda_power=1.0,
               amsoftmax_lambda_min=0.0, amsoftmax_lambda_base=10.0, amsoftmax_lambda_gamma=0.5, amsoftmax_lambda_power=1.0,
               arcsoftmax_lambda_min=0.0, arcsoftmax_lambda_base=10.0, arcsoftmax_lambda_gamma=0.5, arcsoftmax_lambda_power=1.0,
               asoftmax_m=4, amsoftmax_m=0.25, arcsoftmax_m=0.3)


def test_validation_params_zero_the_margins_on_a_copy():
    for func, key, want in (("asoftmax", "asoftmax_m", 1), ("additive_margin_softmax", "amsoftmax_m", 0),
                            ("additive_angular_margin_softmax", "arcsoftmax_m", 0)):
        p = Params(loss_func=func, aux_loss_func=["ring_loss"], **ANGULAR)
        before = dict(p.dict)
        q = losses.valid_params(p)
        assert p.dict == before and q is not p
        assert q.dict[key] == want and q.dict["aux_loss_func"] == []
        name, _, margin, fa = losses.head_config(p, global_step=30, validation=True)
        assert p.dict == before and name == func and margin == float(want)
        if func == "asoftmax":
            assert fa == 0.0
        else:
            assert fa == pytest.approx(1.0 / (1.0 + 10.0 / 16.0))
        with pytest.raises(NotImplementedError):
            losses.head_config(p, global_step=30)                                      # aux_loss_func outside validation
    p = Params(loss_func="asoftmax", **dict(ANGULAR, asoftmax_m=3))
    with pytest.raises(NotImplementedError):
        losses.head_config(p)
    assert losses.head_config(Params(loss_func="additive_margin_softmax", **ANGULAR), global_step=200)[2:] == \
        (0.25, ref_loss.annealing_fa(0.0, 10.0, 0.5, 1.0, 200))


def test_build_valid_accepts_the_softmax_family_only():
    from tf_kaldi_speaker_amd.trainer import Trainer
    for func in ref_loss.HEADS:
        tr = Trainer(Params(**dict(synth.TDNN_STAT_PARAMS, loss_func=func, **ANGULAR)), None, 30)
        tr.build("valid")
        assert tr.embeddings == "output" and tr.is_valid_built
        with pytest.raises(NotImplementedError):
            tr.build("train")
        tr.build("predict")
        assert tr.embeddings == "tdnn6_dense"
    for func in ("semihard_triplet_loss", "angular_triplet_loss", "generalized_angular_triplet_loss", "ge2e"):
        with pytest.raises(NotImplementedError):
            Trainer(Params(**dict(synth.TDNN_STAT_PARAMS, loss_func=func)), None, 30).build("valid")
    with pytest.raises(NotImplementedError):
        Trainer(Params(**dict(synth.TDNN_STAT_PARAMS, batch_type="end2end")), None, 30).build("valid")
    tr = Trainer(Params(**synth.TDNN_STAT_PARAMS), None, 30)
    tr.build("valid")
    with pytest.raises(NotImplementedError):
        tr.valid("nowhere", "nothing", batch_type="end2end")
    with pytest.warns(UserWarning), pytest.raises(RuntimeError):
        tr.valid("nowhere", "nothing")                                                 # no checkpoint: warn and refuse


def test_loader_keeps_the_loss_layer(tmp_path):
    assert model_io._graph_variable("softmax/output/bias") and model_io._graph_variable("softmax/output/kernel")
    assert not model_io._graph_variable("softmax/output/kernel/Momentum")
    w = {"tdnn/tdnn1_conv/kernel": np.zeros((5, 3, 4), np.float32), "softmax/output/kernel": np.ones((4, 6), np.float32),
         "softmax/output/bias": np.arange(6, dtype=np.float32)}
    model_io.save_model(str(tmp_path), {}, 3, w, step=7)
    model_io.save_model(str(tmp_path), {}, 3, dict(w, **{"softmax/output/bias": np.zeros(6, np.float32)}), step=9)
    got, step = model_io.load_weights(os.path.join(str(tmp_path), "nnet"))
    assert step == 9 and not got["softmax/output/bias"].any()
    got, step = model_io.load_weights(os.path.join(str(tmp_path), "nnet"), name="model-7")
    assert step == 7
    np.testing.assert_array_equal(got["softmax/output/bias"], np.arange(6, dtype=np.float32))


def test_cli_arguments_and_line_formats():
    a = valid.build_parser().parse_args(["--gpu", "2", "--checkpoint", "model-5", "--precision", "f32", "--append", "m", "d", "s"])
    assert (a.gpu, a.checkpoint, a.precision, a.no_eer, a.append, a.model_dir, a.valid_dir, a.valid_spklist) == \
        (2, "model-5", "f32", False, True, "m", "d", "s")
    a = valid.build_parser().parse_args(["--no-eer", "m", "d", "s"])
    assert a.no_eer and not a.append and a.gpu == -1 and a.checkpoint == "" and a.precision == ""
    assert "1000" in valid.build_parser().format_help()
    assert valid.format_valid_loss(120000, 1.23456789, 0.0512345) == "120000 1.234568 0.051235\n"      # "%d %f %f\n", train.py:155
    assert valid.format_report(7, 2.5, 0.25, None) == "step 7 loss 2.500000 acc 0.250000 eer nan"
    with pytest.raises(SystemExit):
        valid.main(["--append", "--no-eer", "m", "d", "s"])
