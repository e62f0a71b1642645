"""Host side of the metric-learning loss heads: the float64 oracle (tests/helpers/ref_metric_loss.py) against the reference's
numpy twins (fixtures tests/golden/metric_*.npz, written by tests/golden/make_metric_loss_golden.py) and on the degenerate
cases the rules name, the end-to-end batch planner on a fake data directory with the expected batches written out by hand,
metric_losses.from_params, the build wiring and the argument errors of the Python layer.  No GPU."""
import ctypes
import glob
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_metric_loss as ref                                       # noqa: E402
from valid_data import make_data_dir                                # noqa: E402
from tf_kaldi_speaker_amd import metric_losses as ml, valid          # noqa: E402
from tf_kaldi_speaker_amd.params import Params                      # noqa: E402

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_*.npz")))


def golden_case(path):
    z = np.load(path)
    kind = str(z["kind"])
    if kind == "semihard":
        o = dict(margin=float(z["margin"]), squared=bool(z["squared"]), normalize=bool(z["normalize"]))
    elif kind in ("all", "hard"):
        m = float(z["margin"])
        o = dict(loss_type=str(z["loss_type"]), margin=int(m) if str(z["loss_type"]) == "asoftmax" else m)
    else:
        o = dict(w=float(z["w"]), b=float(z["b"]))
    return kind, z["x"], z["labels"], o, float(z["loss"])


def test_fixtures_cover_the_issue():
    names = {os.path.basename(p)[7:-4] for p in GOLDEN}
    want = {"semihard_sq0", "semihard_sq1", "ge2e_softmax_w20", "ge2e_softmax_w10", "ge2e_contrastive_w20", "ge2e_contrastive_w10"}
    want |= {"%s_%s" % (t, h) for t in ("all", "hard") for h in ("asoftmax_m1", "asoftmax_m2", "asoftmax_m4", "amsoftmax_m02",
                                                                   "arcsoftmax_m03")}
    assert names == {"%s_%s" % (n, o) for n in want for o in ("major", "perm")} and len(GOLDEN) == 32
    for p in GOLDEN:
        z = np.load(p)
        assert z["x"].dtype == np.float32 and z["x"].shape == (24, 16) and z["labels"].dtype == np.int32
        assert set(z["labels"].tolist()) == set(range(3, 42, 7))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[7:-4] for p in GOLDEN])
def test_oracle_matches_reference_twins(path):
    kind, x, labels, o, want = golden_case(path)
    r = ref.evaluate(kind, x, labels, **o)
    assert abs(r["loss"] - want) < 1e-12
    assert r["loss"] == np.cumsum(r["rows"])[-1] / (max(r["group_counts"][0], 1e-16) if kind != "all" else r["group_counts"][0] + 1e-16)
    tol_rows, tol_loss = ref.bounds(kind, x.shape[1], r, labels=labels, **o)
    assert tol_rows.shape == (24,) and 0.0 < tol_loss < 1e-9 and np.all(tol_rows > 0)


def test_order_changes_the_sum_only_by_rounding():
    by_name = {os.path.basename(p)[7:-4]: golden_case(p)[4] for p in GOLDEN}
    for name, loss in by_name.items():
        if name.endswith("_major"):
            assert abs(loss - by_name[name[:-6] + "_perm"]) < 1e-12


def test_oracle_ties_and_zeros():
    rs = np.random.RandomState(3)
    x = rs.standard_normal((7, 5)).astype(np.float32)
    labels = np.array([0, 0, 0, 1, 1, 2, 2])
    x[3] = x[1]                 # a negative of anchor 0 that is a bitwise copy of its positive 1
    x[2] = x[0]                 # two identical rows of one label
    x[6] = 0.0                  # an all-zero row
    r = ref.semihard(x, labels, 0.2)
    d = r["dist"]
    assert d[0, 3] == d[0, 1] and d[0, 2] == 0.0 and d[2, 0] == 0.0 and np.all(np.diag(d) == 0.0)
    # pair (0, 1): the copy at the same distance is NOT semi-hard, z is the least distance strictly above
    neg = d[0, labels != 0]
    above = neg[neg > d[0, 1]]
    assert above.size and d[0, 3] not in above
    a = ref.angular(x, labels, "asoftmax", 1, "all")
    assert a["cos"][0, 3] == a["cos"][0, 1]                      # t = c(0, 3) - pos(c(0, 1)) == 0 exactly: not active
    assert np.all(a["cos"][6] == 0.0) and np.all(np.isfinite(a["rows"]))
    g = ref.ge2e(x, np.array([0, 0, 0, 1, 1, 2, 3]), 20.0, 0.0, "softmax")
    assert g["sim"][5, 2] == 0.0 and g["sim"][6, 3] == 0.0        # classes of one row: e_i = 0
    assert np.all(np.isfinite(g["rows"]))
    with pytest.raises(NotImplementedError):
        ref.angular(x, labels, "asoftmax", 3, "all")
    # an anchor without a negative or without a positive contributes nothing
    one = ref.semihard(x[:3], np.array([5, 5, 5]), 0.2)
    assert one["group_counts"] == (0, 0) and one["loss"] == 0.0
    lone = ref.semihard(x[:3], np.array([5, 6, 7]), 0.2)
    assert lone["group_counts"] == (0, 0)
    hard = ref.angular(x[:3], np.array([5, 5, 5]), "additive_margin_softmax", 0.2, "hard")
    assert np.all(hard["rows"] == 0.0) and hard["group_counts"] == (3, 0)


def test_oracle_against_brute_force():
    """The vectorised mining of the oracle against the three nested loops of the rule."""
    rs = np.random.RandomState(8)
    x = rs.standard_normal((11, 4)).astype(np.float32)
    labels = np.array([4, 9, 4, 9, 9, 1, 4, 1, 9, 4, 1])
    for squared in (False, True):
        r = ref.semihard(x, labels, 0.3, squared)
        d, total, pairs = r["dist"], 0.0, 0
        for i in range(11):
            for j in range(11):
                if j == i or labels[j] != labels[i]:
                    continue
                neg = [d[i, k] for k in range(11) if labels[k] != labels[i]]
                semi = [v for v in neg if v > d[i, j]]
                total += max(0.3 + d[i, j] - (min(semi) if semi else max(neg)), 0.0)
                pairs += 1
        assert pairs == r["group_counts"][0] and abs(total / pairs - r["loss"]) < 1e-14
    r = ref.angular(x, labels, "additive_angular_margin_softmax", 0.3, "all")
    c, s, act, num = r["cos"], 0.0, 0, 0
    for i in range(11):
        for j in range(11):
            if j == i or labels[j] != labels[i]:
                continue
            for k in range(11):
                if labels[k] != labels[i]:
                    t = c[i, k] - ref.pos_value(c[i, j], "additive_angular_margin_softmax", 0.3)
                    s += max(t, 0.0)
                    act += t > 1e-12
                    num += 1
    assert r["group_counts"] == (act, num) and abs(s / (act + 1e-16) - r["loss"]) < 1e-14


# ------------------------------------------------------------------------------------------------ planner
def end2end_dir(tmp_path):
    # speakers out of order; s1's utterance c1 has exactly target_len frames: not eligible (strict); s3 has no eligible one
    spk_utts = [("s2", ["c0", "c1", "c2"]), ("s0", ["a0", "a1"]), ("s1", ["b0", "b1", "b2"]), ("s3", ["d0"])]
    lengths = {"c0": 50, "c1": 30, "c2": 31, "a0": 40, "a1": 45, "b0": 31, "b1": 29, "b2": 60, "d0": 30}
    return make_data_dir(tmp_path, spk_utts, lengths, spklist=[("s0", 0), ("s1", 1), ("s2", 2), ("s3", 3)])


def test_end2end_planner_wraps_speakers_and_utterances(tmp_path):
    data, spklist, _ = end2end_dir(tmp_path)
    plan = valid.plan_end2end_batches(data, spklist, num_speakers=2, num_segments=3, target_len=30)
    # eligible: s0 [a0 a1], s1 [b0 b2], s2 [c0 c2]; S = 3, ceil(3 / 2) = 2 batches: speakers (0, 1), (2, 0)
    assert [b.keys for b in plan] == [["a0", "a1", "a0", "b0", "b2", "b0"], ["c0", "c2", "c0", "a1", "a0", "a1"]]
    assert [list(b.labels) for b in plan] == [[0, 0, 0, 1, 1, 1], [2, 2, 2, 0, 0, 0]]
    assert all(b.length == 30 and b.labels.dtype == np.int32 for b in plan)
    assert [r.split(":")[0] for r in plan[0].rxfiles] == [os.path.join(data, "feats.ark")] * 6
    # max_iterations: the queue of the reference never ends
    plan5 = valid.plan_end2end_batches(data, spklist, 2, 3, 30, max_iterations=5)
    assert [b.keys for b in plan5[:2]] == [b.keys for b in plan]
    assert [sorted(set(b.labels.tolist())) for b in plan5] == [[0, 1], [0, 2], [1, 2], [0, 1], [0, 2]]
    # s1's second appearance (t = 1): utterances (3 + j) mod 2 -> b2 b0 b2
    assert plan5[2].keys[:3] == ["b2", "b0", "b2"]
    assert valid.plan_end2end_batches(data, spklist, 2, 3, 30, max_iterations=0) == []
    # deterministic
    again = valid.plan_end2end_batches(data, spklist, 2, 3, 30, max_iterations=5)
    assert [b.keys for b in again] == [b.keys for b in plan5]


def test_end2end_planner_eligibility_is_strict_and_needs_enough_speakers(tmp_path):
    data, spklist, _ = end2end_dir(tmp_path)
    plan = valid.plan_end2end_batches(data, spklist, 3, 1, 30)
    assert [b.keys for b in plan] == [["a0", "b0", "c0"]]
    with pytest.raises(ValueError):
        valid.plan_end2end_batches(data, spklist, 4, 1, 30)               # s3's only utterance has 30 frames, not more
    assert len(valid.plan_end2end_batches(data, spklist, 4, 1, 29)) == 1   # at 29 it is eligible
    plan = valid.plan_end2end_batches(data, spklist, 2, 2, 44)
    # more than 44 frames: s0 [a1], s1 [b2], s2 [c0]
    assert [b.keys for b in plan] == [["a1", "a1", "b2", "b2"], ["c0", "c0", "a1", "a1"]]
    with pytest.raises(ValueError):
        valid.plan_end2end_batches(data, spklist, 0, 1, 30)


# ------------------------------------------------------------------------------------------------ the Python layer
def test_from_params_switches_as_the_trainer_does(monkeypatch):
    calls = []
    monkeypatch.setattr(ml, "_run", lambda x, labels, offsets, kind, **kw: calls.append((kind, kw)) or "r")
    p = Params(loss_func="semihard_triplet_loss", margin=0.35, triplet_loss_squared=True)
    assert ml.from_params(p)("x", "l", [0, 2]) == "r"
    assert calls[-1][0] == 0 and calls[-1][1]["margin"] == 0.35 and calls[-1][1]["squared"] is True and calls[-1][1]["normalize"] is True
    p = Params(loss_func="angular_triplet_loss", margin=0.2, triplet_type="hard", loss_type="additive_margin_softmax")
    ml.from_params(p, validation=True)("x", "l")
    assert calls[-1][0] == 3 and (calls[-1][1]["w"], calls[-1][1]["b"]) == (20.0, 0.0)                # e2e_valid_loss
    ml.from_params(p, validation=False)("x", "l")
    assert calls[-1][0] == 2 and calls[-1][1]["pos_head"] == 2 and calls[-1][1]["margin"] == 0.2
    with pytest.raises(NotImplementedError, match="m=3 is not unsupported"):
        ml.from_params(Params(loss_func="angular_triplet_loss", margin=3, triplet_type="all", loss_type="asoftmax"), validation=False)
    for func in ("generalized_angular_triplet_loss", "ge2e", "softmax", "asoftmax", "nonsense"):
        with pytest.raises(NotImplementedError):
            ml.from_params(Params(loss_func=func))


def test_argument_errors_come_before_the_device():
    x = np.zeros((6, 4), np.float32)
    labels = np.array([0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError, match="fewer than two distinct labels"):
        ml.semihard_triplet_loss(x, np.zeros(6, np.int32))
    with pytest.raises(ValueError, match="fewer than two distinct labels"):
        ml.e2e_valid_loss(x, labels, offsets=[0, 2, 6])
    with pytest.raises(ValueError, match="labels"):
        ml.semihard_triplet_loss(x, labels[:5])
    with pytest.raises(ValueError, match="offsets"):
        ml.semihard_triplet_loss(x, labels, offsets=[0, 4, 4, 6])
    with pytest.raises(ValueError, match="loss_type"):
        ml.angular_triplet_loss(x, labels, loss_type="softmax")
    with pytest.raises(ValueError, match="triplet_type"):
        ml.angular_triplet_loss(x, labels, triplet_type="semihard")
    with pytest.raises(ValueError, match="ge2e_type"):
        ml.ge2e_loss(x, labels, ge2e_type="hinge")
    with pytest.raises(ValueError, match="at most 4096"):
        ml.semihard_triplet_loss(np.zeros((4097, 2), np.float32), np.arange(4097))
    with pytest.raises(NotImplementedError, match="m=3 is not unsupported"):
        ml.angular_triplet_loss(x, labels, loss_type="asoftmax", margin=3)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ml.semihard_triplet_loss(x, labels)


def test_metric_valid_keeps_the_reference_assertion(tmp_path):
    from tf_kaldi_speaker_amd import synth
    from tf_kaldi_speaker_amd.trainer import Trainer
    p = Params(**dict(synth.TDNN_STAT_PARAMS, loss_func="angular_triplet_loss", batch_type="end2end", min_segment_len=20,
                      max_segment_len=30))
    tr = Trainer(p, None, 30)
    with pytest.raises(AssertionError, match="Valid parameters should be set if E2E loss is selected"):
        valid.metric_valid(tr, "nowhere", "nothing", batch_type="end2end")
    with pytest.raises(NotImplementedError):
        valid.metric_valid(Trainer(Params(**synth.TDNN_STAT_PARAMS), None, 30), "nowhere", "nothing")
    with pytest.raises(NotImplementedError):
        tr.build("valid")                                              # the Trainer's own door stays shut
    assert valid.METRIC_LOSSES == ("semihard_triplet_loss", "angular_triplet_loss")


# ------------------------------------------------------------------------------------------------ build wiring
def test_exports_and_sources(repo_root):
    import __graft_entry__ as g
    from tf_kaldi_speaker_amd import _lib
    assert "metric_loss.hip" in g.SOURCES and os.path.isfile(os.path.join(g.CSRC, "metric_loss.hip"))
    g.build()
    hdr = open(os.path.join(repo_root, "include", "xvec_hip.h")).read()
    lib = _lib.load()
    m = re.search(r"enum \{ XV_METRIC_SEMIHARD = 0, XV_METRIC_ANGULAR_ALL = 1, XV_METRIC_ANGULAR_HARD = 2, XV_METRIC_GE2E_SOFTMAX = 3,\s*"
                  r"XV_METRIC_GE2E_CONTRASTIVE = 4 \};", hdr)
    assert m and (_lib.XV_METRIC_SEMIHARD, _lib.XV_METRIC_ANGULAR_ALL, _lib.XV_METRIC_ANGULAR_HARD, _lib.XV_METRIC_GE2E_SOFTMAX,
                  _lib.XV_METRIC_GE2E_CONTRASTIVE) == (0, 1, 2, 3, 4)
    # the size queries are pure host code: they answer without a device
    off = np.array([0, 640, 1280], dtype=np.int64)
    ptr = off.ctypes.data_as(ctypes.c_void_p)
    base = lib.xv_metric_loss_workspace(2, ptr, 512, 0)
    assert base > 0 and base % 256 == 0 and lib.xv_metric_loss_slot_bytes(640, 512, 0) == 0         # the panel fits LDS
    assert lib.xv_metric_loss_workspace(2, ptr, 512, 3) == base - 768 + 640 * (512 + 640) * 8          # no panel table (80 x 8 bytes), one slot
    assert lib.xv_metric_loss_slot_bytes(640, 512, 3) == 640 * (512 + 640) * 8                      # class sums and similarities
    assert lib.xv_metric_loss_slot_bytes(4096, 512, 1) == (128 * 4097 + 255) // 256 * 256
    assert lib.xv_metric_loss_workspace(0, None, 512, 0) == 0
    for args in ((2, ptr, 0, 0), (2, ptr, 4097, 0), (2, ptr, 512, 5), (2, ptr, 512, -1), (-1, ptr, 512, 0)):
        assert lib.xv_metric_loss_workspace(*args) == _lib.XV_ERR_INVALID, args
    for bad in ([0, 4097], [0, 5, 3], [-1, 4], [0, 0]):
        o = np.array(bad, dtype=np.int64)
        assert lib.xv_metric_loss_workspace(len(bad) - 1, o.ctypes.data_as(ctypes.c_void_p), 16, 0) == _lib.XV_ERR_INVALID, bad
