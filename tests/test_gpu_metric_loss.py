"""The metric-learning loss heads on the GPU (csrc/metric_loss.hip) through the C ABI (xv_metric_loss) and through
tf_kaldi_speaker_amd.metric_losses, against the reference's numpy twins (tests/golden/metric_*.npz, |loss - twin| <= 1e-9) and
against the float64 oracle tests/helpers/ref_metric_loss.py under its bounds() (derived in the header of the kernel file):
rows within the bound, counts equal.  Then what a batched, deterministic kernel owes: edges of the tiles, padded rows, ties and
zeros, groups alone and in a batch bit for bit, the workspace, the limits, and validation end to end.

Every comparison prints the largest observed error as a fraction of its bound before it asserts.
Largest observed fraction of the bound on an MI355X: see profiles/valid.md."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_metric_loss as ref                                       # noqa: E402
from valid_data import make_data_dir                                # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_*.npz")))
KIND = {"semihard": 0, "all": 1, "hard": 2, "softmax": 3, "contrastive": 4}
HEAD = {"asoftmax": 1, "additive_margin_softmax": 2, "additive_angular_margin_softmax": 3}
SENTINEL = -7
# one set of options per kind, every positive-side head among them
OPTIONS = [("semihard", dict(margin=0.2, squared=False, normalize=True)),
           ("semihard", dict(margin=0.5, squared=True, normalize=False)),
           ("all", dict(loss_type="asoftmax", margin=4)),
           ("all", dict(loss_type="additive_angular_margin_softmax", margin=0.3)),
           ("hard", dict(loss_type="asoftmax", margin=2)),
           ("hard", dict(loss_type="additive_margin_softmax", margin=0.2)),
           ("softmax", dict(w=20.0, b=0.0)),
           ("contrastive", dict(w=10.0, b=-5.0))]


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


def abi(x, labels, offsets, kind, o, ldx=None, ws_factor=1, ws_bytes_delta=0, want_top1=True):
    """One xv_metric_loss call on rows padded to `ldx` with NaN behind every row and after the last ->
    dict(rc, need, loss [G], rows, counts, top1, gcounts); the outputs are prefilled with SENTINEL."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    ldx = ldx or d
    host = np.full(n * ldx + 5, np.nan, dtype=np.float32)
    host[:n * ldx].reshape(n, ldx)[:, :d] = x
    xd = torch.from_numpy(host).cuda()
    ld = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    groups = len(off) - 1
    ptr = off.ctypes.data_as(C.c_void_p)
    need = int(lib.xv_metric_loss_workspace(groups, ptr, d, KIND.get(kind, kind)))
    ws = torch.empty(max(need, 0) * ws_factor + 64, dtype=torch.uint8, device="cuda")
    rows = torch.full((n,), float(SENTINEL), dtype=torch.float64, device="cuda")
    counts = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    top1 = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    gloss = torch.full((max(groups, 1),), float(SENTINEL), dtype=torch.float64, device="cuda")
    gcount = torch.full((max(groups, 1), 2), SENTINEL, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    rc = lib.xv_metric_loss(0, p(xd), ldx, ptr, groups, d, p(ld), KIND.get(kind, kind), HEAD.get(o.get("loss_type"), 0),
                            float(o.get("margin", 0.0)), int(o.get("squared", False)), int(o.get("normalize", True)),
                            float(o.get("w", 0.0)), float(o.get("b", 0.0)), p(rows), p(counts), p(top1) if want_top1 else None,
                            p(gloss), p(gcount), p(ws), max(need, 0) * ws_factor + ws_bytes_delta,
                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return dict(rc=rc, need=need, loss=gloss.cpu().numpy(), rows=rows.cpu().numpy(), counts=counts.cpu().numpy(),
                top1=top1.cpu().numpy(), gcounts=gcount.cpu().numpy())


def check_group(tag, kind, o, x, labels, got_rows, got_counts, got_loss, got_gcounts, got_top1=None):
    """One group against the oracle: counts equal, rows and loss within bounds(); prints the observed fractions."""
    r = ref.evaluate(kind, x, labels, **o)
    # a comparison within rounding of a tie could fall either way: a condition on the inputs (four orders over the bounds)
    if kind == "semihard":
        assert r["min_gap"] > 1e-11, "the inputs hold a near-tie (%g): the semi-hard choice is not stable" % r["min_gap"]
    if kind == "all":
        assert r["min_abs_t"] == 0.0 or r["min_abs_t"] > 1e-10
    tol_rows, tol_loss = ref.bounds(kind, x.shape[1], r, labels=labels, **o)
    err_rows, err_loss = np.abs(got_rows - r["rows"]), abs(got_loss - r["loss"])
    with np.errstate(divide="ignore", invalid="ignore"):          # no term, no tolerance: the row must be exact
        frac_rows = float(np.max(np.where(err_rows == 0.0, 0.0, err_rows / tol_rows)))
        frac_loss = 0.0 if err_loss == 0.0 else float(np.float64(err_loss) / tol_loss)
    print("%s %s %s B=%d d=%d: error/bound rows %.3f loss %.3f (loss %.12g)" % (tag, kind, o, len(labels), x.shape[1], frac_rows, frac_loss, got_loss))
    np.testing.assert_array_equal(got_counts, r["counts"])
    assert tuple(int(v) for v in got_gcounts) == tuple(r["group_counts"])
    if got_top1 is not None and kind in ("softmax", "contrastive"):
        np.testing.assert_array_equal(got_top1, r["top1"])
    assert frac_rows <= 1.0 and frac_loss <= 1.0
    return r


def make_group(rs, b, d, classes=None, spread=0.8):
    """Rows round class centres, every class present (b >= classes), labels any int32."""
    classes = classes or max(2, min(b // 3, 9))
    values = np.array([-2147483648, 2147483647, -7, 0, 41, 1 << 30, -(1 << 20), 5, 99][:classes] if classes <= 9
                      else rs.permutation(np.unique(rs.randint(-(1 << 30), 1 << 30, 4 * classes)))[:classes])
    cls = np.concatenate([np.arange(classes), rs.randint(0, classes, b - classes)])
    rs.shuffle(cls)
    centres = rs.standard_normal((classes, d))
    x = centres[cls] * spread + rs.standard_normal((b, d))
    return x.astype(np.float32), values[cls].astype(np.int32)


# ------------------------------------------------------------------------------------------------ 1. pinned
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[7:-4] for p in GOLDEN])
def test_pinned_to_the_reference_twins(path):
    from tf_kaldi_speaker_amd import metric_losses as ml
    kind, x, labels, o, want = golden_case(path)
    g = abi(x, labels, [0, 24], kind, o)
    assert g["rc"] == 0
    if kind == "semihard":
        m = ml.semihard_triplet_loss(x, labels, **o)
    elif kind in ("all", "hard"):
        m = ml.angular_triplet_loss(x, labels, triplet_type=kind, **o)
    else:
        m = ml.ge2e_loss(x, labels, ge2e_type=kind, **o)
    print("%s: |loss - twin| C ABI %.3g, metric_losses %.3g (allowed 1e-9)" % (os.path.basename(path), abs(g["loss"][0] - want), abs(m.loss - want)))
    assert abs(g["loss"][0] - want) <= 1e-9 and abs(m.loss - want) <= 1e-9
    check_group("golden", kind, o, x, labels, g["rows"], g["counts"], g["loss"][0], g["gcounts"][0], g["top1"])
    np.testing.assert_array_equal(m.rows, g["rows"])
    np.testing.assert_array_equal(m.counts, g["counts"])
    np.testing.assert_array_equal(m.group_counts, g["gcounts"])
    assert m.group_loss[0] == g["loss"][0] and m.loss == g["loss"][0]
    if kind in ("softmax", "contrastive"):
        np.testing.assert_array_equal(m.top1, g["top1"])
    else:
        assert m.top1 is None and np.all(g["top1"] == SENTINEL)


def test_e2e_valid_loss_and_many_batches_in_one_call():
    from tf_kaldi_speaker_amd import metric_losses as ml
    import torch
    kind, x, labels, o, want = golden_case([p for p in GOLDEN if p.endswith("ge2e_softmax_w20_major.npz")][0])
    assert abs(ml.e2e_valid_loss(x, labels).loss - want) <= 1e-9
    kind2, x2, labels2, _, want2 = golden_case([p for p in GOLDEN if p.endswith("ge2e_softmax_w20_perm.npz")][0])
    r = ml.e2e_valid_loss(torch.from_numpy(np.concatenate([x, x2[:12]])).cuda(), np.concatenate([labels, labels2[:12]]),
                          offsets=[0, 24, 36], as_tensor=True)
    assert r.rows.is_cuda and r.group_loss.shape == (2,) and abs(float(r.group_loss[0]) - want) <= 1e-9
    assert r.loss == float(np.mean(r.group_loss.cpu().numpy()))
    assert r.group_counts.cpu().numpy()[:, 0].tolist() == [24, 12]


# ------------------------------------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("d,b,ldx", [(1, 2, 1), (3, 3, 5), (17, 15, 17), (130, 16, 131), (3, 17, 8), (17, 33, 19), (130, 257, 130)])
def test_edges_of_tiles_and_padded_rows(d, b, ldx):
    rs = np.random.RandomState(1000 * d + b)
    x, labels = make_group(rs, b, d)
    if d == 1:
        x = np.array([[1.5], [-0.25]], dtype=np.float32)
    for kind, o in OPTIONS:
        if d == 1 and kind in ("all", "hard") and o["loss_type"] == "additive_angular_margin_softmax":
            continue                                  # |c| = 1 off the diagonal: the arc head has no slope there
        g = abi(x, labels, [0, b], kind, o, ldx=ldx)
        assert g["rc"] == 0
        check_group("edge", kind, o, x, labels, g["rows"], g["counts"], g["loss"][0], g["gcounts"][0], g["top1"])


# ------------------------------------------------------------------------------------------------ 3. ties and zeros
def test_ties_and_zeros():
    rs = np.random.RandomState(3)
    x = rs.standard_normal((7, 5)).astype(np.float32)
    labels = np.array([0, 0, 0, 1, 1, 2, 2], dtype=np.int32)
    x[3] = x[1]                 # a negative of anchor 0 that is a bitwise copy of its positive 1
    x[2] = x[0]                 # two identical rows of one label
    x[6] = 0.0                  # an all-zero row
    for kind, o in OPTIONS:
        lab = np.array([0, 0, 0, 1, 1, 2, 3], dtype=np.int32) if kind in ("softmax", "contrastive") else labels
        g = abi(x, lab, [0, 7], kind, o)
        assert g["rc"] == 0 and np.all(np.isfinite(g["rows"]))
        r = check_group("ties", kind, o, x, lab, g["rows"], g["counts"], g["loss"][0], g["gcounts"][0], g["top1"])
        if kind == "semihard" and o["squared"] is False:
            # anchor 0 with positive 2 (an identical row): d = 0 exactly, so the term is max(margin - z, 0) with z the nearest negative
            assert r["dist"][0, 2] == 0.0
    # the copy is not semi-hard for (0, 1): were d(0, 3) taken as > d(0, 1), z would be d(0, 1) itself and the term the margin
    o = dict(margin=0.2, squared=True, normalize=True)
    r = ref.semihard(x, labels, **o)
    g = abi(x, labels, [0, 7], "semihard", o)
    d = r["dist"]
    neg = d[0, labels != 0]
    z = neg[neg > d[0, 1]].min()
    pair_02 = max(0.2 + 0.0 - neg[neg > 0.0].min(), 0.0)
    want = max(0.2 + d[0, 1] - z, 0.0) + pair_02
    assert abs(g["rows"][0] - want) <= ref.bounds("semihard", 5, r, **o)[0][0] and abs(want - (0.2 + pair_02)) > 1e-3
    # asoftmax m = 1, "all": t = c(0, 3) - c(0, 1) is exactly 0 for the copy: not active, on the GPU as in the oracle
    o = dict(loss_type="asoftmax", margin=1)
    g = abi(x, labels, [0, 7], "all", o)
    r = ref.angular(x, labels, "asoftmax", 1, "all")
    assert g["counts"][0] == r["counts"][0] and tuple(g["gcounts"][0]) == r["group_counts"]
    # a class of one row: similarity 0, z = b, on both sides
    g = abi(x, np.array([0, 0, 0, 1, 1, 2, 3], dtype=np.int32), [0, 7], "softmax", dict(w=20.0, b=0.0))
    r = ref.ge2e(x, np.array([0, 0, 0, 1, 1, 2, 3]), 20.0, 0.0, "softmax")
    assert r["sim"][5, 2] == 0.0 and abs(g["rows"][5] - r["rows"][5]) <= 40.0 * 13 * ref.UNIT


# ------------------------------------------------------------------------------------------------ 4. batches
def test_groups_alone_in_a_batch_and_in_any_order_are_the_same_bits():
    rs = np.random.RandomState(44)
    sizes, d = (2, 17, 64, 3, 300), 24
    groups = [make_group(rs, b, d) for b in sizes]
    order = [3, 0, 4, 2, 1]

    def packed(idx):
        return (np.concatenate([groups[i][0] for i in idx]), np.concatenate([groups[i][1] for i in idx]),
                np.concatenate([[0], np.cumsum([sizes[i] for i in idx])]))

    for kind, o in OPTIONS[::2] + [OPTIONS[5], OPTIONS[7]]:
        x, labels, off = packed(range(5))
        g = abi(x, labels, off, kind, o)
        assert g["rc"] == 0
        again = abi(x, labels, off, kind, o)
        wide = abi(x, labels, off, kind, o, ws_factor=2)
        xp, lp, offp = packed(order)
        perm = abi(xp, lp, offp, kind, o)
        for key in ("loss", "rows", "counts", "gcounts", "top1"):
            np.testing.assert_array_equal(g[key], again[key])
            np.testing.assert_array_equal(g[key], wide[key])
        for pos, i in enumerate(order):
            np.testing.assert_array_equal(perm["rows"][offp[pos]:offp[pos + 1]], g["rows"][off[i]:off[i + 1]])
            np.testing.assert_array_equal(perm["counts"][offp[pos]:offp[pos + 1]], g["counts"][off[i]:off[i + 1]])
            assert perm["loss"][pos] == g["loss"][i] and perm["gcounts"][pos].tolist() == g["gcounts"][i].tolist()
        for i, (gx, gl) in enumerate(groups):
            alone = abi(gx, gl, [0, sizes[i]], kind, o)
            np.testing.assert_array_equal(alone["rows"], g["rows"][off[i]:off[i + 1]])
            np.testing.assert_array_equal(alone["counts"], g["counts"][off[i]:off[i + 1]])
            np.testing.assert_array_equal(alone["top1"], g["top1"][off[i]:off[i + 1]])
            assert alone["loss"][0] == g["loss"][i] and alone["gcounts"][0].tolist() == g["gcounts"][i].tolist()
            # the group sum is the sequential double sum of the rows in row order
            total = np.cumsum(g["rows"][off[i]:off[i + 1]])[-1]
            cnt = float(g["gcounts"][i, 0])
            want = total / max(cnt, 1e-16) if kind == "semihard" else total / (cnt + 1e-16) if kind == "all" else total / sizes[i]
            assert g["loss"][i] == want
        # one byte short: refused, nothing written
        short = abi(x, labels, off, kind, o, ws_bytes_delta=-1)
        from tf_kaldi_speaker_amd import _lib
        assert short["rc"] == _lib.XV_ERR_WORKSPACE
        assert np.all(short["rows"] == SENTINEL) and np.all(short["counts"] == SENTINEL) and np.all(short["loss"] == SENTINEL)
        assert np.all(short["gcounts"] == SENTINEL) and np.all(short["top1"] == SENTINEL)
        # without row_top1 the rest is the same
        bare = abi(x, labels, off, kind, o, want_top1=False)
        np.testing.assert_array_equal(bare["rows"], g["rows"])
        np.testing.assert_array_equal(bare["gcounts"], g["gcounts"])
    # the largest group of the batch against the oracle, once per kind of kernel
    i = 4
    for kind, o in (OPTIONS[0], OPTIONS[3], OPTIONS[6]):
        x, labels, off = packed(range(5))
        g = abi(x, labels, off, kind, o)
        s = slice(off[i], off[i + 1])
        check_group("batch", kind, o, groups[i][0], groups[i][1], g["rows"][s], g["counts"][s], g["loss"][i], g["gcounts"][i], g["top1"][s])


def test_a_group_over_the_lds_panel_goes_through_the_workspace():
    """Groups over 1024 rows keep their 16-anchor panels in slots of the workspace: the least workspace is one slot (one
    workgroup walks all panels), a larger one runs more at a time, and the bits are the same."""
    rs = np.random.RandomState(77)
    b, d = 1025, 4
    x, labels = make_group(rs, b, d, classes=40, spread=2.0)
    small = np.concatenate([x, x[:33]]), np.concatenate([labels, labels[:33]]), [0, b, b + 33]
    for kind, o in (OPTIONS[0], OPTIONS[2]):
        g = abi(small[0], small[1], small[2], kind, o)
        wide = abi(small[0], small[1], small[2], kind, o, ws_factor=8)
        assert g["rc"] == 0 and wide["rc"] == 0
        for key in ("loss", "rows", "counts", "gcounts"):
            np.testing.assert_array_equal(g[key], wide[key])
        # the small group of this batch took the workspace path too: the same bits as alone, where its panel sits in LDS
        alone = abi(x[:33], labels[:33], [0, 33], kind, o)
        np.testing.assert_array_equal(alone["rows"], g["rows"][b:])
        assert alone["loss"][0] == g["loss"][1]
        check_group("ws-panel", kind, o, x, labels, g["rows"][:b], g["counts"][:b], g["loss"][0], g["gcounts"][0])


# ------------------------------------------------------------------------------------------------ 5. worst mining case
def test_two_labels_of_300_rows():
    rs = np.random.RandomState(9)
    d = 64
    cls = np.repeat([0, 1], 300)
    rs.shuffle(cls)
    x = (rs.standard_normal((2, d))[cls] * 0.5 + rs.standard_normal((600, d))).astype(np.float32)
    labels = np.array([-5, 12], dtype=np.int32)[cls]
    for kind, o in (OPTIONS[0], OPTIONS[2], OPTIONS[5], OPTIONS[6], OPTIONS[7]):
        g = abi(x, labels, [0, 600], kind, o)
        assert g["rc"] == 0
        check_group("2x300", kind, o, x, labels, g["rows"], g["counts"], g["loss"][0], g["gcounts"][0], g["top1"])
        if kind == "all":
            assert g["gcounts"][0, 1] == 600 * 299 * 300


# ------------------------------------------------------------------------------------------------ 6. limits
def test_limits_and_errors():
    from tf_kaldi_speaker_amd import _lib
    x = np.zeros((4097, 2), dtype=np.float32)
    labels = np.arange(4097, dtype=np.int32) % 3
    o = dict(margin=0.2)
    assert abi(x, labels, [0, 4097], "semihard", o)["rc"] == _lib.XV_ERR_INVALID
    assert abi(x, labels, [0, 9, 5], "semihard", o)["rc"] == _lib.XV_ERR_INVALID
    assert abi(x, labels, [0, 5], 7, o)["rc"] == _lib.XV_ERR_INVALID
    assert abi(x, labels, [0, 5], -1, o)["rc"] == _lib.XV_ERR_INVALID
    assert abi(x, labels, [0, 5], "all", dict(loss_type="nothing", margin=0.2))["rc"] == _lib.XV_ERR_INVALID
    r = abi(x, labels, [0, 5], "all", dict(loss_type="asoftmax", margin=3))
    assert r["rc"] == _lib.XV_ERR_UNSUPPORTED and np.all(r["rows"] == SENTINEL)
    assert abi(x, labels, [0, 5], "semihard", dict(margin=float("nan")))["rc"] == _lib.XV_ERR_INVALID
    r = abi(x, labels, [0], "semihard", o)
    assert r["rc"] == _lib.XV_OK and np.all(r["rows"] == SENTINEL) and np.all(r["loss"] == SENTINEL)
    # d = 0 cannot be laid out as an array: straight through the library
    import torch
    lib = _lib.load()
    off = np.array([0, 5], dtype=np.int64)
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    for d in (0, 4097):
        rc = lib.xv_metric_loss(0, p, 8, off.ctypes.data_as(C.c_void_p), 1, d, p, 0, 0, 0.2, 0, 1, 0.0, 0.0, p, p, None, p, p, p, 512, None)
        assert rc == _lib.XV_ERR_INVALID
    assert b"1 <= d <= 4096" in lib.xv_last_error(None)
    # a legal group of 4096 rows
    x, labels = make_group(np.random.RandomState(2), 4096, 2, classes=8)
    g = abi(x, labels, [0, 4096], "hard", dict(loss_type="additive_margin_softmax", margin=0.2))
    assert g["rc"] == 0 and np.all(g["counts"] == 1) and g["gcounts"][0].tolist() == [4096, 0] and np.all(np.isfinite(g["rows"]))
    c = np.clip(ref.l2_scaling(x) @ ref.l2_scaling(x).T, -1, 1)
    same = labels[:, None] == labels[None, :]
    want = np.maximum(np.where(same, -np.inf, c).max(axis=1) - (np.where(same, c, np.inf).min(axis=1) - 0.2), 0.0)
    assert np.max(np.abs(g["rows"] - want)) <= 2 * (2 * 10 * ref.UNIT)            # both sides within (1 + slope) (d + 8) 2^-53


# ------------------------------------------------------------------------------------------------ 7. end to end
def e2e_setup(tmp_path, loss_func, **extra):
    from tf_kaldi_speaker_amd import model_io, synth
    params = dict(synth.TDNN_STAT_PARAMS, loss_func=loss_func, num_speakers_per_batch=4, num_segments_per_speaker=3,
                  min_segment_len=35, max_segment_len=45, num_nodes_pooling_layer=24, num_nodes_last_layer=16, **extra)
    weights = synth.synth_weights(params, 30, seed=4, channels=8)
    model_dir = str(tmp_path / "exp")
    model_io.save_model(model_dir, params, 30, weights, step=4321)
    rs = np.random.RandomState(21)
    spk_utts = [("spk%d" % s, ["spk%d-u%d" % (s, u) for u in range(3)]) for s in (3, 0, 5, 1, 4, 2)]
    lens = {u: int(t) for (_, us) in spk_utts for u, t in zip(us, rs.randint(36, 61, 3))}
    lens["spk5-u0"] = 40                                                       # exactly the segment length: not eligible
    data, spklist, _ = make_data_dir(tmp_path, spk_utts, lens, dim=32, spklist=[("spk%d" % s, s) for s in range(7)], seed=22)
    return params, model_dir, data, spklist


@pytest.mark.parametrize("loss_func", ["angular_triplet_loss", "semihard_triplet_loss"])
def test_valid_command_end_to_end(tmp_path, capsys, loss_func):
    from tf_kaldi_speaker_amd import valid
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    if loss_func == "angular_triplet_loss":
        extra = dict(batch_type="end2end", num_valid_speakers_per_batch=4, num_valid_segments_per_speaker=3, margin=0.2,
                     triplet_type="all", loss_type="additive_margin_softmax", valid_max_iterations=3)
    else:
        extra = dict(margin=0.3, triplet_loss_squared=False)
    params, model_dir, data, spklist = e2e_setup(tmp_path, loss_func, **extra)
    assert valid.main(["--gpu", "0", "--precision", "f32", "--append", model_dir, data, spklist]) == 0
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step ")]
    assert len(line) == 1
    f = line[0].split()
    assert f[0::2] == ["step", "loss", "acc", "eer"] and int(f[1]) == 4321
    # the oracle on the embeddings metric_valid returns
    tr = Trainer(Params(**params), model_dir, 30, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    batch_type = params.get("batch_type", "softmax")
    loss, emb, labels = valid.metric_valid(tr, data, spklist, batch_type=batch_type, output_embeddings=True)
    n_batches, acc = tr.valid_num_batches, tr.valid_accuracy
    tr.close()
    if loss_func == "angular_triplet_loss":
        assert n_batches == 3 and emb.shape == (36, 16)
        assert labels.reshape(3, 4, 3)[0].tolist() == [[0] * 3, [1] * 3, [2] * 3, [3] * 3]          # speaker-major
        kind, o = "softmax", dict(w=20.0, b=0.0)
        assert 0.0 <= acc <= 1.0 and abs(float(f[5]) - acc) <= 1e-6
    else:
        assert n_batches == 2 and emb.shape == (18, 16)
        kind, o = "semihard", dict(margin=0.3, squared=False, normalize=True)
        assert np.isnan(acc) and f[5] == "nan"
    per = emb.shape[0] // n_batches
    want, tol = [], []
    for b in range(n_batches):
        s = slice(b * per, (b + 1) * per)
        r = ref.evaluate(kind, emb[s], labels[s], **o)
        want.append(r["loss"])
        tol.append(ref.bounds(kind, 16, r, labels=labels[s], **o)[1])
    want, tol = float(np.mean(want)), float(np.mean(tol))
    print("valid %s: loss %.12g oracle %.12g, error/bound %.3f" % (loss_func, loss, want, abs(loss - want) / tol))
    assert abs(loss - want) <= tol
    assert abs(float(f[3]) - want) <= tol + 1e-6                                     # %f prints six decimals
    with open(os.path.join(model_dir, "nnet", "valid_loss")) as fh:
        assert fh.read() == "%d %s %s\n" % (4321, f[3], f[7])
    with pytest.raises(NotImplementedError):
        Trainer(Params(**params), model_dir, 30, single_cpu=True, device=0).build("valid")
