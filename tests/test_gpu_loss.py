"""GPU: the fused classifier-head loss (csrc/loss.hip) through the C ABI against the float64 oracle tests/helpers/ref_loss.py,
and Trainer.valid / the valid command line end to end.

Tolerances come from the bound derived in the header of csrc/loss.hip and restated in ref_loss.bounds: per logit
(E + 8) 2^-24 ||x_i|| max_c ||w_c|| (+ |b| 2^-24); the target logit that bound times max(1, fs + fa |phi'|); the log-sum-exp the
same plus k(C) 2^-24 (1 + |lse_i|); the loss their sum (twice the logit bound plus the k term where no margin acts).
Every test prints the largest observed error as a fraction of its bound before it asserts.

Largest observed fraction of the bound on an MI355X: see profiles/valid.md."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_loss                                                     # noqa: E402
from valid_data import make_data_dir                                # noqa: E402

pytestmark = pytest.mark.gpu

HEAD_ID = {"softmax": 0, "asoftmax": 1, "additive_margin_softmax": 2, "additive_angular_margin_softmax": 3}
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_*.npz")))


def _p(t):
    return C.c_void_p(t.data_ptr())


def prepare(kernel, head):
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    e, c = kernel.shape
    ldc = (e + 3) // 4 * 4
    kd = torch.from_numpy(np.ascontiguousarray(kernel, dtype=np.float32)).cuda()
    classes = torch.zeros((c, ldc), dtype=torch.float32, device="cuda")
    _lib.check(lib.xv_loss_prepare_classes(0, _p(kd), c, e, c, int(head != "softmax"), _p(classes), ldc, None))
    return classes, ldc


def raw_call(x, labels, classes, ldc, num_classes, bias, head, margin, fa, ws_bytes=None, fill=None):
    """xv_loss_classifier on float32 / int32 arrays -> (rc, dict of outputs as numpy)."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    n, e = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    ld = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    bd = None if bias is None else torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float32)).cuda()
    out = torch.full((3, n), float("nan") if fill is None else fill, dtype=torch.float32, device="cuda")
    top1 = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    need = int(lib.xv_loss_workspace(n, num_classes))
    ws = torch.empty(need if ws_bytes is None else ws_bytes, dtype=torch.uint8, device="cuda")
    rc = lib.xv_loss_classifier(0, _p(xd), e, n, e, _p(ld), _p(classes), ldc, num_classes, None if bd is None else _p(bd),
                                HEAD_ID[head], float(margin), float(fa), _p(out[0]), _p(out[1]), _p(out[2]), _p(top1), _p(ws),
                                ws.numel(), None)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return rc, dict(loss=o[0], target_logit=o[1], lse=o[2], top1=top1.cpu().numpy())


def run(x, labels, kernel, bias, head, margin, fa):
    from tf_kaldi_speaker_amd import _lib
    classes, ldc = prepare(kernel, head)
    rc, got = raw_call(x, labels, classes, ldc, kernel.shape[1], bias, head, margin, fa)
    _lib.check(rc)
    return got


def f32(a):
    return np.asarray(a, dtype=np.float32)


def check(got, x, labels, kernel, bias, head, margin, fa, what):
    """Compare with the oracle on the float32 inputs the kernel saw; -> the largest error / bound."""
    e, c = kernel.shape
    ref = ref_loss.classifier_loss(f32(x).astype(np.float64), labels, f32(kernel).astype(np.float64),
                                   None if bias is None else f32(bias).astype(np.float64), head, margin, fa)
    bt, bl, bs = ref_loss.bounds(ref, e, c)
    # the float32 result itself is rounded once more
    half_ulp = lambda v: ref_loss.U * np.abs(v)                                       # noqa: E731
    fr = {}
    for name, b in (("target_logit", bt), ("lse", bl), ("loss", bs)):
        err = np.abs(got[name].astype(np.float64) - ref[name])
        fr[name] = float(np.max(err / (b + half_ulp(ref[name]) + 1e-300)))
    print("%s: n=%d C=%d E=%d %s m=%g fa=%.3f  error/bound target %.3f lse %.3f loss %.3f"
          % (what, len(labels), c, e, head, margin, fa, fr["target_logit"], fr["lse"], fr["loss"]))
    assert np.all(np.isfinite(got["loss"]))
    assert fr["target_logit"] <= 1.0 and fr["lse"] <= 1.0 and fr["loss"] <= 1.0, fr
    # top-1: the class of the largest logit before the margin, wherever the runner-up is further away than the logit bound
    z = f32(x).astype(np.float64) @ (f32(kernel).astype(np.float64) if head == "softmax" else
                                     f32(kernel).astype(np.float64) / np.sqrt(np.maximum(np.sum(f32(kernel).astype(np.float64) ** 2, axis=0, keepdims=True), 1e-12)))
    if bias is not None:
        z = z + f32(bias).astype(np.float64)
    if c > 1:
        part = np.partition(z, -2, axis=1)
        clear = (part[:, -1] - part[:, -2]) > 2.0 * (e + 8) * ref_loss.U * ref["xnorm"] * ref["wnorm_max"] + 2.0 * ref["bias_abs_max"] * ref_loss.U
        np.testing.assert_array_equal(got["top1"][clear], ref["top1"][clear])
        assert clear.mean() > 0.5
    assert np.all((got["top1"] >= 0) & (got["top1"] < c))
    return max(fr.values())


def edge_labels(rs, n, c):
    want = [0, c - 1, min(127, c - 1), min(128, c - 1)]
    labels = rs.randint(0, c, n)
    if n == 1:
        labels[0] = c - 1
    else:
        labels[:min(n, 4)] = want[:min(n, 4)]
    return labels.astype(np.int32)


EDGES = [(1, 3, 7), (1, 129, 130), (5, 127, 32), (5, 128, 33), (5, 129, 7), (5, 300, 130), (129, 3, 33), (129, 127, 7),
         (129, 128, 130), (129, 129, 32), (129, 300, 33)]


@pytest.mark.parametrize("n,c,e", EDGES)
def test_edges(n, c, e):
    rs = np.random.RandomState(1000 * n + 10 * c + e)
    x = rs.standard_normal((n, e)) * rs.uniform(0.5, 3.0, (n, 1))
    w = rs.standard_normal((e, c)) * rs.uniform(0.2, 2.0, (1, c))
    b = rs.standard_normal(c)
    labels = edge_labels(rs, n, c)
    check(run(x, labels, w, b, "softmax", 0.0, 0.0), x, labels, w, b, "softmax", 0.0, 0.0, "edges")
    check(run(x, labels, w, None, "softmax", 0.0, 0.0), x, labels, w, None, "softmax", 0.0, 0.0, "edges")
    for head, m, fa in (("asoftmax", 1, 0.0), ("asoftmax", 2, 0.6), ("asoftmax", 4, 0.3), ("additive_margin_softmax", 0.25, 0.8),
                        ("additive_angular_margin_softmax", 0.3, 0.5)):
        check(run(x, labels, w, None, head, m, fa), x, labels, w, None, head, m, fa, "edges")


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[5:-4] for p in GOLDEN])
def test_golden_cases_and_neighbours(path):
    z = np.load(path)
    head, margin, step = str(z["head"]), float(z["margin"]), int(z["global_step"])
    x = ref_loss.l2_scaling(z["x"], float(z["feature_scaling_factor"])) if int(z["feature_norm"]) else z["x"]
    lam = [float(z[k]) for k in ("lambda_min", "lambda_base", "lambda_gamma", "lambda_power")]
    fa = ref_loss.annealing_fa(lam[0], lam[1], lam[2], lam[3], step)
    got = run(x, z["labels"], z["kernel"], None, head, margin, fa)
    check(got, x, z["labels"], z["kernel"], None, head, margin, fa, "golden")
    # the fixture's own number: float32 inputs against float64 ones move every logit by at most 2^-24 ||x|| per operand
    ref = ref_loss.classifier_loss(x, z["labels"], z["kernel"], None, head, margin, fa)
    slack = 2.0 * ref["lipschitz"] * 2.0 * ref_loss.U * ref["xnorm"]
    assert abs(got["loss"].astype(np.float64).mean() - float(z["loss"])) <= np.mean(ref_loss.bounds(ref, 16, 11)[2] + slack) + 1e-9
    # margins and steps that are not in the fixtures
    others = {"asoftmax": (1, 2, 4), "additive_margin_softmax": (0.0, 0.1, 0.35, 0.5),
              "additive_angular_margin_softmax": (0.0, 0.15, 0.45, 0.55)}[head]
    for m in others:
        for s in (0, 7, 1000, 10 ** 6):
            f = ref_loss.annealing_fa(lam[0], lam[1], lam[2], lam[3], s)
            check(run(x, z["labels"], z["kernel"], None, head, m, f), x, z["labels"], z["kernel"], None, head, m, f, "neighbour")


def test_asoftmax_other_m_is_refused():
    from tf_kaldi_speaker_amd import _lib
    rs = np.random.RandomState(5)
    x, w = rs.standard_normal((4, 8)), rs.standard_normal((8, 5))
    classes, ldc = prepare(w, "asoftmax")
    rc, _ = raw_call(x, np.zeros(4, np.int32), classes, ldc, 5, None, "asoftmax", 3, 0.5)
    assert rc == _lib.XV_ERR_UNSUPPORTED


def test_range():
    rs = np.random.RandomState(6)
    e, c = 32, 300
    w = rs.standard_normal((e, c))
    x = rs.standard_normal((6, e))
    x[0] *= 300.0 / np.linalg.norm(x[0])              # exp(300 cos) overflows without the running maximum
    x[1] *= 1e-30 / np.linalg.norm(x[1])
    x[2] = 0.0
    labels = np.array([5, 140, 299, 0, 128, 127], np.int32)
    for head, m, fa in (("softmax", 0, 0), ("asoftmax", 4, 0.5), ("additive_margin_softmax", 0.3, 1.0),
                        ("additive_angular_margin_softmax", 0.4, 0.7)):
        got = run(x, labels, w, None, head, m, fa)
        check(got, x, labels, w, None, head, m, fa, "range")
        assert got["top1"][2] == 0                    # all-equal logits: the lowest index
        if head != "softmax":
            assert abs(got["loss"][2] - np.log(c)) <= ref_loss.bound_k(c) * ref_loss.U * (1.0 + np.log(c))
    # a target probability below 1e-30: the finite log-sum-exp value, not -log(1e-16) = 36.8
    wh = w / np.linalg.norm(w, axis=0, keepdims=True)
    y = np.zeros((2, e))
    y[0] = 200.0 * wh[:, 7]                           # far from class 8
    y[1] = -150.0 * wh[:, 9]
    lab = np.array([8, 9], np.int32)
    got = run(y, lab, w, None, "asoftmax", 1, 0.0)
    ref = ref_loss.classifier_loss(f32(y).astype(np.float64), lab, f32(w).astype(np.float64), None, "asoftmax", 1, 0.0)
    assert np.all(np.exp(-ref["loss"]) < 1e-30) and np.all(ref["loss"] > 70.0)
    check(got, y, lab, w, None, "asoftmax", 1, 0.0, "tiny probability")


def test_out_of_range_label_is_an_error_and_writes_nothing():
    from tf_kaldi_speaker_amd import _lib
    rs = np.random.RandomState(7)
    x, w = rs.standard_normal((130, 16)), rs.standard_normal((16, 200))
    classes, ldc = prepare(w, "additive_margin_softmax")
    for bad in (-1, 200, 2 ** 31 - 1, -2 ** 31):
        labels = rs.randint(0, 200, 130).astype(np.int32)
        labels[77] = bad
        rc, got = raw_call(x, labels, classes, ldc, 200, None, "additive_margin_softmax", 0.2, 0.5, fill=123.0)
        assert rc == _lib.XV_ERR_INVALID
        assert b"label" in _lib.load().xv_last_error(None)
        assert np.all(got["loss"] == 123.0) and np.all(got["lse"] == 123.0) and np.all(got["top1"] == -7)
    labels = rs.randint(0, 200, 130).astype(np.int32)
    rc, _ = raw_call(x, labels, classes, ldc, 200, None, "additive_margin_softmax", 0.2, 0.5, ws_bytes=1024)
    assert rc == _lib.XV_ERR_WORKSPACE
    from tf_kaldi_speaker_amd import losses
    from tf_kaldi_speaker_amd.params import Params
    p = Params(loss_func="softmax")
    with pytest.raises(_lib.XvError):
        losses.classifier_loss(f32(x), np.full(130, 200), f32(w), None, p)


def test_repeats_and_row_order_are_bit_identical():
    rs = np.random.RandomState(8)
    n, e, c = 300, 33, 700
    x, w = rs.standard_normal((n, e)), rs.standard_normal((e, c))
    labels = rs.randint(0, c, n).astype(np.int32)
    a = run(x, labels, w, None, "additive_angular_margin_softmax", 0.3, 0.6)
    b = run(x, labels, w, None, "additive_angular_margin_softmax", 0.3, 0.6)
    perm = rs.permutation(n)
    p = run(x[perm], labels[perm], w, None, "additive_angular_margin_softmax", 0.3, 0.6)
    for k in ("loss", "target_logit", "lse", "top1"):
        assert a[k].tobytes() == b[k].tobytes(), k
        assert a[k][perm].tobytes() == p[k].tobytes(), k


def test_workspace_is_a_sixteenth_of_the_logits_and_linear_in_n():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    assert lib.xv_loss_workspace(4096, 100000) < 4096 * 100000 * 4 // 16
    w0, w1, w2 = (lib.xv_loss_workspace(n, 100000) for n in (0, 1000, 2000))
    assert w1 - w0 == w2 - w1 > 0


def test_classifier_loss_host_interface():
    import torch
    from tf_kaldi_speaker_amd import losses
    from tf_kaldi_speaker_amd.params import Params
    rs = np.random.RandomState(9)
    x, w, b = f32(rs.standard_normal((40, 24))), f32(rs.standard_normal((24, 150))), f32(rs.standard_normal(150))
    labels = rs.randint(0, 150, 40)
    p = Params(loss_func="additive_margin_softmax", amsoftmax_m=0.3, amsoftmax_lambda_min=0.0, amsoftmax_lambda_base=10.0,
               amsoftmax_lambda_gamma=0.5, amsoftmax_lambda_power=1.0, aux_loss_func=["ring_loss"])
    before = dict(p.dict)
    with pytest.raises(NotImplementedError):
        losses.classifier_loss(x, labels, w, None, p, global_step=30)
    r = losses.classifier_loss(x, labels, w, None, p, global_step=30, validation=True)
    assert p.dict == before
    fa = ref_loss.annealing_fa(0.0, 10.0, 0.5, 1.0, 30)
    check(r._asdict(), x, labels, w, None, "additive_margin_softmax", 0.0, fa, "validation")
    assert r.mean == pytest.approx(float(r.loss.astype(np.float64).mean()))
    t = losses.classifier_loss(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(w).cuda(), None, p,
                               global_step=30, validation=True, as_tensor=True)
    assert t.loss.is_cuda and t.loss.cpu().numpy().tobytes() == r.loss.tobytes()
    s = losses.classifier_loss(x, labels, w, b, Params(loss_func="softmax"))
    check(s._asdict(), x, labels, w, b, "softmax", 0.0, 0.0, "softmax interface")


# ------------------------------------------------------------------------------------------------ end to end
PARITY_BAR = 1e-4             # relative L2 of an embedding against the float64 oracle (BASELINE.json)


def e2e_setup(tmp_path, loss_func):
    from tf_kaldi_speaker_amd import model_io, synth
    extra = dict(loss_func=loss_func, num_speakers_per_batch=4, num_segments_per_speaker=1, min_segment_len=35, max_segment_len=45,
                 valid_max_iterations=100, num_nodes_pooling_layer=24, num_nodes_last_layer=16,
                 amsoftmax_m=0.3, amsoftmax_lambda_min=0.0, amsoftmax_lambda_base=10.0, amsoftmax_lambda_gamma=0.5,
                 amsoftmax_lambda_power=1.0)
    if loss_func != "softmax":
        extra.update(feature_norm=True, feature_scaling_factor=12.0)
    params = dict(synth.TDNN_STAT_PARAMS, **extra)
    weights = synth.synth_weights(params, 30, seed=4, channels=8)
    rs = np.random.RandomState(21)
    weights["softmax/output/kernel"] = f32(rs.standard_normal((16, 7)))            # 7 classes, 6 of them in the data
    weights["softmax/output/bias"] = f32(0.5 * rs.standard_normal(7))
    model_dir = str(tmp_path / "exp")
    model_io.save_model(model_dir, params, 30, weights, step=4321)
    spk_utts = [("spk%d" % s, ["spk%d-u%d" % (s, u) for u in range(3)]) for s in (3, 0, 5, 1, 4, 2)]
    lens = {u: int(t) for (_, us) in spk_utts for u, t in zip(us, rs.randint(30, 61, 3))}
    data, spklist, _ = make_data_dir(tmp_path, spk_utts, lens, dim=32, spklist=[("spk%d" % s, s) for s in range(7)], seed=22)
    return params, weights, model_dir, data, spklist


def e2e_oracle(params, weights, data, spklist):
    """Planner batches -> float64 forward (oracle/ref_numpy) -> ref_loss with the validation margins."""
    from oracle import ref_numpy
    from tf_kaldi_speaker_amd import valid
    from tf_kaldi_speaker_amd.params import Params
    p = Params(**params)
    head = params["loss_func"]
    fa = 0.0 if head == "softmax" else ref_loss.annealing_fa(0.0, 10.0, 0.5, 1.0, 4321)
    bias = weights["softmax/output/bias"] if head == "softmax" else None
    means, tol, embs, labs, correct = [], [], [], [], 0
    for batch in valid.plan_for_params(data, spklist, p):
        emb = np.asarray(ref_numpy.predict(valid.read_batch(batch, 30), weights, params, 30, node="output"), dtype=np.float64)
        r = ref_loss.classifier_loss(emb, batch.labels, weights["softmax/output/kernel"].astype(np.float64),
                                     None if bias is None else bias.astype(np.float64), head, 0.0, fa)
        means.append(r["loss"].mean())
        # an embedding within PARITY_BAR ||x|| of the oracle's moves every logit by at most PARITY_BAR ||x|| max ||w||: twice that
        # for the loss, plus the head's own bound
        tol.append(np.mean(2.0 * PARITY_BAR * r["xnorm"] * r["wnorm_max"] + ref_loss.bounds(r, 16, 7)[2]))
        embs.append(emb)
        labs.append(batch.labels)
        correct += int(np.sum(r["top1"] == batch.labels))
    labs = np.concatenate(labs)
    return float(np.mean(means)), float(np.mean(tol)), np.concatenate(embs), labs, correct / float(len(labs))


@pytest.mark.parametrize("loss_func", ["softmax", "additive_margin_softmax"])
@pytest.mark.parametrize("precision", [None, "f32"])
def test_trainer_valid_matches_oracle(tmp_path, loss_func, precision):
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights, model_dir, data, spklist = e2e_setup(tmp_path, loss_func)
    want_loss, tol, want_emb, want_labels, _ = e2e_oracle(params, weights, data, spklist)
    tr = Trainer(Params(**params), model_dir, 30, single_cpu=True, device=0, precision=precision)
    tr.build("valid")
    loss, emb, labels = tr.valid(data, spklist, output_embeddings=True)
    rel = np.linalg.norm(emb - want_emb, axis=1) / np.linalg.norm(want_emb, axis=1)
    print("valid %s %s: loss %.6f oracle %.6f (tolerance %.2e), embeddings rel-L2 max %.2e, %d batches"
          % (loss_func, precision, loss, want_loss, tol, rel.max(), tr.valid_num_batches))
    np.testing.assert_array_equal(labels, want_labels)
    assert emb.shape == want_emb.shape and rel.max() <= PARITY_BAR
    assert abs(loss - want_loss) <= tol
    assert 0.0 <= tr.valid_accuracy <= 1.0
    loss2, none_emb, none_labels = tr.valid(data, spklist)
    assert loss2 == loss and none_emb is None and none_labels is None
    tr.close()


def test_valid_cli_in_a_child_process(tmp_path, repo_root):
    from tf_kaldi_speaker_amd import scoring
    params, weights, model_dir, data, spklist = e2e_setup(tmp_path, "additive_margin_softmax")
    want_loss, tol, want_emb, want_labels, want_acc = e2e_oracle(params, weights, data, spklist)
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "tf_kaldi_speaker_amd.valid", "--gpu", "0", "--precision", "f32", "--append", model_dir, data, spklist]
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("step ")]
    assert len(line) == 1, r.stdout
    f = line[0].split()
    assert f[0::2] == ["step", "loss", "acc", "eer"] and int(f[1]) == 4321
    assert abs(float(f[3]) - want_loss) <= tol + 1e-6                                # %f prints six decimals
    assert abs(float(f[5]) - want_acc) <= 1.0 / len(want_labels) + 1e-6              # a near-tie may flip one row
    # the EER is the one scoring.pairwise_eer gives on the embeddings Trainer.valid returns
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    tr = Trainer(Params(**params), model_dir, 30, single_cpu=True, device=0, precision="f32")
    tr.build("valid")
    _, emb, labels = tr.valid(data, spklist, output_embeddings=True)
    tr.close()
    eer = scoring.pairwise_eer(emb, labels)[0]
    assert abs(float(f[7]) - eer) <= 1e-6
    with open(os.path.join(model_dir, "nnet", "valid_loss")) as fh:
        appended = fh.read()
    assert appended == "%d %s %s\n" % (4321, f[3], f[7])
