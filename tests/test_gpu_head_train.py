"""GPU: training a classifier head on a frozen encoder (tf_kaldi_speaker_amd/head_train.py, train_head.py): HeadTrainer.step
against the raw gradient and optimizer calls, convergence on separable rows, train_head end to end and its command line."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from valid_data import make_data_dir                                # noqa: E402

pytestmark = pytest.mark.gpu


def f32(a):
    return np.asarray(a, dtype=np.float32)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def separable_rows(seed, n=64, e=16, c=8):
    rs = np.random.RandomState(seed)
    centres = 3.0 * rs.standard_normal((c, e))
    labels = np.arange(n) % c
    return f32(centres[labels] + 0.3 * rs.standard_normal((n, e))), labels.astype(np.int32)


MOMENTUM_PARAMS = dict(loss_func="softmax", optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=1e-3,
                       clip_gradient=True, clip_gradient_norm=3.0)


def test_step_is_the_raw_gradient_call_then_the_raw_optimizer_calls():
    import torch
    from tf_kaldi_speaker_amd import _lib, head_train, losses
    from tf_kaldi_speaker_amd.params import Params
    lib = _lib.load()
    x, labels = separable_rows(3, n=37, e=18, c=5)                       # E = 18: rows padded to 20 floats
    for extra in (dict(MOMENTUM_PARAMS), dict(MOMENTUM_PARAMS, use_nesterov=True), dict(loss_func="softmax", optimizer="adam", weight_l2_regularizer=0.0),
                  dict(loss_func="additive_margin_softmax", optimizer="sgd", weight_l2_regularizer=1e-2, amsoftmax_m=0.2,
                       amsoftmax_lambda_min=0.0, amsoftmax_lambda_base=10.0, amsoftmax_lambda_gamma=0.5, amsoftmax_lambda_power=1.0)):
        params = Params(**extra)
        ht = head_train.HeadTrainer(params, 18, 5, device=0, seed=11)
        kind, mom, nest, l2, clip = head_train.optimizer_config(params)
        e, c, ldc = 18, 5, 20
        rows = ht.head.raw_rows.clone()
        assert tuple(rows.shape) == (c, ldc)
        bias = None if ht.head.bias is None else ht.head.bias.clone()
        nslots = {0: 0, 1: 1, 2: 2}[kind]
        rslots = [torch.zeros_like(rows) for _ in range(nslots)]
        bslots = [] if bias is None else [torch.zeros_like(bias) for _ in range(nslots)]
        xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
        for t in range(1, 4):
            res = ht.step(x, labels, 0.05, global_step=100 * t)
            _, head, margin, fa = losses.head_config(params, 100 * t, False)
            out = torch.empty((3, 37), dtype=torch.float32, device="cuda")
            top1 = torch.empty((37,), dtype=torch.int32, device="cuda")
            grows = torch.zeros_like(rows)
            gbias = None if bias is None else torch.empty_like(bias)
            ws = torch.empty(int(lib.xv_loss_grad_workspace(37, c, e)), dtype=torch.uint8, device="cuda")
            _lib.check(lib.xv_loss_classifier_grad(0, _p(xd), e, 37, e, _p(ld), _p(rows), ldc, c, _p(bias), head, margin, fa, 1.0 / 37,
                                                   _p(out[0]), _p(out[1]), _p(out[2]), _p(top1), None, e, _p(grows), _p(gbias), _p(ws),
                                                   ws.numel(), None))
            ows = torch.empty(max(int(lib.xv_opt_workspace(rows.numel())), 8), dtype=torch.uint8, device="cuda")
            for w, g, slots, reg in ((rows, grows, rslots, l2),) + (() if bias is None else ((bias, gbias, bslots, 0.0),)):
                _lib.check(lib.xv_opt_step(0, kind, int(nest), _p(w), _p(g), _p(slots[0]) if slots else None,
                                           _p(slots[1]) if len(slots) > 1 else None, w.numel(), 0.05, reg, clip, mom, t, _p(ows),
                                           ows.numel(), None))
            torch.cuda.synchronize()
            assert ht.head.raw_rows.cpu().numpy().tobytes() == rows.cpu().numpy().tobytes(), (extra, t)
            if bias is not None:
                assert ht.head.bias.cpu().numpy().tobytes() == bias.cpu().numpy().tobytes(), (extra, t)
            assert res.loss == float(out[0].double().mean())
        np.testing.assert_array_equal(ht.kernel(), rows.cpu().numpy()[:, :e].T)
        assert ht.kernel().shape == (e, c) and (ht.bias() is None) == (bias is None)


SEED = 0      # start loss within 0.5 of ln 8 for this seed: checked with the numpy oracle loop in tests/test_loss_grad_host.py


def test_separable_rows_are_learned():
    from tf_kaldi_speaker_amd import head_train
    from tf_kaldi_speaker_amd.params import Params
    x, labels = separable_rows(SEED)
    x = f32(x / 12.0)                                                     # ||x|| around 1: a Xavier start near ln 8
    ht = head_train.HeadTrainer(Params(loss_func="softmax", optimizer="momentum", momentum=0.9, use_nesterov=False,
                                       weight_l2_regularizer=0.0), 16, 8, device=0, seed=SEED)
    first = acc = loss = None
    for t in range(50):
        res = ht.step(x, labels, 0.5, global_step=t)
        first = res.loss if first is None else first
        loss, acc = res.loss, res.accuracy
    print("separable rows: mean loss %.4f -> %.4f (ln 8 = %.4f), top-1 %.3f" % (first, loss, np.log(8.0), acc))
    assert abs(first - np.log(8.0)) <= 0.5
    assert loss < 0.5 * first
    assert acc == 1.0


def train_setup(tmp_path, loss_func="softmax"):
    from tf_kaldi_speaker_amd import model_io, synth
    extra = dict(loss_func=loss_func, num_speakers_per_batch=4, num_segments_per_speaker=2, min_segment_len=30, max_segment_len=40,
                 valid_max_iterations=100, num_nodes_pooling_layer=24, num_nodes_last_layer=16, num_steps_per_epoch=4, num_epochs=1,
                 learning_rate=0.1, optimizer="momentum", momentum=0.9, use_nesterov=True, weight_l2_regularizer=1e-3,
                 reduce_lr_epochs=2, seed=5)
    params = dict(synth.TDNN_STAT_PARAMS, **extra)
    weights = synth.synth_weights(params, 30, seed=4, channels=8)
    rs = np.random.RandomState(21)
    weights["softmax/output/kernel"] = f32(rs.standard_normal((16, 3)))             # the OLD head: another speaker list
    weights["softmax/output/bias"] = f32(rs.standard_normal(3))
    pre = str(tmp_path / "pretrain")
    model_io.save_model(pre, params, 30, weights, step=4321)
    spk_utts = [("spk%d" % s, ["spk%d-u%d" % (s, u) for u in range(3)]) for s in (3, 0, 5, 1, 4, 2)]
    lens = {u: int(t) for (_, us) in spk_utts for u, t in zip(us, rs.randint(42, 61, 18))}
    data, spklist, _ = make_data_dir(tmp_path, spk_utts, lens, dim=32, spklist=[("spk%d" % s, s) for s in range(6)], seed=22)
    return params, weights, pre, data, spklist


def run_train(tmp_path, name, params, weights, pre, data, spklist):
    from tf_kaldi_speaker_amd import head_train
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    tr = Trainer(Params(**params), pre, 30, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    out = str(tmp_path / name)
    endpoint = tr.embeddings
    hist = head_train.train_head(tr, data, spklist, data, spklist, out, weights=weights, seed=5, precision="f32")
    assert tr.embeddings == endpoint                                      # the caller's trainer is handed back as it came
    tr.close()
    return out, hist


def test_train_head_end_to_end(tmp_path):
    from tf_kaldi_speaker_amd import losses, model_io, valid
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights, pre, data, spklist = train_setup(tmp_path)
    out, hist = run_train(tmp_path, "tuned", params, weights, pre, data, spklist)
    assert len(hist) == 1 and hist[0][1] == 4
    nnet = os.path.join(out, "nnet")
    saved, step = model_io.load_weights(nnet)
    assert step == 4 and os.path.isfile(os.path.join(nnet, "config.json")) and os.path.isfile(os.path.join(nnet, "feature_dim"))
    assert saved["softmax/output/kernel"].shape == (16, 6) and saved["softmax/output/bias"].shape == (6,)
    for k, v in weights.items():
        if not k.startswith("softmax/"):
            assert saved[k].tobytes() == f32(v).tobytes(), k               # the encoder is frozen
    assert set(saved) == set(weights)
    # Trainer.valid on the new directory = the saved head on the same batches
    tr = Trainer(Params(**params), out, 30, single_cpu=True, device=0, precision="f32")
    tr.build("valid")
    loss, emb, labels = tr.valid(data, spklist, output_embeddings=True)
    head = losses.ClassifierHead(saved["softmax/output/kernel"], saved["softmax/output/bias"], Params(**params), 0)
    means, at = [], 0
    for batch in valid.plan_for_params(data, spklist, Params(**params)):
        n = len(batch.labels)
        means.append(head.loss(emb[at:at + n], batch.labels, global_step=4, validation=True).mean)
        at += n
    tr.close()
    assert loss == float(np.mean(np.asarray(means, dtype=np.float64)))
    assert abs(hist[0][2] - loss) == 0.0
    with open(os.path.join(nnet, "valid_loss")) as f:
        lines = f.read().splitlines()
    assert len(lines) == 1 and re.match(r"^0 \d+\.\d{6} \d+\.\d{6}$", lines[0]) and lines[0].split()[1] == "%f" % loss
    with open(os.path.join(nnet, "learning_rate")) as f:
        lines = f.read().splitlines()
    assert lines == ["0 0.10000000", "1 0.10000000"]
    # the same seed writes the same bits
    out2, _ = run_train(tmp_path, "again", params, weights, pre, data, spklist)
    again, _ = model_io.load_weights(os.path.join(out2, "nnet"))
    for k in saved:
        assert saved[k].tobytes() == again[k].tobytes(), k
    assert not np.array_equal(saved["softmax/output/kernel"], head_train_start(16, 6))


def head_train_start(e, c):
    from tf_kaldi_speaker_amd import head_train
    return head_train.xavier_uniform(e, c, 5)


def test_command_line_in_a_child_process(tmp_path, repo_root):
    from tf_kaldi_speaker_amd import model_io
    params, weights, pre, data, spklist = train_setup(tmp_path)
    out, hist = run_train(tmp_path, "inproc", params, weights, pre, data, spklist)
    cli_out = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "tf_kaldi_speaker_amd.train_head", "--gpu", "0", "--precision", "f32", pre, data, spklist, data, spklist,
           cli_out]
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("epoch ")]
    assert len(line) == 1 and line[0].split()[0::2] == ["epoch", "step", "loss", "eer", "lr"], r.stdout
    a, _ = model_io.load_weights(os.path.join(out, "nnet"))
    b, step = model_io.load_weights(os.path.join(cli_out, "nnet"))
    assert step == 4 and set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k                        # params.seed = 5 is the default seed
    assert float(line[0].split()[5]) == float("%f" % hist[0][2])
