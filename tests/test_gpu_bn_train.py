"""GPU: the trainers' batch_norm="batch" mode (tail_train.Layer with batch_stats on xv_bn_batch_forward / xv_bn_batch_backward)
against a torch float64 model of the same stack in training mode, on the small synthetic TDNN of tests/test_gpu_conv_train.py.

The torch model is rebuilt from the device's own parameters (trainer.variables()) before every step, so only the step under
test is compared, not an optimizer's history; its running statistics live on across the steps.  torch's batch_norm moves its
running variance towards the Bessel-corrected batch variance, which is the rule of the layers with bessel (rank-4 kernels); for
the others the same update is fed the biased variance.  Judged by the project's parity requirement, 1e-4 relative L2 per
tensor.  The bias in front of a batch norm in training mode has the exact gradient zero (the mean is subtracted): it is judged
against the column sums of |gz|, the size of the terms that cancel.

batchnorm_momentum is 0.5 here so that three steps move the statistics far from the checkpoint's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from test_gpu_conv_train import CHANNELS, CLASSES, LENGTHS, POOL, small_model, toy_segments       # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
MOMENTUM = 0.5
EPS = 1e-3
HEAD_K, HEAD_B = "softmax/output/kernel", "softmax/output/bias"
EXTRA = dict(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=1e-3, batchnorm_momentum=MOMENTUM)


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


class TorchStack(object):
    """frame layers (conv1d of any width) -> statistics pooling -> segment layers -> softmax head, float64, with the
    running statistics R (name -> tensor) kept across calls."""

    def __init__(self, frame_specs, seg_specs, weights, bessel, pool=True):
        import torch
        self.torch, self.frame_specs, self.seg_specs, self.bessel, self.pool = torch, tuple(frame_specs), tuple(seg_specs), bessel, pool
        self.R = {}
        for spec in self.frame_specs + self.seg_specs:
            if spec.bn:
                for s in ("moving_mean", "moving_variance"):
                    self.R[spec.bn + "/" + s] = torch.tensor(np.asarray(weights[spec.bn + "/" + s], dtype=np.float64))

    def _bn(self, z, spec, P, train):
        torch = self.torch
        bn = torch.nn.functional.batch_norm
        mm, mv = self.R[spec.bn + "/moving_mean"], self.R[spec.bn + "/moving_variance"]
        g, b = P[spec.bn + "/gamma"], P[spec.bn + "/beta"]
        if not train:
            return bn(z, mm, mv, g, b, False, 0.0, EPS)
        if self.bessel[spec.kernel]:
            return bn(z, mm, mv, g, b, True, 1.0 - MOMENTUM, EPS)           # torch's running_var takes n / (n - 1)
        y = bn(z, None, None, g, b, True, 0.0, EPS)
        with torch.no_grad():                                                # the same update fed the biased variance
            mm += (z.mean(0) - mm) * (1.0 - MOMENTUM)
            mv += (z.var(0, unbiased=False) - mv) * (1.0 - MOMENTUM)
        return y

    def _act(self, h, act):
        torch = self.torch
        return h if act == 0 else torch.relu(h) if act == 1 else torch.nn.functional.leaky_relu(h, float(np.float32(0.2)))

    def run(self, variables, x, offsets, labels, train):
        """-> (output endpoint, name -> gradient in TensorFlow shapes, name of a bias -> column sums of |gz| of its layer)."""
        torch = self.torch
        P = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in variables.items()}
        h, off, zs = torch.tensor(np.asarray(x, dtype=np.float64)), [int(o) for o in offsets], {}
        for spec in self.frame_specs:
            k = P[spec.kernel]
            k3 = k[0] if k.dim() == 4 else k if k.dim() == 3 else k[None]                       # [W, C, N]
            w = k3.permute(2, 1, 0)
            outs = [torch.nn.functional.conv1d(h[off[u]:off[u + 1]].t()[None], w, P[spec.bias])[0].t() for u in range(len(off) - 1)]
            z = torch.cat(outs, dim=0)
            z.retain_grad()
            zs[spec.bias] = z
            off = [0] + list(np.cumsum([o.shape[0] for o in outs]))
            h = self._act(self._bn(z, spec, P, train), spec.act)
        if self.pool:
            rows = []
            for u in range(len(off) - 1):
                xu = h[off[u]:off[u + 1]]
                m = xu.mean(0)
                v = ((xu - m) ** 2).mean(0)
                rows.append(torch.cat([m, torch.sqrt(torch.clamp(v, min=1e-12))]))
            h = torch.stack(rows)
        for spec in self.seg_specs:
            z = h @ P[spec.kernel] + P[spec.bias]
            z.retain_grad()
            zs[spec.bias] = z
            h = self._act(self._bn(z, spec, P, train) if spec.bn else z, spec.act)
        out = h
        if labels is None:
            return out.detach().numpy(), None, None
        logits = out @ P[HEAD_K] + P[HEAD_B]
        torch.nn.functional.cross_entropy(logits, torch.tensor(np.asarray(labels, dtype=np.int64))).backward()
        return (out.detach().numpy(), {k: p.grad.numpy() for k, p in P.items() if p.grad is not None},
                {k: z.grad.abs().sum(0).numpy() for k, z in zs.items()})


def device_grads(trainer):
    """name -> the gradient the last step left on the device, in TensorFlow shapes."""
    from tf_kaldi_speaker_amd import conv_train
    shapes = {spec.kernel: (layer, getattr(layer, "shape", (layer.in_dim, layer.out_dim))) for spec, layer in zip(trainer.specs, trainer.layers)}
    out = {}
    for name, _, g, _ in trainer.tensors():
        g = g.cpu().numpy()
        if name in shapes:
            layer, shape = shapes[name]
            g = conv_train.rows_to_kernel(g[:, :layer.in_dim], shape)
        elif name == HEAD_K:
            g = g[:, :trainer.embed_dim].T
        out[name] = g
    return out


def three_checks(trainer, train_forward, stack, x, offsets, labels, weights, args):
    """The three checks of one trainer: a backward and the training-mode endpoint, the moving statistics after three steps, the
    inference forward after them."""
    bn_specs = [s for s in trainer.specs if s.bn]
    assert all(layer.batch_stats for spec, layer in zip(trainer.specs, trainer.layers) if spec.bn)
    for t in range(3):
        variables = {k: v for k, v in trainer.variables().items() if "moving" not in k}
        assert set(variables) == set(n for n, _, _, _ in trainer.tensors())               # the optimizer's list has no moving statistics
        if t == 0:
            y_dev = train_forward().cpu().numpy()                                          # training mode, on a twin: one update each
        trainer.step(*args, labels, 0.05, global_step=t)
        y, grads, gz_sums = stack.run(variables, x, offsets, labels, True)
        got = device_grads(trainer)
        assert set(got) == set(grads)
        if t == 0:
            print("output endpoint (training mode): relative L2 %.3e" % rel(y_dev, y))
            assert rel(y_dev, y) <= TOL
        for name in sorted(grads):
            if name in gz_sums and any(s.bias == name and s.bn for s in trainer.specs):
                err = np.linalg.norm(got[name] - grads[name]) / np.linalg.norm(gz_sums[name])
                print("step %d %s: |error| / |column sums of |gz|| %.3e (the exact gradient is zero)" % (t, name, err))
            else:
                err = rel(got[name], grads[name])
                print("step %d %s: relative L2 %.3e" % (t, name, err))
            assert err <= TOL, (name, t, err)
    after = trainer.variables()
    for spec in bn_specs:
        for s in ("moving_mean", "moving_variance"):
            name = spec.bn + "/" + s
            err = rel(after[name], stack.R[name].numpy())
            moved = rel(after[name], weights[name])
            print("%s after three steps: relative L2 %.3e against torch, %.3e away from the checkpoint" % (name, err, moved))
            assert err <= TOL and moved > 100 * TOL, (name, err, moved)
    final = {k: v for k, v in after.items() if "moving" not in k}
    want, _, _ = stack.run(final, x, offsets, None, False)
    got = trainer.forward(*args).cpu().numpy()
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    print("forward() against torch eval(): relative L2 per row, largest %.3e" % float(err.max()))
    assert err.max() <= TOL
    assert trainer.variables()[bn_specs[0].bn + "/moving_mean"].tobytes() == after[bn_specs[0].bn + "/moving_mean"].tobytes()   # forward() moves nothing


@pytest.mark.parametrize("network_type", ("tdnn", "extended_tdnn"))
def test_conv_trainer_against_torch(network_type):
    import torch
    from tf_kaldi_speaker_amd import conv_train
    from tf_kaldi_speaker_amd.params import Params
    params, weights = small_model(network_type=network_type, **EXTRA)
    feats, offsets, labels = toy_segments(17, CLASSES, 2, LENGTHS[network_type])
    make = lambda: conv_train.ConvTrainer(Params(**params), weights, CLASSES, device=0, seed=3, batch_norm="batch")       # noqa: E731
    ct, twin = make(), make()
    rank4 = network_type == "tdnn"
    bessel = {spec.kernel: layer.bessel for spec, layer in zip(ct.specs, ct.layers)}
    # the rank of the layer's own kernel: the conv2d layers of the TDNN alone (tail_train.batch_stats_options)
    assert bessel == {spec.kernel: rank4 and getattr(spec, "taps", 1) > 1 for spec in ct.specs}
    assert all(layer.momentum == MOMENTUM for layer in ct.layers)
    stack = TorchStack(ct.frame_specs, ct.tail.specs, weights, bessel)
    dev = torch.from_numpy(feats).cuda()
    three_checks(ct, lambda: twin._forward(dev, offsets), stack, feats, offsets, labels, weights, (dev, offsets))


def test_frame_trainer_against_torch():
    import torch
    from tf_kaldi_speaker_amd import frame_train
    from tf_kaldi_speaker_amd.params import Params
    params, weights = small_model(**EXTRA)
    r = np.random.RandomState(5)
    lens = [23, 31, 20, 36, 27, 29]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    labels = np.repeat(np.arange(CLASSES), 2).astype(np.int32)
    frames = np.maximum(r.standard_normal((int(offsets[-1]), CHANNELS)) + 0.3 * labels[np.repeat(np.arange(6), lens)][:, None], 0.0).astype(np.float32)
    make = lambda: frame_train.FrameTrainer(Params(**params), weights, CLASSES, device=0, seed=3, batch_norm="batch")     # noqa: E731
    ft, twin = make(), make()
    assert not any(layer.bessel for layer in ft.layers)                                   # dense layers behind the squeeze
    stack = TorchStack(ft.frame_specs, ft.tail.specs, weights, {spec.kernel: False for spec in ft.specs})
    dev = torch.from_numpy(frames).cuda()
    assert ft.in_dim == CHANNELS
    three_checks(ft, lambda: twin._forward(dev, offsets), stack, frames, offsets, labels, weights, (dev, offsets))


def test_tail_trainer_against_torch():
    from tf_kaldi_speaker_amd import tail_train
    from tf_kaldi_speaker_amd.params import Params
    params, weights = small_model(**EXTRA)
    r = np.random.RandomState(6)
    labels = np.repeat(np.arange(CLASSES), 4).astype(np.int32)
    pooled = (r.standard_normal((labels.size, 2 * POOL)) + 0.5 * labels[:, None]).astype(np.float32)
    make = lambda: tail_train.TailTrainer(Params(**params), weights, CLASSES, device=0, seed=3, batch_norm="batch")       # noqa: E731
    tt, twin = make(), make()
    import torch
    assert tt.pool_dim == 2 * POOL and not any(layer.bessel for layer in tt.layers)
    stack = TorchStack((), tt.specs, weights, {spec.kernel: False for spec in tt.specs}, pool=False)
    three_checks(tt, lambda: twin._forward(torch.from_numpy(pooled).cuda()), stack, pooled, [0], labels, weights, (pooled,))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def test_layers_without_batch_stats_keep_their_bits():
    """A SegLayer and a TConvLayer built as before (batch_stats=False) and one built with batch_stats but run with training=False
    return the bits of the operators called directly with the four batch-norm vectors, and move no moving statistic."""
    import torch
    from tf_kaldi_speaker_amd import _lib, conv_train, tail_train
    lib = _lib.load()
    r = np.random.RandomState(8)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                                          # noqa: E731
    K, N, n, act = 10, 7, 37, _lib.XV_SEG_ACT_LRELU
    kernel, bias = f32(r.standard_normal((K, N)) / 3.0), f32(r.standard_normal(N))
    bn = [f32(r.standard_normal(N)), f32(r.standard_normal(N)), f32(0.1 * r.standard_normal(N)), f32(0.5 + r.rand(N))]
    x, gy = torch.from_numpy(f32(r.standard_normal((n, K)))).cuda(), torch.from_numpy(f32(r.standard_normal((n, N)))).cuda()
    # ---- the operators, directly
    ldw = (K + 3) // 4 * 4
    w = torch.zeros((N, ldw), dtype=torch.float32, device="cuda")
    w[:, :K] = torch.from_numpy(kernel.T.copy()).cuda()
    b, bnd = torch.from_numpy(bias).cuda(), [torch.from_numpy(v).cuda() for v in bn]
    z, y = torch.empty((n, N), device="cuda"), torch.empty((n, N), device="cuda")
    _lib.check(lib.xv_seg_forward(0, _p(x), K, n, K, _p(w), ldw, N, _p(b), _p(bnd[0]), _p(bnd[1]), _p(bnd[2]), _p(bnd[3]), act, _p(z), N,
                                  _p(y), N, None))
    gx, gw, gb, gg, gbe = (torch.zeros(s, device="cuda") for s in ((n, K), (N, ldw), (N,), (N,), (N,)))
    ws = torch.empty(int(lib.xv_seg_workspace(n, K, N)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.xv_seg_backward(0, _p(gy), N, _p(x), K, _p(z), N, n, K, _p(w), ldw, N, _p(bnd[0]), _p(bnd[1]), _p(bnd[2]), _p(bnd[3]),
                                   act, _p(gx), K, _p(gw), _p(gb), _p(gg), _p(gbe), _p(ws), ws.numel(), None))
    torch.cuda.synchronize()
    want = [t.cpu().numpy().tobytes() for t in (y, gx, gw, gb, gg, gbe)]
    for layer, kw in ((tail_train.SegLayer(kernel, bias, bn, act), {}),
                      (tail_train.SegLayer(kernel, bias, bn, act, batch_stats=True, momentum=0.5), dict(training=False))):
        ly = layer.forward(x, **kw)
        lgx = layer.backward(gy, True)
        got = [t.cpu().numpy().tobytes() for t in (ly, lgx, layer.gw, layer.gb, layer.ggamma, layer.gbeta)]
        assert got == want
        assert layer.bn[2].cpu().numpy().tobytes() == bn[2].tobytes() and layer.bn[3].cpu().numpy().tobytes() == bn[3].tobytes()
    # ---- the temporal convolution
    W, Cc = 3, 5
    k4 = f32(r.standard_normal((1, W, Cc, N)) / 3.0)
    rows, _, _ = conv_train.kernel_to_rows(k4)
    offsets = np.array([0, 9, 20, 27], dtype=np.int64)
    xc = torch.from_numpy(f32(r.standard_normal((27, Cc)))).cuda()
    out_off = conv_train.out_offsets(offsets, W)
    total_out, batch, total_in = int(out_off[-1]), 3, 27
    gyc = torch.from_numpy(f32(r.standard_normal((total_out, N)))).cuda()
    ldw = (W * Cc + 3) // 4 * 4
    w = torch.zeros((N, ldw), dtype=torch.float32, device="cuda")
    w[:, :W * Cc] = torch.from_numpy(rows).cuda()
    off = torch.from_numpy(offsets.astype(np.int32)).cuda()
    z, y = torch.empty((total_out, N), device="cuda"), torch.empty((total_out, N), device="cuda")
    ws = torch.empty(int(lib.xv_tconv_workspace(batch, total_in, total_out, W, Cc, N)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.xv_tconv_forward(0, _p(xc), Cc, Cc, W, _p(off), batch, total_in, total_out, _p(w), ldw, N, _p(b), _p(bnd[0]), _p(bnd[1]),
                                    _p(bnd[2]), _p(bnd[3]), act, _p(z), N, _p(y), N, _p(ws), ws.numel(), None))
    gx, gw, gb, gg, gbe = (torch.zeros(s, device="cuda") for s in ((27, Cc), (N, ldw), (N,), (N,), (N,)))
    _lib.check(lib.xv_tconv_backward(0, _p(gyc), N, _p(xc), Cc, Cc, W, _p(off), batch, total_in, total_out, _p(z), N, _p(w), ldw, N,
                                     _p(bnd[0]), _p(bnd[1]), _p(bnd[2]), _p(bnd[3]), act, _p(gx), Cc, _p(gw), _p(gb), _p(gg), _p(gbe),
                                     _p(ws), ws.numel(), None))
    torch.cuda.synchronize()
    want = [t.cpu().numpy().tobytes() for t in (y, gx, gw, gb, gg, gbe)]
    for layer, kw in ((conv_train.TConvLayer(k4, bias, bn, act), {}),
                      (conv_train.TConvLayer(k4, bias, bn, act, batch_stats=True, bessel=True), dict(training=False))):
        ly, oo = layer.forward(xc, offsets, **kw)
        assert np.array_equal(oo, out_off)
        lgx = layer.backward(gyc, True)
        got = [t.cpu().numpy().tobytes() for t in (ly, lgx, layer.gw, layer.gb, layer.ggamma, layer.gbeta)]
        assert got == want
        assert layer.bn[2].cpu().numpy().tobytes() == bn[2].tobytes() and layer.bn[3].cpu().numpy().tobytes() == bn[3].tobytes()


def test_train_head_writes_the_moved_statistics(tmp_path):
    """train_head(conv_layers=True, batch_norm="batch"): the checkpoint holds moving statistics that moved, of every trained batch
    norm, beside everything --conv-layers writes; the validation ran on it (a finite loss)."""
    from test_gpu_head_train import train_setup
    from tf_kaldi_speaker_amd import conv_train, head_train, model_io
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights, pre, data, spklist = train_setup(tmp_path)
    tr = Trainer(Params(**params), pre, 30, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights, 0)
    out = str(tmp_path / "batch")
    hist = head_train.train_head(tr, data, spklist, data, spklist, out, weights=weights, seed=5, precision="f32", conv_layers=True,
                                 batch_norm="batch")
    tr.close()
    assert len(hist) == 1 and np.isfinite(hist[0][2])
    saved, _ = model_io.load_weights(os.path.join(out, "nnet"))
    assert set(saved) == set(weights)
    names = set(conv_train.trained_names(params))
    moving = [k for k in weights if k.endswith("/moving_mean") or k.endswith("/moving_variance")]
    assert len(moving) == 14
    for k, v in weights.items():
        changed = saved[k].tobytes() != np.asarray(v, dtype=np.float32).tobytes()
        assert changed == (k in names or k in moving), k


def test_default_mode_is_todays_trainer():
    """batch_norm="moving", given or left out: the same bits after a step, no moving statistic among the variables."""
    import torch
    from tf_kaldi_speaker_amd import conv_train
    from tf_kaldi_speaker_amd.params import Params
    params, weights = small_model(**EXTRA)
    feats, offsets, labels = toy_segments(17, CLASSES, 2, LENGTHS["tdnn"])
    dev = torch.from_numpy(feats).cuda()
    a = conv_train.ConvTrainer(Params(**params), weights, CLASSES, device=0, seed=3)
    b = conv_train.ConvTrainer(Params(**params), weights, CLASSES, device=0, seed=3, batch_norm="moving")
    assert a.step(dev, offsets, labels, 0.05).loss == b.step(dev, offsets, labels, 0.05).loss
    va, vb = a.variables(), b.variables()
    assert list(va) == list(vb) == [n for n in va if "moving" not in n] and set(va) == set(conv_train.trained_names(params))
    assert all(va[k].tobytes() == vb[k].tobytes() for k in va)
    assert not any(layer.batch_stats for layer in a.layers)
    with pytest.raises(ValueError):
        conv_train.ConvTrainer(Params(**params), weights, CLASSES, device=0, seed=3, batch_norm="renorm")
