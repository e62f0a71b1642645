#!/usr/bin/env python
"""Time the gradient of the triplet heads and a training step that uses it.  The numbers of profiles/metric_train.md come from
this tool:

    python tools/metric_train_bench.py [--iters 50] [--step-iters 20] [--warmup 3] [--rounds 3]

1. xv_metric_loss_grad beside xv_metric_loss through the C ABI on the same rows, labels and preallocated buffers, at 640 x 512
   (64 speakers x 10 segments) and 1024 x 512 (64 x 16), for the semi-hard loss and the angular loss "all" and "hard"
   (amsoftmax, margin 0.2).
2. One conv_train.ConvTrainer step at 64 segments x 300 frames (the model of tools/conv_train_bench.py) through the metric door
   (16 speakers x 4 segments, no classifier layer) beside the classifier-head step (7000 classes) of the same build, and
   MetricHead.loss_and_grad alone on the 64 x 512 embeddings of that step: the share of the step the new op takes.

Nothing is gated.  Device events around back-to-back calls after warm-up calls of each, alternating rounds in one process, one
JSON line with every round's figure."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = (5, 5, 7, 1, 1)
KINDS = (("semihard", 0, 0), ("all", 1, 2), ("hard", 2, 2))       # name, XV_METRIC_*, pos_head (amsoftmax)
MARGIN = 0.2


def window_ms(fn, torch, iters):
    """Milliseconds per call over `iters` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def rounds(fns, torch, iters, warmup, count):
    """name -> [ms per call of each round], the functions taking turns."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(count):
        for name, fn in fns.items():
            out[name].append(round(window_ms(fn, torch, iters), 4))
    return out


def op_calls(torch, lib, speakers, segments, d, device):
    """-> {"<kind> forward" / "<kind> grad": callable} on one group of speakers x segments rows."""
    n = speakers * segments
    rs = np.random.RandomState(n)
    cls = rs.permutation(np.repeat(np.arange(speakers), segments))
    x = torch.from_numpy((rs.standard_normal((speakers, d))[cls] * 0.8 + rs.standard_normal((n, d))).astype(np.float32)).to(device)
    labels = torch.from_numpy(cls.astype(np.int32)).to(device)
    off = np.array([0, n], dtype=np.int64)
    optr = off.ctypes.data_as(C.c_void_p)
    p = lambda t: C.c_void_p(t.data_ptr())                                 # noqa: E731
    rows = torch.empty(n, dtype=torch.float64, device=device)
    counts = torch.empty(n, dtype=torch.int64, device=device)
    gloss = torch.empty(1, dtype=torch.float64, device=device)
    gcount = torch.empty(2, dtype=torch.int64, device=device)
    gx = torch.empty((n, d), dtype=torch.float32, device=device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fns = {}
    for name, kind, head in KINDS:
        ws_f = torch.empty(max(int(lib.xv_metric_loss_workspace(1, optr, d, kind)), 8), dtype=torch.uint8, device=device)
        ws_g = torch.empty(int(lib.xv_metric_loss_grad_workspace(1, optr, d, kind)), dtype=torch.uint8, device=device)

        def forward(kind=kind, head=head, ws=ws_f, keep=off):
            rc = lib.xv_metric_loss(0, p(x), d, optr, 1, d, p(labels), kind, head, MARGIN, 0, 1, 0.0, 0.0, p(rows), p(counts), None, p(gloss),
                                    p(gcount), p(ws), ws.numel(), stream)
            assert rc == 0, rc

        def grad(kind=kind, head=head, ws=ws_g, keep=off):
            rc = lib.xv_metric_loss_grad(0, p(x), d, optr, 1, d, p(labels), kind, head, MARGIN, 0, 1, 1.0, p(rows), p(counts), p(gloss),
                                         p(gcount), p(gx), d, p(ws), ws.numel(), stream)
            assert rc == 0, rc
        fns[name + " forward"], fns[name + " grad"] = forward, grad
    return fns


def conv_weights(rs, d, ch, pool, nodes, embed):
    weights, cin, shapes = {}, d, []
    for idx, w in enumerate(WIDTHS, start=1):
        cout = pool if idx == len(WIDTHS) else ch
        shapes.append((idx, "conv" if w > 1 else "dense", (1, w, cin, cout) if w > 1 else (cin, cout), w * cin, cout))
        cin = cout
    shapes += [(6, "dense", (2 * pool, nodes), 2 * pool, nodes), (7, "dense", (nodes, embed), nodes, embed)]
    for idx, kind, shape, k, n in shapes:
        lim = np.sqrt(6.0 / (k + n))
        weights["tdnn/tdnn%d_%s/kernel" % (idx, kind)] = rs.uniform(-lim, lim, shape).astype(np.float32)
        weights["tdnn/tdnn%d_%s/bias" % (idx, kind)] = (0.1 * rs.standard_normal(n)).astype(np.float32)
        weights["tdnn/tdnn%d_bn/gamma" % idx] = rs.uniform(0.5, 1.5, n).astype(np.float32)
        weights["tdnn/tdnn%d_bn/beta" % idx] = (0.1 * rs.standard_normal(n)).astype(np.float32)
        weights["tdnn/tdnn%d_bn/moving_mean" % idx] = (0.1 * rs.standard_normal(n)).astype(np.float32)
        weights["tdnn/tdnn%d_bn/moving_variance" % idx] = rs.uniform(0.5, 1.5, n).astype(np.float32)
    return weights


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    args = ap.parse_args(argv)
    import torch
    from tf_kaldi_speaker_amd import _lib, conv_train, metric_losses
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("metric_train_bench needs a HIP device")
    lib = _lib.load()
    report = {"ops_ms": {}, "step_ms": {}}
    with torch.cuda.device(0):
        for speakers, segments in ((64, 10), (64, 16)):
            fns = op_calls(torch, lib, speakers, segments, 512, "cuda:0")
            report["ops_ms"]["%dx512" % (speakers * segments)] = rounds(fns, torch, args.iters, args.warmup, args.rounds)
        b, t, d = args.segments, args.frames, 30
        rs = np.random.RandomState(7000)
        weights = conv_weights(rs, d, 512, 1500, 512, 512)
        feats = torch.from_numpy(rs.standard_normal((b * t, d)).astype(np.float32)).cuda()
        offsets = np.arange(b + 1, dtype=np.int64) * t
        opt = dict(network_type="tdnn", pooling_type="statistics_pooling", optimizer="momentum", momentum=0.9, use_nesterov=False,
                   weight_l2_regularizer=1e-4)
        speakers = np.repeat(np.arange(b // 4), 4).astype(np.int32)
        losses = {"classifier (softmax, 7000 classes)": (dict(loss_func="softmax"), False, rs.randint(0, 7000, b).astype(np.int32)),
                  "metric semihard": (dict(loss_func="semihard_triplet_loss", margin=MARGIN, triplet_loss_squared=False), True, speakers),
                  "metric angular all": (dict(loss_func="angular_triplet_loss", margin=MARGIN, triplet_type="all",
                                              loss_type="additive_margin_softmax"), True, speakers)}
        fns, keep = {}, []
        for name, (extra, metric, labels) in losses.items():
            params = Params(**dict(opt, **extra))
            ct = conv_train.ConvTrainer(params, weights, 7000, device=0, seed=1, metric=metric)
            keep.append(ct)
            fns[name] = lambda ct=ct, labels=labels: ct.step(feats, offsets, labels, 0.01)
            if metric:
                head = metric_losses.MetricHead(params, 0)
                y = ct.forward(feats, offsets).clone()
                lab = torch.from_numpy(labels).cuda()
                fns[name + ": loss_and_grad alone"] = lambda head=head, y=y, lab=lab: head.loss_and_grad(y, lab, as_tensor=True, sync=False)
        report["step_ms"] = rounds(fns, torch, args.step_iters, args.warmup, args.rounds)
    report["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
