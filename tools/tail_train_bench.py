#!/usr/bin/env python
"""Time one training step of the two segment-level layers and the head on frozen pooled rows (tail_train.TailTrainer.step: two
xv_seg_forward, one xv_loss_classifier_grad, two xv_seg_backward and one xv_opt_step per tensor) beside the same step written in
torch fp32 autograd on the same device, TF32 off: linear, eval-mode batch_norm, relu, cross_entropy, backward to the ten tensors,
and a hand-written momentum update.  The numbers of profiles/tail_train.md come from this tool:

    python tools/tail_train_bench.py [--n 640] [--pool 3000] [--nodes 512] [--embed 512] [--classes 7000] [--iters 500]
                                     [--warmup 10] [--rounds 3]

No time is gated: the torch number is the context.  The two are timed in alternating rounds inside one process, device events
around `iters` back-to-back steps, one JSON line with every round's figure.  The parameters after the first step are compared
with the torch step at the size that is timed."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window_ms(fn, torch, iters):
    """Milliseconds per call over `iters` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=640)
    ap.add_argument("--pool", type=int, default=3000)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--classes", type=int, default=7000)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as fn
    from tf_kaldi_speaker_amd import _lib, tail_train
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("tail_train_bench needs a HIP device")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    lib = _lib.load()
    dev = "cuda:%d" % args.device
    n, k, h, e, c = args.n, args.pool, args.nodes, args.embed, args.classes
    rs = np.random.RandomState(c)
    weights = {}
    for idx, (a, b) in ((6, (k, h)), (7, (h, e))):
        lim = np.sqrt(6.0 / (a + b))
        weights["tdnn/tdnn%d_dense/kernel" % idx] = rs.uniform(-lim, lim, (a, b)).astype(np.float32)
        weights["tdnn/tdnn%d_dense/bias" % idx] = (0.1 * rs.standard_normal(b)).astype(np.float32)
        weights["tdnn/tdnn%d_bn/gamma" % idx] = rs.uniform(0.5, 1.5, b).astype(np.float32)
        weights["tdnn/tdnn%d_bn/beta" % idx] = (0.1 * rs.standard_normal(b)).astype(np.float32)
        weights["tdnn/tdnn%d_bn/moving_mean" % idx] = (0.1 * rs.standard_normal(b)).astype(np.float32)
        weights["tdnn/tdnn%d_bn/moving_variance" % idx] = rs.uniform(0.5, 1.5, b).astype(np.float32)
    x = torch.from_numpy(rs.standard_normal((n, k)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rs.randint(0, c, n).astype(np.int32)).to(dev)
    lab64 = labels.long()
    l2, lr, mom = 1e-4, 0.01, 0.9
    params = Params(network_type="tdnn", loss_func="softmax", optimizer="momentum", momentum=mom, use_nesterov=False,
                    weight_l2_regularizer=l2)
    with torch.cuda.device(args.device):
        tt = tail_train.TailTrainer(params, weights, c, device=args.device, seed=1)
        start = tt.variables()
        names = list(start)
        tensors = [torch.from_numpy(start[name]).to(dev).requires_grad_(True) for name in names]
        decay = [l2 if name.endswith("/kernel") else 0.0 for name in names]
        accum = [torch.zeros_like(t) for t in tensors]
        stats = [[torch.from_numpy(weights["tdnn/tdnn%d_bn/%s" % (idx, s)]).to(dev) for s in ("moving_mean", "moving_variance")]
                 for idx in (6, 7)]

        def eager():
            w1, b1, g1, be1, w2, b2, g2, be2, wk, bk = tensors
            y = fn.relu(fn.batch_norm(x @ w1 + b1, stats[0][0], stats[0][1], g1, be1, training=False, eps=1e-3))
            y = fn.relu(fn.batch_norm(y @ w2 + b2, stats[1][0], stats[1][1], g2, be2, training=False, eps=1e-3))
            loss = fn.cross_entropy(y @ wk + bk, lab64)
            grads = torch.autograd.grad(loss, tensors)
            with torch.no_grad():
                for t, gr, a, d in zip(tensors, grads, accum, decay):
                    a.mul_(mom).add_(gr + d * t)
                    t.sub_(lr * a)
            return loss

        def ours():
            tt.step(x, labels, lr, global_step=0)

        # agreement at this size: the parameters after one step of each
        ours()
        eager()
        after = tt.variables()
        agree = {}
        for name, t in zip(names, tensors):
            moved = float(np.max(np.abs(after[name] - start[name])))
            agree[name] = float(np.max(np.abs(after[name] - t.detach().cpu().numpy()))) / max(moved, 1e-30)
        for _ in range(args.warmup):
            ours()
            eager()
        torch.cuda.synchronize()
        hip_ms, torch_ms = [], []
        for _ in range(args.rounds):
            hip_ms.append(window_ms(ours, torch, args.iters))
            torch_ms.append(window_ms(eager, torch, args.iters))
    flops = 3 * 2.0 * n * (k * h + h * e + e * c) - 2.0 * n * k * h          # three products per layer; no gx of the first layer
    print(json.dumps(dict(n=n, pool=k, nodes=h, embed=e, classes=c, iters=args.iters, hip_step_ms=hip_ms, torch_step_ms=torch_ms,
                          hip_step_ms_median=float(np.median(hip_ms)), torch_step_ms_median=float(np.median(torch_ms)),
                          first_step_difference_over_update=agree,
                          seg_workspace_bytes=[int(lib.xv_seg_workspace(n, k, h)), int(lib.xv_seg_workspace(n, h, e))],
                          note="TailTrainer.step reads the mean loss back every step (one host synchronisation) and waits once "
                               "for the label check; the torch loop does neither",
                          gemm_flops=flops, hip_tflops=flops / (float(np.median(hip_ms)) * 1e-3) / 1e12)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
