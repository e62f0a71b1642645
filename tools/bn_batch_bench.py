#!/usr/bin/env python
"""Time batch norm in training mode (csrc/bn_batch.hip): xv_bn_batch_forward and xv_bn_batch_backward alone, with the bytes per
second they reach beside the traffic their passes imply, and one conv_train.ConvTrainer step with batch_norm="batch" beside the
same step with batch_norm="moving" of the same build and beside torch fp32 autograd of the same stack in training mode, TF32 off.
The numbers of profiles/bn_batch.md come from this tool:

    python tools/bn_batch_bench.py [--rows 18304,64] [--width 512] [--segments 64] [--frames 300] [--dim 30] [--channels 512]
                                   [--pool 1500] [--nodes 512] [--embed 512] [--classes 7000] [--iters 20] [--warmup 3] [--rounds 3]

No time is gated.  Everything is timed in alternating rounds inside one process, device events around back-to-back calls after
warm-up calls of each, one JSON line with every round's figure.  The stages of both steps are timed on ConvTrainer.step itself,
through its `mark` callback; the difference of a stage between the two modes is what the mode costs there: in the forward stages
the three sweeps and the scratch y the operator still writes, in the backward stages the sweep, the gz pass and the
pass-through mask of the operator, which reads gz and z and writes gz once more.  Those two redundant passes are also given as
the time their bytes take at the rate the operators reach at the same size (an estimate, named as such)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = (5, 5, 7, 1, 1)
STAGES = ("frame_forward", "pool_forward", "segment_forward", "head", "segment_backward", "pool_backward", "frame_backward", "optimizer")


def window_ms(fn, torch, iters):
    """Milliseconds per call over `iters` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def marked_step(ct, feats, offsets, labels, lr, torch):
    """One ConvTrainer.step(mark=...) with a device event at every mark -> milliseconds per stage."""
    spare = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 2 * len(ct.frame_layers) + 1)]
    ev = {}

    def mark(stage):
        ev[stage] = spare.pop()
        ev[stage].record()
    ct.step(feats, offsets, labels, lr, global_step=0, mark=mark)
    ev["optimizer"].synchronize()
    borders = [ev["start"]] + [ev[s] for s in STAGES]
    return [borders[i].elapsed_time(borders[i + 1]) for i in range(len(STAGES))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=str, default="18304,64")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--dim", type=int, default=30)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--pool", type=int, default=1500)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--classes", type=int, default=7000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as fn
    from tf_kaldi_speaker_amd import _lib, conv_train
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("bn_batch_bench needs a HIP device")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    lib = _lib.load()
    dev = "cuda:%d" % args.device
    ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())        # noqa: E731
    med = lambda v: float(np.median(v))                                     # noqa: E731
    out = dict(iters=args.iters, rounds=args.rounds, ops=[])
    with torch.cuda.device(args.device):
        stream = C.c_void_p(torch.cuda.current_stream(args.device).cuda_stream)
        # ---- the two operators alone
        N = args.width
        for n in [int(v) for v in args.rows.split(",")]:
            z, gy = torch.randn((n, N), device=dev), torch.randn((n, N), device=dev)
            y, gz = torch.empty((n, N), device=dev), torch.empty((n, N), device=dev)
            gamma, beta = torch.rand((N,), device=dev) + 0.5, torch.randn((N,), device=dev)
            mm, mv = torch.zeros((N,), device=dev), torch.ones((N,), device=dev)
            mu, var, gg, gb = (torch.empty((N,), device=dev) for _ in range(4))
            ws = torch.empty(int(lib.xv_bn_batch_workspace(n, N)), dtype=torch.uint8, device=dev)

            def fwd():
                _lib.check(lib.xv_bn_batch_forward(args.device, ptr(z), N, n, N, ptr(gamma), ptr(beta), 1, 0.99, 0, ptr(mm), ptr(mv),
                                                   ptr(y), N, ptr(mu), ptr(var), ptr(ws), ws.numel(), stream))

            def bwd():
                _lib.check(lib.xv_bn_batch_backward(args.device, ptr(gy), N, ptr(z), N, n, N, ptr(mu), ptr(var), ptr(gamma), ptr(beta), 1,
                                                    ptr(gz), N, ptr(gg), ptr(gb), ptr(ws), ws.numel(), stream))

            zt = z.clone().requires_grad_(True)
            gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)

            def torch_fwd():
                return fn.relu(fn.batch_norm(zt, mm, mv, gt, bt, training=True, momentum=0.01, eps=1e-3))

            def torch_fb():
                torch.autograd.grad(torch_fwd(), (zt, gt, bt), gy)

            for f in (fwd, bwd, torch_fwd, torch_fb):
                for _ in range(args.warmup):
                    f()
            torch.cuda.synchronize()
            ms = {k: [] for k in ("forward", "backward", "torch_forward", "torch_forward_backward")}
            for _ in range(args.rounds):
                ms["forward"].append(window_ms(fwd, torch, args.iters))
                ms["backward"].append(window_ms(bwd, torch, args.iters))
                ms["torch_forward"].append(window_ms(torch_fwd, torch, args.iters))
                ms["torch_forward_backward"].append(window_ms(torch_fb, torch, args.iters))
            fbytes, bbytes = 4 * 4 * n * N, 5 * 4 * n * N                   # 3 reads of z + y; 2 reads of gy and z + gz
            out["ops"].append(dict(rows=n, width=N, ms=ms, ms_median={k: med(v) for k, v in ms.items()}, forward_bytes=fbytes,
                                   backward_bytes=bbytes, forward_gb_per_s=fbytes / med(ms["forward"]) / 1e6,
                                   backward_gb_per_s=bbytes / med(ms["backward"]) / 1e6, forward_launches=5, backward_launches=3))

        # ---- one ConvTrainer step in both modes and torch autograd in training mode
        b, t, d, ch, p, h, e, c = args.segments, args.frames, args.dim, args.channels, args.pool, args.nodes, args.embed, args.classes
        rs = np.random.RandomState(c)
        weights, cin, shapes = {}, d, []
        for idx, w in enumerate(WIDTHS, start=1):
            cout = p if idx == len(WIDTHS) else ch
            shapes.append((idx, "conv" if w > 1 else "dense", (1, w, cin, cout) if w > 1 else (cin, cout), w * cin, cout))
            cin = cout
        shapes += [(6, "dense", (2 * p, h), 2 * p, h), (7, "dense", (h, e), h, e)]
        for idx, kind, shape, k, n in shapes:
            lim = np.sqrt(6.0 / (k + n))
            weights["tdnn/tdnn%d_%s/kernel" % (idx, kind)] = rs.uniform(-lim, lim, shape).astype(np.float32)
            weights["tdnn/tdnn%d_%s/bias" % (idx, kind)] = (0.1 * rs.standard_normal(n)).astype(np.float32)
            weights["tdnn/tdnn%d_bn/gamma" % idx] = rs.uniform(0.5, 1.5, n).astype(np.float32)
            weights["tdnn/tdnn%d_bn/beta" % idx] = (0.1 * rs.standard_normal(n)).astype(np.float32)
            weights["tdnn/tdnn%d_bn/moving_mean" % idx] = (0.1 * rs.standard_normal(n)).astype(np.float32)
            weights["tdnn/tdnn%d_bn/moving_variance" % idx] = rs.uniform(0.5, 1.5, n).astype(np.float32)
        feats = torch.from_numpy(rs.standard_normal((b * t, d)).astype(np.float32)).to(dev)
        feats_nct = feats.view(b, t, d).permute(0, 2, 1).contiguous()
        offsets = np.arange(b + 1, dtype=np.int64) * t
        labels = torch.from_numpy(rs.randint(0, c, b).astype(np.int32)).to(dev)
        lab64 = labels.long()
        l2, lr, mom = 1e-4, 0.01, 0.9
        params = Params(network_type="tdnn", loss_func="softmax", pooling_type="statistics_pooling", optimizer="momentum", momentum=mom,
                        use_nesterov=False, weight_l2_regularizer=l2, batchnorm_momentum=0.99)
        moving = conv_train.ConvTrainer(params, weights, c, device=args.device, seed=1)
        batch = conv_train.ConvTrainer(params, weights, c, device=args.device, seed=1, batch_norm="batch")
        start = {k: v for k, v in batch.variables().items() if "moving" not in k}
        names = list(start)
        tensors = [torch.from_numpy(start[name]).to(dev).requires_grad_(True) for name in names]
        decay = [l2 if name.endswith("/kernel") else 0.0 for name in names]
        accum = [torch.zeros_like(v) for v in tensors]
        stats = [[torch.from_numpy(weights["tdnn/tdnn%d_bn/%s" % (idx, s)]).to(dev) for s in ("moving_mean", "moving_variance")]
                 for idx in range(1, 8)]

        def conv_weight(k):
            return k[0].permute(2, 1, 0) if k.dim() == 4 else k.t()[:, :, None]

        def eager():
            y = feats_nct
            for i in range(5):
                w, bias, g, be = tensors[4 * i:4 * i + 4]
                y = fn.relu(fn.batch_norm(fn.conv1d(y, conv_weight(w), bias), stats[i][0], stats[i][1], g, be, training=True,
                                          momentum=0.01, eps=1e-3))
            mean = y.mean(dim=2, keepdim=True)
            var = ((y - mean) ** 2).mean(dim=2)
            mask = (var <= 1e-12).float().detach()
            y = torch.cat([mean.squeeze(2), torch.sqrt((1.0 - mask) * var + mask * 1e-12)], dim=1)
            for i in range(5, 7):
                w, bias, g, be = tensors[4 * i:4 * i + 4]
                y = fn.relu(fn.batch_norm(y @ w + bias, stats[i][0], stats[i][1], g, be, training=True, momentum=0.01, eps=1e-3))
            loss = fn.cross_entropy(y @ tensors[28] + tensors[29], lab64)
            grads = torch.autograd.grad(loss, tensors)
            with torch.no_grad():
                for v, gr, a, dd in zip(tensors, grads, accum, decay):
                    a.mul_(mom).add_(gr + dd * v)
                    v.sub_(lr * a)
            return loss

        def ours_moving():
            moving.step(feats, offsets, labels, lr, global_step=0)

        def ours_batch():
            batch.step(feats, offsets, labels, lr, global_step=0)

        # agreement at this size: the parameters after one step of the batch mode and of torch in training mode
        ours_batch()
        eager()
        after = batch.variables()
        agree = {}
        for name, v in zip(names, tensors):
            if name.endswith("/bias") and not name.startswith("softmax/"):
                continue                     # in front of a batch norm in training mode: the exact gradient is zero, no update to judge by
            moved = float(np.max(np.abs(after[name] - start[name])))
            agree[name] = float(np.max(np.abs(after[name] - v.detach().cpu().numpy()))) / max(moved, 1e-30)
        for _ in range(args.warmup):
            ours_moving()
            ours_batch()
            eager()
        torch.cuda.synchronize()
        ms = dict(moving=[], batch=[], torch=[])
        for _ in range(args.rounds):
            ms["moving"].append(window_ms(ours_moving, torch, args.iters))
            ms["batch"].append(window_ms(ours_batch, torch, args.iters))
            ms["torch"].append(window_ms(eager, torch, args.iters))
        stage = {}
        for name, ct in (("moving", moving), ("batch", batch)):
            marked_step(ct, feats, offsets, labels, lr, torch)
            per = np.array([marked_step(ct, feats, offsets, labels, lr, torch) for _ in range(args.iters)])
            stage[name] = {s: float(np.median(per[:, i])) for i, s in enumerate(STAGES)}
        # the two redundant passes as bytes: the scratch y of every layer's z-only forward (one write of [rows, N]) and the
        # pass-through mask of every layer's backward (reads gz and z, writes gz)
        rows, elems = t, 0
        for w, (_, _, _, _, cout) in zip(WIDTHS, shapes[:5]):
            rows -= w - 1
            elems += b * rows * cout
        elems += b * (h + e)
        big = out["ops"][0]
        rate = 0.5 * (big["forward_gb_per_s"] + big["backward_gb_per_s"]) * 1e6          # bytes per millisecond
        out["step"] = dict(segments=b, frames=t, dim=d, channels=ch, pool=p, nodes=h, embed=e, classes=c, step_ms=ms,
                           step_ms_median={k: med(v) for k, v in ms.items()}, batch_over_moving=med(ms["batch"]) / med(ms["moving"]),
                           stage_ms_median=stage, stage_difference_ms={s: stage["batch"][s] - stage["moving"][s] for s in STAGES},
                           first_step_difference_over_update=agree, activations=elems,
                           scratch_y_bytes=4 * elems, scratch_y_ms_estimate=4 * elems / rate,
                           pass_through_mask_bytes=12 * elems, pass_through_mask_ms_estimate=12 * elems / rate,
                           estimate_rate_gb_per_s=rate / 1e6)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
