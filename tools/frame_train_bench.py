#!/usr/bin/env python
"""Time one training step of the trailing 1-tap frame layers, statistics pooling, the segment-level layers and the head on frozen
packed frames (frame_train.FrameTrainer.step) beside the same step written in torch fp32 autograd on the same device, TF32 off;
the two pooling kernels on their own beside a torch device-to-device copy that moves the same compulsory bytes; and the share of
the step each of its stages takes.  The numbers of profiles/frame_train.md come from this tool:

    python tools/frame_train_bench.py [--segments 64] [--frames 286] [--channels 512] [--pool 1500] [--nodes 512] [--embed 512]
                                      [--classes 7000] [--iters 20] [--warmup 3] [--rounds 3] [--pool-iters 200]

64 segments of 300 frames leave 286 rows each behind tdnn3_relu: 18 304 rows through 512 -> 512 -> 1500, pooling width 3000 ->
512 -> 512, 7000 classes, momentum.  No time is gated: the torch numbers are the context.  Everything is timed in alternating
rounds inside one process, device events around back-to-back calls after warm-up calls of each, one JSON line with every round's
figure.  The stages are timed on FrameTrainer.step itself, through its `mark` callback (a device event at every border): that
run reads the mean loss back like every step, after the last event.  The parameters after the first step are compared with the
torch step at the size that is timed."""
import argparse
import ctypes as C
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


STAGES = ("frame_forward", "pool_forward", "segment_forward", "head", "segment_backward", "pool_backward", "frame_backward", "optimizer")


def marked_step(ft, frames, offsets, labels, lr, torch):
    """One FrameTrainer.step(mark=...) with a device event at the marks of STAGES -> milliseconds per stage.  It is the step
    itself, so the mean loss is read back, after the last event."""
    ev = {stage: torch.cuda.Event(enable_timing=True) for stage in ("start",) + STAGES}
    ft.step(frames, offsets, labels, lr, global_step=0, mark=lambda stage: stage in ev and ev[stage].record())
    ev["optimizer"].synchronize()
    borders = [ev["start"]] + [ev[s] for s in STAGES]
    return [borders[i].elapsed_time(borders[i + 1]) for i in range(len(STAGES))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=286)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--pool", type=int, default=1500)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--classes", type=int, default=7000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pool-iters", type=int, default=200)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as fn
    from tf_kaldi_speaker_amd import _lib, frame_train
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("frame_train_bench needs a HIP device")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    lib = _lib.load()
    dev = "cuda:%d" % args.device
    b, t, ch, p, h, e, c = args.segments, args.frames, args.channels, args.pool, args.nodes, args.embed, args.classes
    rows = b * t
    rs = np.random.RandomState(c)
    dims = ((4, (ch, ch)), (5, (ch, p)), (6, (2 * p, h)), (7, (h, e)))
    weights = {}
    for idx, (k, n) in dims:
        lim = np.sqrt(6.0 / (k + n))
        weights["tdnn/tdnn%d_dense/kernel" % idx] = rs.uniform(-lim, lim, (k, n)).astype(np.float32)
        weights["tdnn/tdnn%d_dense/bias" % idx] = (0.1 * rs.standard_normal(n)).astype(np.float32)
        weights["tdnn/tdnn%d_bn/gamma" % idx] = rs.uniform(0.5, 1.5, n).astype(np.float32)
        weights["tdnn/tdnn%d_bn/beta" % idx] = (0.1 * rs.standard_normal(n)).astype(np.float32)
        weights["tdnn/tdnn%d_bn/moving_mean" % idx] = (0.1 * rs.standard_normal(n)).astype(np.float32)
        weights["tdnn/tdnn%d_bn/moving_variance" % idx] = rs.uniform(0.5, 1.5, n).astype(np.float32)
    frames = torch.from_numpy(np.maximum(rs.standard_normal((rows, ch)), 0.0).astype(np.float32)).to(dev)
    offsets = np.arange(b + 1, dtype=np.int64) * t
    labels = torch.from_numpy(rs.randint(0, c, b).astype(np.int32)).to(dev)
    lab64 = labels.long()
    l2, lr, mom = 1e-4, 0.01, 0.9
    params = Params(network_type="tdnn", loss_func="softmax", pooling_type="statistics_pooling", optimizer="momentum", momentum=mom,
                    use_nesterov=False, weight_l2_regularizer=l2)
    with torch.cuda.device(args.device):
        ft = frame_train.FrameTrainer(params, weights, c, device=args.device, seed=1)
        start = ft.variables()
        names = list(start)
        tensors = [torch.from_numpy(start[name]).to(dev).requires_grad_(True) for name in names]
        decay = [l2 if name.endswith("/kernel") else 0.0 for name in names]
        accum = [torch.zeros_like(v) for v in tensors]
        stats = [[torch.from_numpy(weights["tdnn/tdnn%d_bn/%s" % (idx, s)]).to(dev) for s in ("moving_mean", "moving_variance")]
                 for idx, _ in dims]

        def eager():
            y = frames
            for i in range(2):
                w, bias, g, be = tensors[4 * i:4 * i + 4]
                y = fn.relu(fn.batch_norm(y @ w + bias, stats[i][0], stats[i][1], g, be, training=False, eps=1e-3))
            y = y.view(b, t, p)
            mean = y.mean(dim=1, keepdim=True)
            var = ((y - mean) ** 2).mean(dim=1)
            mask = (var <= 1e-12).float().detach()
            y = torch.cat([mean.squeeze(1), torch.sqrt((1.0 - mask) * var + mask * 1e-12)], dim=1)
            for i in range(2, 4):
                w, bias, g, be = tensors[4 * i:4 * i + 4]
                y = fn.relu(fn.batch_norm(y @ w + bias, stats[i][0], stats[i][1], g, be, training=False, eps=1e-3))
            loss = fn.cross_entropy(y @ tensors[16] + tensors[17], lab64)
            grads = torch.autograd.grad(loss, tensors)
            with torch.no_grad():
                for v, gr, a, d in zip(tensors, grads, accum, decay):
                    a.mul_(mom).add_(gr + d * v)
                    v.sub_(lr * a)
            return loss

        def ours():
            ft.step(frames, offsets, labels, lr, global_step=0)

        # agreement at this size: the parameters after one step of each
        ours()
        eager()
        after = ft.variables()
        agree = {}
        for name, v in zip(names, tensors):
            moved = float(np.max(np.abs(after[name] - start[name])))
            agree[name] = float(np.max(np.abs(after[name] - v.detach().cpu().numpy()))) / max(moved, 1e-30)
        for _ in range(args.warmup):
            ours()
            eager()
        torch.cuda.synchronize()
        hip_ms, torch_ms = [], []
        for _ in range(args.rounds):
            hip_ms.append(window_ms(ours, torch, args.iters))
            torch_ms.append(window_ms(eager, torch, args.iters))

        # the stages of the step
        marked_step(ft, frames, offsets, labels, lr, torch)
        per = np.array([marked_step(ft, frames, offsets, labels, lr, torch) for _ in range(args.iters)])
        stage_ms = {s: float(np.median(per[:, i])) for i, s in enumerate(STAGES)}
        total = float(sum(stage_ms.values()))
        seg_share = (stage_ms["frame_forward"] + stage_ms["segment_forward"] + stage_ms["segment_backward"]
                     + stage_ms["frame_backward"]) / total

        # the two pooling kernels on their own, beside a copy of the same compulsory bytes
        x = torch.relu(torch.randn((rows, p), device=dev))
        gx = torch.empty_like(x)
        gp = torch.randn((b, 2 * p), device=dev)
        off = torch.from_numpy(offsets.astype(np.int32)).to(dev)
        pooled = torch.empty((b, 2 * p), device=dev)
        var = torch.empty((b, p), device=dev)
        ptr = lambda v: C.c_void_p(v.data_ptr())                            # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream(args.device).cuda_stream)

        def pool_fwd():
            _lib.check(lib.xv_stat_pool_forward(args.device, ptr(x), p, p, ptr(off), b, rows, ptr(pooled), 2 * p, ptr(var), p, stream))

        def pool_bwd():
            _lib.check(lib.xv_stat_pool_backward(args.device, ptr(gp), 2 * p, ptr(x), p, p, ptr(off), b, rows, ptr(pooled), 2 * p, ptr(var),
                                                 p, ptr(gx), p, stream))

        half = rows // 2
        dst = torch.empty_like(x)

        def copy_half():                                                    # reads rows / 2, writes rows / 2: the bytes of x once
            dst[:half].copy_(x[:half])

        def copy_all():                                                     # reads x, writes as much: the bytes of x and gx
            dst.copy_(x)

        for f in (pool_fwd, pool_bwd, copy_half, copy_all):
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        pool_ms = {k: [] for k in ("forward", "copy_x_once", "backward", "copy_x_and_gx")}
        for _ in range(args.rounds):
            pool_ms["forward"].append(window_ms(pool_fwd, torch, args.pool_iters))
            pool_ms["copy_x_once"].append(window_ms(copy_half, torch, args.pool_iters))
            pool_ms["backward"].append(window_ms(pool_bwd, torch, args.pool_iters))
            pool_ms["copy_x_and_gx"].append(window_ms(copy_all, torch, args.pool_iters))
    med = {k: float(np.median(v)) for k, v in pool_ms.items()}
    x_bytes = rows * p * 4
    print(json.dumps(dict(segments=b, frames=t, rows=rows, channels=ch, pool=p, nodes=h, embed=e, classes=c, iters=args.iters,
                          hip_step_ms=hip_ms, torch_step_ms=torch_ms, hip_step_ms_median=float(np.median(hip_ms)),
                          torch_step_ms_median=float(np.median(torch_ms)), first_step_difference_over_update=agree,
                          stage_ms_median=stage_ms, stage_sum_ms=total, seg_calls_share_of_step=seg_share,
                          pool_iters=args.pool_iters, pool_ms=pool_ms, pool_ms_median=med, x_bytes=x_bytes,
                          pool_forward_over_copy=med["forward"] / med["copy_x_once"],
                          pool_backward_over_copy=med["backward"] / med["copy_x_and_gx"],
                          pool_forward_gbytes_per_s=x_bytes / (med["forward"] * 1e-3) / 1e9,
                          pool_backward_gbytes_per_s=2 * x_bytes / (med["backward"] * 1e-3) / 1e9,
                          note="FrameTrainer.step reads the mean loss back every step (one host synchronisation) and waits once for "
                               "the label check; the torch loop does neither")), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
