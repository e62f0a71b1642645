#!/usr/bin/env python
"""Time one training step of the whole ResNet-18 on packed features (resnet_train.ResNetTrainer.step: every 2-D convolution
through xv_gconv_forward / xv_gconv_backward, the residual joins through xv_add_act_*, conv5 and the dense layers through
xv_tconv_*, statistics pooling, the segment-level layers, the head, one optimizer step per tensor) beside the same step written
in torch fp32 autograd (F.pad + conv2d, TensorFlow's 'same' placement) on the same device, TF32 off, in both batch-norm modes;
the share of the step each of its stages takes; every operator call (each layer's forward and backward, each join); the peak
device memory of a step; and the time a device-to-device copy of the bytes a step must move takes (the HBM yardstick).  The
numbers of profiles/resnet_train.md come from this tool:

    python tools/resnet_train_bench.py [--segments 64] [--frames 300] [--width 64] [--pool 1500] [--embed 512] [--classes 7000]
                                       [--iters 3] [--warmup 1] [--rounds 2] [--modes moving,batch]

The recipe's batch (egs/voxceleb/v3/nnet_conf/resnet18_softmax_1e-2.json) is 64 segments of 200 to 400 frames: 64 x 300, width
64.  No time is gated: torch's time and the copy are the context.  Everything is timed in alternating rounds inside one process,
device events around back-to-back calls after warm-up calls of each, one JSON line with every round's figure.  The stages and
the layers are timed on ResNetTrainer.step itself, through its `mark` callback (a device event at every mark): that run reads the
mean loss back like every step, after the last event.  The parameters after the first step are compared with the torch step
at the size that is timed (moving mode)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def marked_step(rt, feats, offsets, labels, lr, torch):
    """One ResNetTrainer.step(mark=...) with a device event at every mark -> (milliseconds per stage, {mark: milliseconds since
    the mark before it} for every layer and join).  It is the step itself, so the mean loss is read back, after the last event."""
    order, ev = [], {}

    def mark(stage):
        ev[stage] = torch.cuda.Event(enable_timing=True)
        ev[stage].record()
        order.append(stage)
    rt.step(feats, offsets, labels, lr, global_step=0, mark=mark)
    ev["optimizer"].synchronize()
    borders = [ev["start"]] + [ev[s] for s in STAGES]
    stages = [borders[i].elapsed_time(borders[i + 1]) for i in range(len(STAGES))]
    calls = {}
    for prev, cur in zip(order[:-1], order[1:]):
        if "/" in cur:
            calls[cur] = ev[prev].elapsed_time(ev[cur])
    return stages, calls


def same_pad(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--pool", type=int, default=1500)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--classes", type=int, default=7000)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", default="moving,batch")
    ap.add_argument("--time-stride", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as fn
    from tf_kaldi_speaker_amd import resnet_train, synth
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("resnet_train_bench needs a HIP device")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    dev = "cuda:%d" % args.device
    b, t, c = args.segments, args.frames, args.classes
    l2, lr, mom, bn_mom = 1e-4, 0.01, 0.9, 0.99
    pd = dict(synth.RESNET_PARAMS, num_nodes_pooling_layer=args.pool, num_nodes_last_layer=args.embed, optimizer="momentum", momentum=mom,
              use_nesterov=False, weight_l2_regularizer=l2, batchnorm_momentum=bn_mom, resnet_time_stride=bool(args.time_stride))
    weights = synth.synth_resnet_weights(pd, seed=1, width=args.width)
    rs = np.random.RandomState(c)
    feats = torch.from_numpy(rs.standard_normal((b * t, 40)).astype(np.float32)).to(dev)
    offsets = np.arange(b + 1, dtype=np.int64) * t
    labels = torch.from_numpy(rs.randint(0, c, b).astype(np.int32)).to(dev)
    lab64 = labels.long()
    specs, blocks = resnet_train.frame_variables(pd), resnet_train.block_plan(pd)
    seg = resnet_train.tail_train.segment_variables(pd)
    out = dict(segments=b, frames=t, width=args.width, pool=args.pool, embed=args.embed, classes=c, iters=args.iters,
               time_stride=bool(args.time_stride), modes={})
    with torch.cuda.device(args.device):
        # the HBM yardstick: a device-to-device copy, read + write
        buf = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(buf)
        for _ in range(3):
            dst.copy_(buf)
        copy_ms = float(np.median([window_ms(lambda: dst.copy_(buf), torch, 10) for _ in range(3)]))
        out["copy_gb_per_s"] = 2.0 * buf.numel() / copy_ms / 1e6
        del buf, dst
        for mode in [m for m in args.modes.split(",") if m]:
            batch = mode == "batch"
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            rt = resnet_train.ResNetTrainer(Params(**pd), weights, c, device=args.device, seed=1, batch_norm=mode)
            start = rt.variables()
            names = [n for n in start if "moving" not in n]
            T = {n: torch.from_numpy(start[n]).to(dev).requires_grad_(True) for n in names}
            tensors = [T[n] for n in names]
            decay = [float(rt.l2[n]) for n in names]
            accum = [torch.zeros_like(v) for v in tensors]
            R = {k: torch.from_numpy(np.asarray(v, dtype=np.float32).copy()).to(dev) for k, v in weights.items() if "moving" in k}

            def bn(z, scope, rank4):
                g, be, mm, mv = T[scope + "/gamma"], T[scope + "/beta"], R[scope + "/moving_mean"], R[scope + "/moving_variance"]
                if not batch:
                    return fn.batch_norm(z, mm, mv, g, be, False, 0.0, 1e-3)
                return fn.batch_norm(z, mm, mv, g, be, True, 1.0 - bn_mom, 1e-3)      # (the biased variance of rank < 4 not modelled)

            def conv(x, spec):
                kh, kw, st, sf = spec.window
                pt, pf = same_pad(x.shape[2], kh, st), same_pad(x.shape[3], kw, sf)
                z = fn.conv2d(fn.pad(x, pf + pt), T[spec.kernel].permute(3, 2, 0, 1), None, stride=(st, sf))
                z = bn(z, spec.bn, True)
                return torch.relu(z) if spec.act else z

            def eager():
                x = conv(feats.view(b, 1, t, 40), specs[0])
                i = 1
                for blk in blocks:
                    p = conv(conv(x, specs[i]), specs[i + 1])
                    q = conv(x, specs[i + 2]) if blk.shortcut else x
                    x = torch.relu(p + q)
                    i += 3 if blk.shortcut else 2
                y = x.permute(0, 2, 3, 1).reshape(b * x.shape[2], -1)             # [frames, 5 C], column f C + c
                frames = x.shape[2]
                for spec in specs[i:]:
                    k = T[spec.kernel]
                    y = torch.relu(bn(y @ k.reshape(-1, k.shape[-1]) + T[spec.bias], spec.bn, k.dim() == 4))
                y = y.view(b, frames, -1)
                mean = y.mean(dim=1, keepdim=True)
                var = ((y - mean) ** 2).mean(dim=1)
                mask = (var <= 1e-12).float().detach()
                y = torch.cat([mean.squeeze(1), torch.sqrt((1.0 - mask) * var + mask * 1e-12)], dim=1)
                for spec in seg:
                    y = torch.relu(bn(y @ T[spec.kernel] + T[spec.bias], spec.bn, False))
                loss = fn.cross_entropy(y @ T["softmax/output/kernel"] + T["softmax/output/bias"], lab64)
                grads = torch.autograd.grad(loss, tensors)
                with torch.no_grad():
                    for v, gr, a, dd in zip(tensors, grads, accum, decay):
                        a.mul_(mom).add_(gr + dd * v)
                        v.sub_(lr * a)
                return loss

            def ours():
                rt.step(feats, offsets, labels, lr, global_step=0)

            # agreement at this size: the parameters after one step of each, and the peak memory of that step
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ours()
            torch.cuda.synchronize()
            hip_peak = torch.cuda.max_memory_allocated() - base
            live = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            eager()
            torch.cuda.synchronize()
            torch_peak = torch.cuda.max_memory_allocated() - live
            after = rt.variables()
            agree = {}
            for name in names:
                moved = float(np.max(np.abs(after[name] - start[name])))
                agree[name] = float(np.max(np.abs(after[name] - T[name].detach().cpu().numpy()))) / max(moved, 1e-30)
            for _ in range(args.warmup):
                ours()
                eager()
            torch.cuda.synchronize()
            hip_ms, torch_ms = [], []
            for _ in range(args.rounds):
                hip_ms.append(window_ms(ours, torch, args.iters))
                torch_ms.append(window_ms(eager, torch, args.iters))
            runs = [marked_step(rt, feats, offsets, labels, lr, torch) for _ in range(args.iters)]
            per = np.array([r[0] for r in runs])
            stage_ms = {s: float(np.median(per[:, i])) for i, s in enumerate(STAGES)}
            calls = {k: float(np.median([r[1][k] for r in runs])) for k in runs[0][1]}
            layers = []
            for i, (spec, layer) in enumerate(zip(rt.frame_specs, rt.frame_layers)):
                x = layer._x
                rows_in, rows_out = int(x.shape[0]), int(layer._z.shape[0])
                layers.append(dict(index=i, kernel=spec.kernel, window=list(getattr(spec, "window", (1, 1, 1, 1))), K=layer.in_dim,
                                   N=layer.out_dim, rows_in=rows_in, rows_out=rows_out, forward_ms=calls.get("frame_forward/%d" % i),
                                   backward_ms=calls.get("frame_backward/%d" % i), gflop_forward=2.0 * rows_out * layer.in_dim * layer.out_dim / 1e9))
            joins = {k: v for k, v in calls.items() if k.startswith("join_")}
            gflop = 3.0 * sum(l["gflop_forward"] for l in layers)
            # what a step must move at the least: every layer reads x and writes z and y forward, reads gy, z and x and writes gx backward
            moved_bytes = 4.0 * sum(2 * l["rows_in"] * (l["K"] // (l["window"][0] * l["window"][1])) + 4 * l["rows_out"] * l["N"] for l in layers)
            worst = max(agree.values())
            out["modes"][mode] = dict(
                hip_step_ms=hip_ms, torch_step_ms=torch_ms, hip_step_ms_median=float(np.median(hip_ms)),
                torch_step_ms_median=float(np.median(torch_ms)), stage_ms_median=stage_ms, stage_sum_ms=float(sum(stage_ms.values())),
                layers=layers, joins_ms=joins, step_gflop=gflop, tflops=gflop / float(np.median(hip_ms)),
                hip_peak_bytes=int(hip_peak), torch_peak_bytes=int(torch_peak), moved_bytes_floor=moved_bytes,
                copy_of_moved_bytes_ms=moved_bytes / (out["copy_gb_per_s"] * 1e6),
                first_step_difference_over_update_max=worst if not batch else None,
                first_step_difference_over_update={k: v for k, v in agree.items() if v > 0.01} if not batch else None)
            del rt, T, tensors, accum, R
    out["note"] = ("ResNetTrainer.step reads the mean loss back every step (one host synchronisation) and uploads the offsets of "
                   "every layer; the torch loop does neither, and batches the equal-length segments into one conv2d per layer")
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
