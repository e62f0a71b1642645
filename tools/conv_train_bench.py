#!/usr/bin/env python
"""Time one training step of the whole TDNN on packed features (conv_train.ConvTrainer.step: every frame-level layer through
xv_tconv_forward / xv_tconv_backward, statistics pooling, the segment-level layers, the head, one optimizer step per tensor)
beside the same step written in torch fp32 autograd (a conv1d stack) on the same device, TF32 off; the share of the step each of
its stages takes; each operator call of the three convolutions beside torch's conv1d forward and backward; and the new operator
at W = 1 beside xv_seg_forward / xv_seg_backward on the same operands.  The numbers of profiles/conv_train.md come from this tool:

    python tools/conv_train_bench.py [--segments 64] [--frames 300] [--dim 30] [--channels 512] [--pool 1500] [--nodes 512]
                                     [--embed 512] [--classes 7000] [--iters 20] [--warmup 3] [--rounds 3] [--op-iters 20]

No time is gated: the torch and xv_seg numbers are the context.  Everything is timed in alternating rounds inside one process,
device events around back-to-back calls after warm-up calls of each, one JSON line with every round's figure.  The stages and
the frame layers are timed on ConvTrainer.step itself, through its `mark` callback (a device event at every border): that run
reads the mean loss back like every step, after the last event.  The parameters after the first step are compared with the
torch step at the size that is timed."""
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
    """One ConvTrainer.step(mark=...) with a device event at every mark -> (milliseconds per stage, milliseconds of every frame
    layer forward and backward).  It is the step itself, so the mean loss is read back, after the last event."""
    n = len(ct.frame_layers)
    spare = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 2 * n + 1)]
    ev = {}

    def mark(stage):
        ev[stage] = spare.pop()
        ev[stage].record()
    ct.step(feats, offsets, labels, lr, global_step=0, mark=mark)
    ev["optimizer"].synchronize()
    borders = [ev["start"]] + [ev[s] for s in STAGES]
    fwd = [ev["start"]] + [ev["frame_forward/%d" % i] for i in range(n)]
    bwd = [ev["frame_backward/%d" % i] for i in range(n)] + [ev["pool_backward"]]
    return ([borders[i].elapsed_time(borders[i + 1]) for i in range(len(STAGES))], [fwd[i].elapsed_time(fwd[i + 1]) for i in range(n)],
            [bwd[i + 1].elapsed_time(bwd[i]) for i in range(n)])


def main(argv=None):
    ap = argparse.ArgumentParser()
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
    ap.add_argument("--op-iters", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as fn
    from tf_kaldi_speaker_amd import _lib, conv_train
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("conv_train_bench needs a HIP device")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    lib = _lib.load()
    dev = "cuda:%d" % args.device
    b, t, d, ch, p, h, e, c = args.segments, args.frames, args.dim, args.channels, args.pool, args.nodes, args.embed, args.classes
    rs = np.random.RandomState(c)
    weights, cin, frame_dims = {}, d, []
    for idx, w in enumerate(WIDTHS, start=1):
        cout = p if idx == len(WIDTHS) else ch
        frame_dims.append((idx, w, cin, cout))
        cin = cout
    shapes = [(idx, "conv" if w > 1 else "dense", (1, w, ci, co) if w > 1 else (ci, co), w * ci, co) for idx, w, ci, co in frame_dims]
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
    feats_nct = feats.view(b, t, d).permute(0, 2, 1).contiguous()          # torch's layout [B, C, T]
    offsets = np.arange(b + 1, dtype=np.int64) * t
    labels = torch.from_numpy(rs.randint(0, c, b).astype(np.int32)).to(dev)
    lab64 = labels.long()
    l2, lr, mom = 1e-4, 0.01, 0.9
    params = Params(network_type="tdnn", loss_func="softmax", pooling_type="statistics_pooling", optimizer="momentum", momentum=mom,
                    use_nesterov=False, weight_l2_regularizer=l2)
    ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())        # noqa: E731
    with torch.cuda.device(args.device):
        stream = C.c_void_p(torch.cuda.current_stream(args.device).cuda_stream)
        ct = conv_train.ConvTrainer(params, weights, c, device=args.device, seed=1)
        start = ct.variables()
        names = list(start)
        tensors = [torch.from_numpy(start[name]).to(dev).requires_grad_(True) for name in names]
        decay = [l2 if name.endswith("/kernel") else 0.0 for name in names]
        accum = [torch.zeros_like(v) for v in tensors]
        stats = [[torch.from_numpy(weights["tdnn/tdnn%d_bn/%s" % (idx, s)]).to(dev) for s in ("moving_mean", "moving_variance")]
                 for idx in range(1, 8)]

        def conv_weight(k):                                                 # TensorFlow [1, W, C, N] -> conv1d's [N, C, W]
            return k[0].permute(2, 1, 0) if k.dim() == 4 else k.t()[:, :, None]

        def eager():
            y = feats_nct
            for i in range(5):
                w, bias, g, be = tensors[4 * i:4 * i + 4]
                y = fn.relu(fn.batch_norm(fn.conv1d(y, conv_weight(w), bias), stats[i][0], stats[i][1], g, be, training=False, eps=1e-3))
            mean = y.mean(dim=2, keepdim=True)
            var = ((y - mean) ** 2).mean(dim=2)
            mask = (var <= 1e-12).float().detach()
            y = torch.cat([mean.squeeze(2), torch.sqrt((1.0 - mask) * var + mask * 1e-12)], dim=1)
            for i in range(5, 7):
                w, bias, g, be = tensors[4 * i:4 * i + 4]
                y = fn.relu(fn.batch_norm(y @ w + bias, stats[i][0], stats[i][1], g, be, training=False, eps=1e-3))
            loss = fn.cross_entropy(y @ tensors[28] + tensors[29], lab64)
            grads = torch.autograd.grad(loss, tensors)
            with torch.no_grad():
                for v, gr, a, dd in zip(tensors, grads, accum, decay):
                    a.mul_(mom).add_(gr + dd * v)
                    v.sub_(lr * a)
            return loss

        def ours():
            ct.step(feats, offsets, labels, lr, global_step=0)

        # agreement at this size: the parameters after one step of each
        ours()
        eager()
        after = ct.variables()
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

        # the stages of the step, and every frame layer on its own
        marked_step(ct, feats, offsets, labels, lr, torch)
        runs = [marked_step(ct, feats, offsets, labels, lr, torch) for _ in range(args.iters)]
        per = np.array([r[0] for r in runs])
        stage_ms = {s: float(np.median(per[:, i])) for i, s in enumerate(STAGES)}
        layer_fwd = np.median(np.array([r[1] for r in runs]), axis=0).tolist()
        layer_bwd = np.median(np.array([r[2] for r in runs]), axis=0).tolist()
        total = float(sum(stage_ms.values()))

        # each convolution beside torch's conv1d, forward and backward (weight, bias and, behind the first layer, input gradients)
        ops = []
        rows_in = t
        for i, (idx, w, ci, co) in enumerate(frame_dims[:3]):
            x = torch.relu(torch.randn((b, ci, rows_in), device=dev)).requires_grad_(i > 0)
            wt = torch.randn((co, ci, w), device=dev).mul_(0.05).requires_grad_(True)
            bt = torch.zeros((co,), device=dev, requires_grad=True)
            gy = torch.randn((b, co, rows_in - (w - 1)), device=dev)
            wanted = [wt, bt] + ([x] if i > 0 else [])

            def conv_f(x=x, wt=wt, bt=bt):
                return fn.conv1d(x, wt, bt)

            def conv_fb(x=x, wt=wt, bt=bt, gy=gy, wanted=wanted):
                torch.autograd.grad(fn.conv1d(x, wt, bt), wanted, gy)

            for f in (conv_f, conv_fb):
                for _ in range(3):
                    f()
            tf_ms, tfb_ms = [], []
            for _ in range(args.rounds):
                tf_ms.append(window_ms(conv_f, torch, args.op_iters))
                tfb_ms.append(window_ms(conv_fb, torch, args.op_iters))
            ops.append(dict(layer="tdnn%d" % idx, taps=w, cin=ci, cout=co, rows_in=b * rows_in, rows_out=b * (rows_in - (w - 1)),
                            xv_forward_ms=layer_fwd[i], xv_backward_ms=layer_bwd[i], torch_forward_ms=tf_ms,
                            torch_forward_backward_ms=tfb_ms, torch_forward_ms_median=float(np.median(tf_ms)),
                            torch_backward_ms_median=float(np.median(tfb_ms)) - float(np.median(tf_ms)),
                            gflop_forward=2.0 * b * (rows_in - (w - 1)) * w * ci * co / 1e9))
            rows_in -= w - 1

        # W = 1 beside the dense-layer calls on the same operands: rows x channels -> channels
        n1 = b * (t - sum(w - 1 for w in WIDTHS))
        x1 = torch.relu(torch.randn((n1, ch), device=dev))
        w1 = torch.randn((ch, ch), device=dev).mul_(0.05)
        vecs = [torch.rand((ch,), device=dev) + 0.5 for _ in range(4)]      # bias / gamma, beta, moving_mean, moving_variance > 0
        b1, bn1 = vecs[0], [vecs[1], vecs[2] - 1.0, vecs[3] - 1.0, vecs[0]]
        gy1 = torch.randn((n1, ch), device=dev)
        z1, y1, gx1 = (torch.empty((n1, ch), device=dev) for _ in range(3))
        gw1 = torch.empty((ch, ch), device=dev)
        gv = [torch.empty((ch,), device=dev) for _ in range(3)]
        off1 = torch.from_numpy((np.arange(b + 1) * (n1 // b)).astype(np.int32)).to(dev)
        ws_t = torch.empty(int(lib.xv_tconv_workspace(b, n1, n1, 1, ch, ch)), dtype=torch.uint8, device=dev)
        ws_s = torch.empty(int(lib.xv_seg_workspace(n1, ch, ch)), dtype=torch.uint8, device=dev)

        def tconv_f():
            _lib.check(lib.xv_tconv_forward(args.device, ptr(x1), ch, ch, 1, ptr(off1), b, n1, n1, ptr(w1), ch, ch, ptr(b1), ptr(bn1[0]),
                                            ptr(bn1[1]), ptr(bn1[2]), ptr(bn1[3]), 1, ptr(z1), ch, ptr(y1), ch, ptr(ws_t), ws_t.numel(),
                                            stream))

        def tconv_b():
            _lib.check(lib.xv_tconv_backward(args.device, ptr(gy1), ch, ptr(x1), ch, ch, 1, ptr(off1), b, n1, n1, ptr(z1), ch, ptr(w1), ch,
                                             ch, ptr(bn1[0]), ptr(bn1[1]), ptr(bn1[2]), ptr(bn1[3]), 1, ptr(gx1), ch, ptr(gw1), ptr(gv[0]),
                                             ptr(gv[1]), ptr(gv[2]), ptr(ws_t), ws_t.numel(), stream))

        def seg_f():
            _lib.check(lib.xv_seg_forward(args.device, ptr(x1), ch, n1, ch, ptr(w1), ch, ch, ptr(b1), ptr(bn1[0]), ptr(bn1[1]), ptr(bn1[2]),
                                          ptr(bn1[3]), 1, ptr(z1), ch, ptr(y1), ch, stream))

        def seg_b():
            _lib.check(lib.xv_seg_backward(args.device, ptr(gy1), ch, ptr(x1), ch, ptr(z1), ch, n1, ch, ptr(w1), ch, ch, ptr(bn1[0]),
                                           ptr(bn1[1]), ptr(bn1[2]), ptr(bn1[3]), 1, ptr(gx1), ch, ptr(gw1), ptr(gv[0]), ptr(gv[1]),
                                           ptr(gv[2]), ptr(ws_s), ws_s.numel(), stream))

        # the two backward calls give the same gradients (other summation orders): largest difference over the largest value
        seg_f()
        seg_b()
        ref = [v.clone() for v in (gx1, gw1, gv[0], gv[1], gv[2])]
        tconv_f()
        tconv_b()
        w1_diff = [float((a - r).abs().max() / r.abs().max()) for a, r in zip((gx1, gw1, gv[0], gv[1], gv[2]), ref)]
        for f in (tconv_f, tconv_b, seg_f, seg_b):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        w1_ms = {k: [] for k in ("tconv_forward", "seg_forward", "tconv_backward", "seg_backward")}
        for _ in range(args.rounds):
            w1_ms["tconv_forward"].append(window_ms(tconv_f, torch, args.op_iters))
            w1_ms["seg_forward"].append(window_ms(seg_f, torch, args.op_iters))
            w1_ms["tconv_backward"].append(window_ms(tconv_b, torch, args.op_iters))
            w1_ms["seg_backward"].append(window_ms(seg_b, torch, args.op_iters))
    print(json.dumps(dict(segments=b, frames=t, dim=d, channels=ch, pool=p, nodes=h, embed=e, classes=c, iters=args.iters,
                          hip_step_ms=hip_ms, torch_step_ms=torch_ms, hip_step_ms_median=float(np.median(hip_ms)),
                          torch_step_ms_median=float(np.median(torch_ms)), first_step_difference_over_update=agree,
                          stage_ms_median=stage_ms, stage_sum_ms=total, frame_layer_forward_ms=layer_fwd,
                          frame_layer_backward_ms=layer_bwd, conv_ops=ops, one_tap_rows=n1, one_tap_ms=w1_ms,
                          one_tap_ms_median={k: float(np.median(v)) for k, v in w1_ms.items()},
                          one_tap_gradient_difference=dict(zip(("gx", "gw", "gbias", "ggamma", "gbeta"), w1_diff)),
                          note="ConvTrainer.step reads the mean loss back every step (one host synchronisation) and uploads the "
                               "offsets of every layer; the torch loop does neither")), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
