#!/usr/bin/env python
"""Time the two attentive-pooling calls (xv_att_pool_forward / xv_att_pool_backward) on their own, beside torch fp32 autograd of
the same function on the same device and beside device-to-device copies (of the call's compulsory bytes, and of 1 GiB: the
achievable HBM rate as this process sees it); then one step of att_train.AttConvTrainer with its stages through `mark`, beside
the step of conv_train.ConvTrainer (statistics pooling) of the same build.  The numbers of profiles/att_train.md come from here:

    python tools/att_train_bench.py [--segments 64] [--frames 300] [--dim 1500] [--iters 100] [--step-iters 10] [--rounds 3]

64 segments of 300 frames leave 286 rows each behind the convolutions: 18 304 rows x 1500 columns of key and of value, H = 1
(both split) and H = 4 with the key split and the value not.  No time is gated.  Everything is timed in alternating rounds
inside one process, device events around back-to-back calls after warm-up calls of each; one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("frame_forward", "attention_forward", "pool_forward", "segment_forward", "head", "segment_backward", "pool_backward",
          "attention_backward", "frame_backward", "optimizer")


def window_ms(fn, torch, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def marked_step(tr, feats, offsets, labels, lr, torch, stages):
    ev = {s: torch.cuda.Event(enable_timing=True) for s in ("start",) + stages}
    tr.step(feats, offsets, labels, lr, global_step=0, mark=lambda s: s in ev and ev[s].record())
    ev["optimizer"].synchronize()
    borders = [ev["start"]] + [ev[s] for s in stages]
    return [borders[i].elapsed_time(borders[i + 1]) for i in range(len(stages))]


def operator(args, torch, lib, H, split_k, split_v):
    """The two calls at [segments x out_frames, dim] -> dict of medians and the bytes they must move."""
    from tf_kaldi_speaker_amd import _lib
    dev = "cuda:%d" % args.device
    b, t, D = args.segments, args.frames - 14, args.dim
    rows = b * t
    dq, dv = (D // H if split_k else D), (D // H if split_v else D)
    P = H * dv
    scale = float(np.float32(1.0 / np.sqrt(dq)))
    key, value = torch.randn((rows, D), device=dev), torch.relu(torch.randn((rows, D), device=dev))
    q = 0.1 * torch.randn((H, dq), device=dev)
    gp = torch.randn((b, 2 * P), device=dev)
    off = torch.arange(b + 1, dtype=torch.int32, device=dev) * t
    w, pooled, var = torch.empty((rows, H), device=dev), torch.empty((b, 2 * P), device=dev), torch.empty((b, P), device=dev)
    gk, gv, gq = torch.empty_like(key), torch.empty_like(value), torch.empty_like(q)
    ws = torch.empty(int(lib.xv_att_pool_workspace(b, rows, H, D, D, split_k, split_v)), dtype=torch.uint8, device=dev)
    p = lambda v: C.c_void_p(v.data_ptr())                                   # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(args.device).cuda_stream)
    common = (p(key), D, D, p(value), D, D, p(q), dq, H, split_k, split_v, C.c_float(scale), p(off), b, rows, p(w), H, p(pooled), 2 * P,
              p(var), P)

    def fwd():
        _lib.check(lib.xv_att_pool_forward(args.device, *common, stream))

    def bwd():
        _lib.check(lib.xv_att_pool_backward(args.device, p(gp), 2 * P, *common, p(gk), D, p(gv), D, p(gq), dq, p(ws), ws.numel(), stream))

    k3, v3 = key.view(b, t, D).clone().requires_grad_(True), value.view(b, t, D).clone().requires_grad_(True)
    qt = q.clone().requires_grad_(True)

    def torch_fwd():
        vh = v3.view(b, t, H, dv).permute(0, 2, 1, 3) if split_v else v3[:, None]
        kh = k3.view(b, t, H, dq).permute(0, 2, 1, 3) if split_k else k3[:, None]
        s = torch.einsum("bhld,hd->blh" if split_k else "bmld,hd->blh", kh, qt) * scale
        wt = torch.softmax(s.transpose(1, 2), dim=-1)
        mean = torch.einsum("bhld,bhl->bhd" if split_v else "bmld,bhl->bhd", vh, wt)
        vr = torch.einsum("bhld,bhl->bhd", (vh - mean[:, :, None, :]) ** 2, wt).reshape(b, -1)
        mask = (vr <= 1e-12).float().detach()
        return torch.cat([mean.reshape(b, -1), torch.sqrt((1.0 - mask) * vr + mask * 1e-12)], dim=1)

    def torch_both():
        torch.autograd.grad(torch_fwd(), (k3, v3, qt), gp)

    def torch_fwd_only():
        with torch.no_grad():
            torch_fwd()

    src = torch.empty(rows * D, device=dev)
    dst = torch.empty(2 * rows * D, device=dev)

    def copy_fwd():                                                          # the forward reads key and value once: 2 x, as a copy of x
        dst[:rows * D].copy_(src)

    def copy_bwd():                                                          # the backward reads both and writes both: 4 x
        dst[:rows * D].copy_(src)
        dst[rows * D:].copy_(src)

    fns = dict(forward=fwd, backward=bwd, torch_forward=torch_fwd_only, torch_forward_backward=torch_both, copy_2x=copy_fwd, copy_4x=copy_bwd)
    fwd()
    bwd()
    ours = pooled.clone()
    ref = torch_fwd().detach()
    agree = float((ours - ref).norm() / ref.norm())
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, f in fns.items():
            ms[k].append(window_ms(f, torch, args.iters))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    x = rows * D * 4
    fwd_bytes = 2 * x + 2 * rows * H * 4 * 2                                 # key and value once; the weights written, rewritten, read
    bwd_bytes = 4 * x + rows * H * 4 * 3                                     # key, value read; gkey, gvalue written; weights, gscore
    return dict(heads=H, split_key=split_k, split_value=split_v, rows=rows, dim=D, ms=ms, ms_median=med, x_bytes=x,
                forward_floor_bytes=fwd_bytes, backward_floor_bytes=bwd_bytes, pooled_relative_l2_against_torch=agree,
                forward_gbytes_per_s=fwd_bytes / (med["forward"] * 1e-3) / 1e9,
                backward_gbytes_per_s=bwd_bytes / (med["backward"] * 1e-3) / 1e9)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--dim", type=int, default=1500)
    ap.add_argument("--classes", type=int, default=7000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    from tf_kaldi_speaker_amd import _lib, att_train, conv_train, synth
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("att_train_bench needs a HIP device")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    lib = _lib.load()
    dev = "cuda:%d" % args.device
    out = dict(segments=args.segments, frames=args.frames, iters=args.iters, rounds=args.rounds)
    with torch.cuda.device(args.device):
        # the achievable HBM rate as a copy sees it: 1 GiB read + 1 GiB written, far beyond the 256 MiB of the last-level cache
        big_a, big_b = torch.empty(1 << 28, device=dev), torch.empty(1 << 28, device=dev)
        for _ in range(3):
            big_b.copy_(big_a)
        copy_ms = [window_ms(lambda: big_b.copy_(big_a), torch, 20) for _ in range(args.rounds)]
        out["copy_1gib_ms"] = copy_ms
        out["copy_gbytes_per_s"] = 2 * (1 << 30) / (float(np.median(copy_ms)) * 1e-3) / 1e9
        del big_a, big_b
        out["operator"] = [operator(args, torch, lib, 1, 1, 1), operator(args, torch, lib, 4, 1, 0)]

        # one step of the attention model beside the statistics-pooling model of the same build
        extra = dict(loss_func="softmax", optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=1e-4)
        rs = np.random.RandomState(3)
        b, t = args.segments, args.frames
        feats = torch.from_numpy(rs.standard_normal((b * t, 30)).astype(np.float32)).to(dev)
        offsets = np.arange(b + 1, dtype=np.int64) * t
        labels = torch.from_numpy(rs.randint(0, args.classes, b).astype(np.int32)).to(dev)
        steps = {}
        for name, base, cls in (("attention", synth.TDNN_ATT_PARAMS, att_train.AttConvTrainer),
                                ("statistics", synth.TDNN_STAT_PARAMS, conv_train.ConvTrainer)):
            params = dict(base, **extra)
            weights = synth.synth_weights(params, 30, seed=1)
            tr = cls(Params(**params), weights, args.classes, device=args.device, seed=1)
            stages = STAGES if name == "attention" else tuple(s for s in STAGES if not s.startswith("attention"))
            for _ in range(3):
                tr.step(feats, offsets, labels, 0.01, global_step=0)
            torch.cuda.synchronize()
            ms = [window_ms(lambda: tr.step(feats, offsets, labels, 0.01, global_step=0), torch, args.step_iters) for _ in range(args.rounds)]
            per = np.array([marked_step(tr, feats, offsets, labels, 0.01, torch, stages) for _ in range(args.step_iters)])
            steps[name] = dict(step_ms=ms, step_ms_median=float(np.median(ms)),
                               stage_ms_median={s: float(np.median(per[:, i])) for i, s in enumerate(stages)})
            del tr
        out["step"] = steps
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
