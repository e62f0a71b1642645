#!/usr/bin/env python
"""Time the fused classifier-head loss (csrc/loss.hip, through losses.ClassifierHead) beside
torch.nn.functional.cross_entropy(x @ W + b, labels) in fp32 on the same device, and set the kernel's workspace beside the
n * C * 4 bytes of the logit matrix it never writes.  The numbers of profiles/valid.md come from this tool:

    python tools/valid_bench.py [--n 4096] [--embed 512] [--classes 7185 100000] [--iters 20] [--warmup 3] [--device 0]

One JSON line per class count.

    python tools/valid_bench.py --metric [--groups 1000] [--speakers 64] [--segments 10] [--embed 512] [--torch-chunk 25]

times the metric-learning heads (csrc/metric_loss.hip, through metric_losses.py: every group of the set in one call) beside the
same losses written in torch float64 on the same device (batched over chunks of groups: the [pairs, rows] mining tensors of
the triplet kinds would not fit otherwise), every kind, one JSON line each.  The parent of this path had no implementation to
compare with: torch float64 is the only baseline at hand."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, torch, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def torch_metric(kind, o, x, labels, torch):
    """The rules of include/xvec_hip.h (xv_metric_loss) in torch float64 for a chunk of equally sized groups:
    x [G, B, D] float32, labels [G, B] -> the group losses [G]."""
    inf = float("inf")
    xd = x.double()
    u = xd / torch.sqrt((xd * xd).sum(-1, keepdim=True).clamp_min(1e-12))
    G, B, _ = u.shape
    same = labels[:, :, None] == labels[:, None, :]
    eye = torch.eye(B, dtype=torch.bool, device=u.device)[None]
    pos, neg = same & ~eye, ~same
    if kind in ("softmax", "contrastive"):
        classes = int(labels.max()) + 1                         # the bench's labels are 0 .. speakers - 1
        onehot = torch.nn.functional.one_hot(labels.long(), classes).double()
        sums = torch.bmm(onehot.transpose(1, 2), u)
        chat = sums / torch.sqrt((sums * sums).sum(-1, keepdim=True).clamp_min(1e-12))
        sim = torch.bmm(u, chat.transpose(1, 2))
        e = torch.bmm(onehot, sums) - u
        e = e / torch.sqrt((e * e).sum(-1, keepdim=True).clamp_min(1e-12))
        own = (u * e).sum(-1)
        sim = torch.where(onehot.bool(), own[:, :, None], sim)
        z = o["w"] * sim + o["b"]
        z_own = o["w"] * own + o["b"]
        if kind == "softmax":
            return (torch.logsumexp(z, dim=2) - z_own).mean(1)
        other = torch.where(onehot.bool(), torch.zeros_like(z), torch.sigmoid(z)).amax(2)
        return (1.0 - torch.sigmoid(z_own) + other).mean(1)
    c = torch.bmm(u, u.transpose(1, 2))
    if kind == "semihard":
        n = torch.diagonal(c, dim1=1, dim2=2)
        d = torch.sqrt((n[:, :, None] - 2.0 * c + n[:, None, :]).clamp_min(0.0)).masked_fill(eye, 0.0)
        gi, ii, jj = pos.nonzero(as_tuple=True)
        dik, dij, nk = d[gi, ii], d[gi, ii, jj][:, None], neg[gi, ii]
        least = torch.where(nk & (dik > dij), dik, torch.full_like(dik, inf)).amin(1)
        z = torch.where(torch.isfinite(least), least, torch.where(nk, dik, torch.full_like(dik, -inf)).amax(1))
        terms = (o["margin"] + dij[:, 0] - z).clamp_min(0.0)
        return torch.zeros(G, dtype=torch.float64, device=u.device).index_add_(0, gi, terms) / pos.sum((1, 2)).clamp_min(1)
    c = c.clamp(-1.0, 1.0)
    pv = c - o["margin"]                                        # additive margin: the head the bench runs
    if kind == "hard":
        hp = torch.where(same, pv, torch.full_like(c, inf)).amin(2)
        hn = torch.where(neg, c, torch.full_like(c, -inf)).amax(2)
        return (hn - hp).clamp_min(0.0).mean(1)
    gi, ii, jj = pos.nonzero(as_tuple=True)
    t = c[gi, ii] - pv[gi, ii, jj][:, None]
    nk = neg[gi, ii]
    s = torch.zeros(G, dtype=torch.float64, device=u.device).index_add_(0, gi, (t.clamp_min(0.0) * nk).sum(1))
    a = torch.zeros(G, dtype=torch.float64, device=u.device).index_add_(0, gi, ((t > 1e-12) & nk).sum(1).double())
    return s / (a + 1e-16)


def metric_main(args):
    import torch
    from tf_kaldi_speaker_amd import metric_losses as ml
    if not torch.cuda.is_available():
        sys.exit("valid_bench needs a HIP device")
    dev = "cuda:%d" % args.device
    G, S, M, D = args.groups, args.speakers, args.segments, args.embed
    B = S * M
    gen = torch.Generator(device="cpu").manual_seed(7)
    spk = torch.randn((G, S, 1, D), generator=gen)
    x = (0.8 * spk + torch.randn((G, S, M, D), generator=gen)).reshape(G * B, D).to(dev)
    labels = torch.arange(S, dtype=torch.int32).repeat_interleave(M).repeat(G).to(dev)
    offsets = np.arange(G + 1, dtype=np.int64) * B
    kinds = [("semihard", dict(margin=0.2), lambda: ml.semihard_triplet_loss(x, labels, 0.2, offsets=offsets, device=args.device, as_tensor=True)),
             ("all", dict(margin=0.2), lambda: ml.angular_triplet_loss(x, labels, "additive_margin_softmax", 0.2, "all", offsets, args.device, True)),
             ("hard", dict(margin=0.2), lambda: ml.angular_triplet_loss(x, labels, "additive_margin_softmax", 0.2, "hard", offsets, args.device, True)),
             ("softmax", dict(w=20.0, b=0.0), lambda: ml.e2e_valid_loss(x, labels, offsets, args.device, True)),
             ("contrastive", dict(w=20.0, b=0.0), lambda: ml.ge2e_loss(x, labels, 20.0, 0.0, "contrastive", offsets, args.device, True))]
    chunk = max(1, min(args.torch_chunk, G))
    with torch.cuda.device(args.device):
        for kind, o, ours in kinds:
            def eager():
                return torch.cat([torch_metric(kind, o, x[g0 * B:(g0 + chunk) * B].view(-1, B, D), labels[g0 * B:(g0 + chunk) * B].view(-1, B), torch)
                                  for g0 in range(0, G, chunk)])
            hip = timed(ours, torch, args.warmup, args.iters)
            ref = timed(eager, torch, 1, max(1, args.iters // 5))
            diff = float((ours().group_loss - eager()).abs().max())
            print(json.dumps(dict(kind=kind, groups=G, rows_per_group=B, embed=D, hip_ms_median=hip[0], hip_ms_min=hip[1],
                                  torch_f64_ms_median=ref[0], torch_f64_ms_min=ref[1], torch_chunk_groups=chunk,
                                  max_abs_group_loss_diff=diff)), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--metric", action="store_true", help="time the metric-learning heads instead of the classifier head")
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--speakers", type=int, default=64)
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--torch-chunk", type=int, default=25, help="groups per batched torch evaluation")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--classes", type=int, nargs="+", default=[7185, 100000])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if args.metric:
        return metric_main(args)
    import torch
    from tf_kaldi_speaker_amd import _lib, losses
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("valid_bench needs a HIP device")
    lib = _lib.load()
    dev = "cuda:%d" % args.device
    params = Params(loss_func="softmax")
    for c in args.classes:
        g = torch.Generator(device="cpu").manual_seed(c)
        x = torch.randn((args.n, args.embed), generator=g).to(dev)
        w = (torch.randn((args.embed, c), generator=g) / np.sqrt(args.embed)).to(dev)
        b = (0.1 * torch.randn((c,), generator=g)).to(dev)
        labels = torch.randint(0, c, (args.n,), generator=g).to(dev)
        head = losses.ClassifierHead(w, b, params, device=args.device)
        with torch.cuda.device(args.device):
            fused = timed(lambda: head.loss(x, labels, as_tensor=True), torch, args.warmup, args.iters)
            eager = timed(lambda: torch.nn.functional.cross_entropy(x @ w + b, labels.long(), reduction="none"), torch,
                          args.warmup, args.iters)
            got = head.loss(x, labels, as_tensor=True).loss
            want = torch.nn.functional.cross_entropy((x.double() @ w.double() + b.double()), labels.long(), reduction="none")
            err = float((got.double() - want).abs().max())
        print(json.dumps(dict(n=args.n, embed=args.embed, classes=c, fused_ms_median=fused[0], fused_ms_min=fused[1],
                              torch_ms_median=eager[0], torch_ms_min=eager[1], workspace_bytes=int(lib.xv_loss_workspace(args.n, c)),
                              logit_bytes=args.n * c * 4, max_abs_diff_vs_fp64=err,
                              tflops_fused=2.0 * args.n * c * args.embed / (fused[0] * 1e-3) / 1e12)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
