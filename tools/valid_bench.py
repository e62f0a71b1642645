#!/usr/bin/env python
"""Time the fused classifier-head loss (csrc/loss.hip, through losses.ClassifierHead) beside
torch.nn.functional.cross_entropy(x @ W + b, labels) in fp32 on the same device, and set the kernel's workspace beside the
n * C * 4 bytes of the logit matrix it never writes.  The numbers of profiles/valid.md come from this tool:

    python tools/valid_bench.py [--n 4096] [--embed 512] [--classes 7185 100000] [--iters 20] [--warmup 3] [--device 0]

One JSON line per class count."""
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--classes", type=int, nargs="+", default=[7185, 100000])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
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
