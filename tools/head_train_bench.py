#!/usr/bin/env python
"""Time one training step of a classifier head on frozen embeddings (head_train.HeadTrainer.step: one xv_loss_classifier_grad
and one xv_opt_step per tensor) beside the same head written in torch fp32 autograd on the same device, TF32 off: the forward,
cross_entropy, backward to the kernel and the bias, and a hand-written momentum update.  The numbers of profiles/head_train.md
come from this tool:

    python tools/head_train_bench.py [--n 512] [--embed 512] [--classes 7323] [--iters 3000] [--warmup 10] [--rounds 3]

No time is gated: the torch number is the context.  The two are timed in alternating rounds inside one process (other work
shares the host), device events around `iters` back-to-back steps (3000 steps of about 0.3 ms: a window of about a second),
one JSON line per head with every round's figure.  The gradients of the first step are compared with torch float64 at the
size that is timed."""
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


def torch_head(head, margin, fa, x, labels, w, b, torch):
    """The mean training loss of the head in torch, differentiable in w and b (softmax, additive_margin_softmax)."""
    if head == "softmax":
        return torch.nn.functional.cross_entropy(x @ w + b, labels)
    wh = w / torch.sqrt((w * w).sum(0, keepdim=True).clamp_min(1e-12))
    z = x @ wh
    fn = torch.sqrt((x * x).sum(1)).clamp_min(1e-12)
    sel = z.gather(1, labels[:, None])[:, 0]
    c = (sel / fn).clamp(-1.0 + 1e-12, 1.0 - 1e-12)
    t = (1.0 - fa) * sel + fa * ((c - margin) * fn)
    z = z.scatter(1, labels[:, None], t[:, None])
    return torch.nn.functional.cross_entropy(z, labels)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--classes", type=int, default=7323)
    ap.add_argument("--iters", type=int, default=3000, help="steps per timed window: about a second at the default size")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    from tf_kaldi_speaker_amd import _lib, head_train, losses
    from tf_kaldi_speaker_amd.params import Params
    if not torch.cuda.is_available():
        sys.exit("head_train_bench needs a HIP device")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    lib = _lib.load()
    dev = "cuda:%d" % args.device
    n, e, c = args.n, args.embed, args.classes
    g = torch.Generator(device="cpu").manual_seed(c)
    x = (torch.randn((n, e), generator=g) / np.sqrt(e) * 4.0).to(dev)
    labels = torch.randint(0, c, (n,), generator=g).to(dev)
    heads = [("softmax", dict(loss_func="softmax"), 0.0),
             ("additive_margin_softmax", dict(loss_func="additive_margin_softmax", amsoftmax_m=0.2, amsoftmax_lambda_min=0.0,
                                              amsoftmax_lambda_base=0.0, amsoftmax_lambda_gamma=0.0, amsoftmax_lambda_power=1.0), 0.2)]
    with torch.cuda.device(args.device):
        for name, extra, margin in heads:
            params = Params(optimizer="momentum", momentum=0.9, use_nesterov=False, weight_l2_regularizer=1e-4, **extra)
            fa = losses.head_config(params, 0, False)[3]
            ht = head_train.HeadTrainer(params, e, c, device=args.device, seed=1)
            w0 = torch.from_numpy(ht.kernel()).to(dev)
            # agreement at this size: the first step's gradients against torch float64
            res = ht.head.loss_and_grad(x, labels, need_grad_x=False, as_tensor=True)
            wd = w0.double().requires_grad_(True)
            bd = torch.zeros(c, dtype=torch.float64, device=dev, requires_grad=True)
            torch_head(name, margin, fa, x.double(), labels.long(), wd, bd, torch).backward()
            gk_err = float((res.grad_kernel.double() - wd.grad).abs().max() / wd.grad.abs().max())
            gb_err = None if res.grad_bias is None else float((res.grad_bias.double() - bd.grad).abs().max() / bd.grad.abs().max())

            w = w0.clone().requires_grad_(True)
            b = torch.zeros(c, device=dev, requires_grad=(name == "softmax"))
            tensors = [w, b] if name == "softmax" else [w]
            accum = [torch.zeros_like(t) for t in tensors]
            lab64 = labels.long()

            def ours():
                ht.step(x, labels, 0.01, global_step=0)

            def eager():
                loss = torch_head(name, margin, fa, x, lab64, w, b, torch)
                grads = torch.autograd.grad(loss, tensors)
                with torch.no_grad():
                    for t, gr, a, l2 in zip(tensors, grads, accum, (1e-4, 0.0)):
                        a.mul_(0.9).add_(gr + l2 * t)
                        t.sub_(0.01 * a)
                return loss

            for _ in range(args.warmup):
                ours()
                eager()
            torch.cuda.synchronize()
            hip_ms, torch_ms = [], []
            for _ in range(args.rounds):
                hip_ms.append(window_ms(ours, torch, args.iters))
                torch_ms.append(window_ms(eager, torch, args.iters))
            print(json.dumps(dict(head=name, n=n, embed=e, classes=c, iters=args.iters, hip_step_ms=hip_ms, torch_step_ms=torch_ms,
                                  hip_step_ms_median=float(np.median(hip_ms)), torch_step_ms_median=float(np.median(torch_ms)),
                                  grad_kernel_rel_err_vs_fp64=gk_err, grad_bias_rel_err_vs_fp64=gb_err,
                                  workspace_bytes=int(lib.xv_loss_grad_workspace(n, c, e)), logit_bytes=n * c * 4,
                                  note="HeadTrainer.step reads the mean loss back every step (one host synchronisation); "
                                       "the torch loop does not; two products: z and grad_kernel (grad_x is not asked for)",
                                  gemm_flops_two_products=2 * 2.0 * n * c * e,
                                  hip_tflops_two_products=2 * 2.0 * n * c * e / (float(np.median(hip_ms)) * 1e-3) / 1e12)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
