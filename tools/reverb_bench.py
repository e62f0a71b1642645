"""Timing of the reverberation pass (csrc/reverb.hip through tf_kaldi_speaker_amd.augment.reverberate_packed) on one MI355X:
--utts utterances (default 256) of --seconds (8) at 16 kHz, every one with its own impulse response of --taps (8000 and 16000)
taps and one additive signal of the utterance's length, as stage 2 of the recipes makes them.

  reverb   one xv_reverb call (all seven launches and the table copy), inputs and workspace on the device, timed with events:
           --warmup calls, then --repeats calls timed one by one; median, min and max.  `utt_per_s`; `gflops` counts the
           2 N L floating-point operations per utterance the direct form needs (the early-window pass, 2 N (e - s) more, is
           reported apart as `gflops_with_early`).
  torch    the same convolution alone (no early energy, no mixing, no scaling) with torch.fft on the same device: rfft of
           both operands at the next power of two above N + L - 1, product, irfft; same timing rule.
  numpy    the same FFT convolution in numpy float64 on one host core for --numpy-utts utterances, scaled to --utts.

The kernel's y is compared with the torch.fft result before anything is timed.  A record, not a gate: prints one JSON line;
profiles/augment.md keeps the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"median_s": ms[len(ms) // 2] * 1e-3, "min_s": ms[0] * 1e-3, "max_s": ms[-1] * 1e-3, "repeats": repeats}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--rate", type=int, default=16000)
    ap.add_argument("--taps", default="8000,16000")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--numpy-utts", type=int, default=4)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from tf_kaldi_speaker_amd import augment
    if not torch.cuda.is_available():
        raise SystemExit("reverb_bench: no HIP device: nothing is measured")
    dev = "cuda:0"
    B, N, fs = args.utts, int(args.seconds * args.rate), args.rate
    out = {"device": torch.cuda.get_device_name(0), "utts": B, "samples": N, "rate": fs, "tile": augment.tile(), "cases": []}
    for L in [int(v) for v in args.taps.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(1000 + L)
        x = (torch.randn((B, N), generator=gen, device=dev) * 3000.0).clamp(-32768, 32767).to(torch.int16)
        decay = torch.exp(-torch.arange(L, device=dev) / (L / 6.0))
        h = (torch.randn((B, L), generator=gen, device=dev) * 5000.0 * decay).clamp(-20000, 20000)
        h[:, 40] = 30000.0
        h = h.to(torch.int16)
        v = (torch.randn((B, N), generator=gen, device=dev) * 1500.0).clamp(-32768, 32767).to(torch.int16)
        utts = [{"wave": (i * N, N), "rir": (i * L, L), "noises": [(i * N, N, N, 10.0, 0.0)], "sample_rate": fs} for i in range(B)]
        need = augment.workspace_bytes(utts, B * N, B * L, B * N)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        o16 = torch.empty(B * N, dtype=torch.int16, device=dev)
        xf, hf, vf = x.reshape(-1), h.reshape(-1), v.reshape(-1)
        run = lambda **kw: augment.reverberate_packed(xf, utts, hf, vf, workspace=ws, out_i16=o16, **kw)      # noqa: E731
        nfft = 1 << int(np.ceil(np.log2(N + L - 1)))

        def fft_conv(rows=slice(None)):
            X = torch.fft.rfft(x[rows].float(), nfft)
            H = torch.fft.rfft(h[rows].float() / 32768.0, nfft)
            return torch.fft.irfft(X * H, nfft)[:, :N + L - 1]

        # the kernel's convolution against torch.fft's, before either is timed: no additive signal, no shift, no scaling
        plain = [{"wave": (i * N, N), "rir": (i * L, L), "sample_rate": fs, "shift_output": False, "normalize_output": False}
                 for i in range(4)]
        r = augment.reverberate_packed(xf, plain, hf, want_i16=False, want_f32=True)
        ref = fft_conv(slice(0, 4)).reshape(-1)
        case = {"taps": L, "workspace_bytes": int(need),
                "max_abs_diff_vs_torch_fft": float((r.out_f32 - ref).abs().max().item()),
                "rms_of_y": float(ref.square().mean().sqrt().item())}
        res = run()
        early = int(0.001 * fs) + int(0.05 * fs)
        case["clipped"] = int(res.clipped.sum())
        case["reverb"] = timed(torch, run, args.warmup, args.repeats)
        s = case["reverb"]["median_s"]
        case["reverb"]["utt_per_s"] = B / s
        case["reverb"]["gflops"] = 2.0 * N * L * B / s * 1e-9
        case["reverb"]["gflops_with_early"] = 2.0 * N * (L + early) * B / s * 1e-9
        case["torch_fft"] = timed(torch, fft_conv, args.warmup, args.repeats)
        case["torch_fft"]["utt_per_s"] = B / case["torch_fft"]["median_s"]
        case["torch_fft"]["nfft"] = nfft
        xh, hh = x[:args.numpy_utts].cpu().numpy().astype(np.float64), h[:args.numpy_utts].cpu().numpy().astype(np.float64) / 32768.0
        t0 = time.perf_counter()
        for i in range(args.numpy_utts):
            np.fft.irfft(np.fft.rfft(xh[i], nfft) * np.fft.rfft(hh[i], nfft), nfft)[:N + L - 1]
        dt = time.perf_counter() - t0
        case["numpy_fft"] = {"utts": args.numpy_utts, "seconds": dt, "utt_per_s": args.numpy_utts / dt}
        out["cases"].append(case)
        del x, h, v, ws, o16
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
