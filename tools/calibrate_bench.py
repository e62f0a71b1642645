"""Timing of the calibration pass (csrc/calibrate.hip + tf_kaldi_speaker_amd/calibration.py) on one MI355X at the size of an
all-pairs trial list, N = 10^8 trials, for K = 1 and K = 4 systems:

  stats   one xv_logreg_stats call (both launches), scores on the device, timed with events: --warmup calls, then --repeats
          calls timed one by one; median, min and max.  `gbytes_per_s` counts the 4 K + 1 bytes per trial the pass must read.
  fit     calibration.fit as a user calls it (wall clock, scores and targets already on the device, result on the host),
          --fit-repeats times after one warm-up fit; with the number of Newton steps and of passes (line search included).
  torch   baseline 1: the same F, g and H written with torch float64 ops on the same GPU, events, same warm-up rule.
  numpy   baseline 2: the numpy oracle (tests/helpers/ref_calibration.py, pairwise sums) on the host at --numpy-rows trials
          (default 10^6), scaled by N / rows in `numpy_s_scaled`.

The scores are the recipe of the test fixtures (class means +-6, standard deviation 4 j for system j, 20 % targets) drawn on
the device from a seed.  The two GPU results are compared entry by entry before anything is timed.  A record, not a gate.
Prints one JSON line; profiles/calibration.md keeps the numbers."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))


def torch_stats(torch, s, t, theta, tau, c_tar, c_non):
    """F, g, H of include/xvec_hip.h in torch float64, element-wise ops and sums only (hipblasDgemv refused the [2^24, K + 1]
    products with HIPBLAS_STATUS_INTERNAL_ERROR, so no matmul); rows in chunks of 2^24, so that the temporaries stay a few GB."""
    k = s.shape[1]
    ct, cn = (torch.tensor(v, dtype=torch.float64, device=s.device) for v in (c_tar, c_non))
    F = torch.zeros((), dtype=torch.float64, device=s.device)
    g = torch.zeros((k + 1,), dtype=torch.float64, device=s.device)
    H = torch.zeros((k + 1, k + 1), dtype=torch.float64, device=s.device)
    for b in range(0, s.shape[0], 1 << 24):
        sb, tb = s[b:b + (1 << 24)], t[b:b + (1 << 24)] != 0
        cols = [sb[:, j].double() for j in range(k)] + [torch.ones((sb.shape[0],), dtype=torch.float64, device=s.device)]
        z = cols[0] * float(theta[0])
        for j in range(1, k):
            z = z + cols[j] * float(theta[j])
        z = z + (float(theta[k]) + tau)
        c = torch.where(tb, ct, cn)
        x = torch.where(tb, -z, z)
        F += (c * torch.nn.functional.softplus(x, threshold=1e30)).sum()
        r = c * torch.where(tb, -torch.sigmoid(-z), torch.sigmoid(z))
        w = c * torch.sigmoid(z) * torch.sigmoid(-z)
        for i in range(k + 1):
            g[i] += (r * cols[i]).sum()
            wi = w * cols[i]
            for j in range(i, k + 1):
                H[i, j] += (wi * cols[j]).sum()
                H[j, i] = H[i, j]
    return F, g, H


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
    ap.add_argument("--rows", type=int, default=100000000)
    ap.add_argument("--systems", default="1,4")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--fit-repeats", type=int, default=3)
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--numpy-rows", type=int, default=1000000)
    ap.add_argument("--prior", type=float, default=0.01)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    import ref_calibration as R
    from tf_kaldi_speaker_amd import _lib, calibration
    if not torch.cuda.is_available():
        raise SystemExit("calibrate_bench: no HIP device: nothing is measured")
    lib = _lib.load()
    n, prior = args.rows, args.prior
    tau = math.log(prior / (1.0 - prior))
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "prior": prior, "cases": []}
    P = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    for k in [int(v) for v in args.systems.split(",")]:
        gen = torch.Generator(device="cuda:0").manual_seed(100 + k)
        t = (torch.rand((n,), generator=gen, device="cuda:0") < 0.2).to(torch.uint8)
        t[0], t[1] = 1, 0
        s = torch.randn((n, k), generator=gen, device="cuda:0") * (4.0 * torch.arange(1, k + 1, device="cuda:0"))
        s += torch.where(t != 0, 6.0, -6.0)[:, None]
        n_tar = int(t.sum(dtype=torch.int64).item())
        c_tar, c_non = prior / n_tar, (1.0 - prior) / (n - n_tar)
        theta = np.concatenate([np.full(k, 1.0 / k), [0.0]])
        nd = 1 + (k + 1) + (k + 1) * (k + 2) // 2
        need = lib.xv_logreg_workspace(n, k)
        ws = torch.empty((max(need, 8),), dtype=torch.uint8, device="cuda:0")
        st = torch.empty((nd,), dtype=torch.float64, device="cuda:0")
        cnt = torch.empty((19,), dtype=torch.int64, device="cuda:0")
        run = lambda: _lib.check(lib.xv_logreg_stats(0, P(s), k, n, k, P(t), C.c_void_p(theta.ctypes.data), tau, c_tar, c_non,   # noqa: E731
                                                     None, 0, P(st), P(cnt), P(ws), need, None))
        case = {"k": k, "n_tar": n_tar, "workspace_bytes": int(need)}
        # the two GPU computations agree before either is timed
        run()
        F, gr, H = torch_stats(torch, s, t, theta, tau, c_tar, c_non)
        o = st.cpu().numpy()
        Hk = np.zeros((k + 1, k + 1))
        Hk[np.triu_indices(k + 1)] = o[k + 2:]
        Hk = Hk + np.triu(Hk, 1).T
        case["max_rel_diff_vs_torch"] = float(max(abs(o[0] - F.item()) / abs(F.item()),
                                                  np.max(np.abs(o[1:k + 2] - gr.cpu().numpy()) / np.abs(gr.cpu().numpy()).max()),
                                                  np.max(np.abs(Hk - H.cpu().numpy()) / np.abs(H.cpu().numpy()).max())))
        case["stats"] = timed(torch, run, args.warmup, args.repeats)
        case["stats"]["rows_per_s"] = n / case["stats"]["median_s"]
        case["stats"]["gbytes_per_s"] = n * (4 * k + 1) / case["stats"]["median_s"] * 1e-9
        case["torch"] = timed(torch, lambda: torch_stats(torch, s, t, theta, tau, c_tar, c_non), 1, args.torch_repeats)
        case["torch_over_stats"] = case["torch"]["median_s"] / case["stats"]["median_s"]
        # the whole fit
        calls = [0]
        inner = calibration._stats_dev

        def counting(*a, **kw):
            calls[0] += 1
            return inner(*a, **kw)
        calibration._stats_dev = counting
        try:
            calibration.fit(s, t, prior=prior)
            fits = []
            for _ in range(args.fit_repeats):
                calls[0] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model, report = calibration.fit(s, t, prior=prior)
                fits.append(time.perf_counter() - t0)
            fits.sort()
            case["fit"] = {"median_s": fits[len(fits) // 2], "min_s": fits[0], "max_s": fits[-1], "repeats": len(fits),
                           "newton_steps": report.iterations, "passes": calls[0], "F": report.F, "decrement": report.decrement,
                           "theta": model.theta.tolist()}
        except RuntimeError as e:                      # recorded, not hidden: the other legs are still worth having
            case["fit"] = {"error": str(e), "passes": calls[0]}
        finally:
            calibration._stats_dev = inner
        # the numpy oracle on the host
        rows = min(args.numpy_rows, n)
        sh, tn = s[:rows].cpu().numpy(), t[:rows].cpu().numpy() != 0
        f = R.objective(sh, tn, prior)
        f(theta)
        t0 = time.perf_counter()
        f(theta)
        case["numpy_rows"] = rows
        case["numpy_s"] = time.perf_counter() - t0
        case["numpy_s_scaled"] = case["numpy_s"] * n / rows
        out["cases"].append(case)
        del s, t, ws
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
