"""Timing of back-end training (csrc/backend.hip + tf_kaldi_speaker_amd/backend.py) on one MI355X at the size of a recipe:

  lda    scatter_stats of 1.2 M x 512 rows of 7 k speakers, then lda_from_stats --dim 200
  plda   scatter_stats of 1.2 M x 200 rows of the same speakers, then plda_from_stats with 10 EM iterations
  numpy  the same statistics (class means, total and between-class scatter) in numpy float64 on the host's threads, on
         --numpy-rows rows (default: all), scaled to the full set in `numpy_s_scaled`

scatter_stats is timed as a user sees it (wall clock around the call, rows already on the device, results on the host); the
Gram kernel alone is timed with events (`gram_s`, and `gram_tflops` = 2 n d^2 / time: the useful rate, the mirror half is not
counted twice).  A record, not a gate.  Prints one JSON line; profiles/backend.md keeps the numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def numpy_stats(x, labels, s):
    x = x.astype(np.float64)
    counts = np.bincount(labels, minlength=s).astype(np.float64)
    order = np.argsort(labels, kind="stable")
    sums = np.add.reduceat(x[order], np.concatenate([[0], np.cumsum(counts[:-1].astype(np.int64))]), axis=0)
    means = sums / counts[:, None]
    mean = x.mean(axis=0)
    y, m = x - mean, means - mean
    return y.T @ y, (m * counts[:, None]).T @ m


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1200000)
    ap.add_argument("--speakers", type=int, default=7000)
    ap.add_argument("--numpy-rows", type=int, default=0, help="rows of the numpy leg (0: all)")
    ap.add_argument("--em-iters", type=int, default=10)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from tf_kaldi_speaker_amd import _lib, backend
    lib = _lib.load()
    rng = np.random.default_rng(1)
    n, s = args.rows, args.speakers
    labels = np.sort(rng.integers(0, s, n))
    labels[:s] = np.arange(s)                      # every speaker has a row
    labels = np.sort(labels)
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "speakers": s, "cases": []}
    for d, lda_dim in ((512, 200), (200, 0)):
        spk = torch.randn((s, d), device="cuda:0")
        x = (spk[torch.from_numpy(labels).to("cuda:0")] * 0.7 + torch.randn((n, d), device="cuda:0")).contiguous()
        torch.cuda.synchronize()
        case = {"d": d}
        backend.scatter_stats(x[:4096], labels[:4096])                       # warm-up
        t0 = time.perf_counter()
        stats = backend.scatter_stats(x, labels)
        case["scatter_stats_s"] = time.perf_counter() - t0
        need = lib.xv_gram_f64_workspace(n, d)
        ws = torch.empty((max(need, 8) // 8,), dtype=torch.float64, device="cuda:0")
        gm = torch.empty((d, d), dtype=torch.float64, device="cuda:0")
        cd = torch.from_numpy(stats.mean).to("cuda:0")
        P = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
        run = lambda: _lib.check(lib.xv_gram_f64(0, P(x), d, n, d, P(cd), None, P(gm), P(ws), need, None))   # noqa: E731
        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            run()
        e1.record()
        e1.synchronize()
        case["gram_s"] = e0.elapsed_time(e1) * 1e-3 / 3
        case["gram_tflops"] = 2.0 * n * d * d / case["gram_s"] * 1e-12
        t0 = time.perf_counter()
        if lda_dim:
            backend.lda_from_stats(stats, dim=lda_dim)
            case["lda_from_stats_s"] = time.perf_counter() - t0
        else:
            backend.plda_from_stats(stats, args.em_iters)
            case["plda_from_stats_s"] = time.perf_counter() - t0
            case["em_iters"] = args.em_iters
            case["distinct_counts"] = int(np.unique(stats.counts).size)
        rows = args.numpy_rows or n
        xh = x[:rows].cpu().numpy()
        t0 = time.perf_counter()
        numpy_stats(xh, labels[:rows] - labels[0], int(labels[rows - 1] - labels[0]) + 1)
        case["numpy_rows"] = rows
        case["numpy_s"] = time.perf_counter() - t0
        case["numpy_s_scaled"] = case["numpy_s"] * n / rows
        out["cases"].append(case)
        del x, spk
    print(json.dumps(out))


if __name__ == "__main__":
    main()
