"""Timing of the cosine scoring kernels (csrc/score.hip) on one MI355X, 512-dimensional vectors:

  pairs      0.5 M trials over 145 k rows (xv_score_pairs)            beside torch gather + row-wise dot product
  matrix     8192 x 8192 scores (xv_score_matrix)                     beside torch.matmul in fp32
  self-hist  all pairs i < j of n = 16 384, 65 536, 145 000 rows      beside torch.matmul (+ torch.histc on the masked
             (xv_score_histogram; 65 536 bins = one 64-bit global      result at n = 16 384; matmul alone at 65 536, 17 GB;
             atomic per score, 8192 bins = counts in LDS)              nothing at 145 000: the matrix would be 84 GB)
  numpy      the reference-shaped host loop (misc/utils.py:318-327) at n = 1000

  --plda     instead of the above: the PLDA entry points (xv_plda_matrix / _pairs / _histogram / _prepare) beside the cosine
             entry point of the same (n, m, K), D = 200 and 512, enrolment sets of uniform and of mixed num_utts

  --snorm    instead of the above: cohort statistics for score normalisation (xv_cohort_stats): --snorm-rows rows (40 000)
             against a cohort of --snorm-cohort (10 000), top-300 and top_k = 0, cosine and PLDA operands, at several workspace
             sizes, beside xv_score_matrix alone and beside torch.matmul + torch.topk + mean / std of the same shape;
             `panel_gbytes_per_s` counts the panel written once and read once (rows of up to 12 288 scores are swept in LDS)

  --topk     instead of the above: identification (xv_score_topk): --topk-queries queries (10 000) against a gallery of
             --topk-gallery rows (1 000 000), d = --topk-dim (200), K = 10 and K = 300, cosine, at several workspace sizes,
             beside the only way without it: xv_score_matrix over row chunks (a chunk buffer of the same bytes as the
             workspace) and torch.topk on every chunk.  The two alternate in one process; medians of --topk-repeats runs

Device times are hipEvent times around repeated calls of one entry point (warmed up, at least --seconds of work each); the
host-side setup of scoring.py (uploads, label coding) is outside them.  Rates: useful FLOP = 2 d per score (the self
histogram computes n (n - 1) / 2 scores, plus the lower halves of the diagonal tiles, which are not counted); `of_peak` is
that rate over the 155 TFLOP/s measured fp32-matrix peak.  Prints one JSON line; profiles/scoring.md keeps the numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MATRIX = 155e12


def timed(torch, fn, seconds, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    iters, total = 0, 0.0
    while total < seconds * 1e3 and iters < 200:
        n = max(1, min(50, iters))          # growing batches between two events
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1)
        iters += n
    return total / iters * 1e-3, iters


def plda_leg(args, torch, lib, _lib, scoring):
    """xv_plda_* beside the cosine twin of the same (n, m, K), in one process, the two alternating case by case."""
    from tf_kaldi_speaker_amd import plda
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    rng = np.random.default_rng(3)
    n, m, k_pairs, nbins = args.plda_rows, args.plda_rows, 500000, 8192
    out = {"device": torch.cuda.get_device_name(0), "n": n, "m": m, "trials": k_pairs, "nbins": nbins, "cases": []}
    for d in (200, 512):
        q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        psi = np.sort(np.exp(rng.uniform(np.log(1e-3), np.log(1e2), d)))[::-1].copy()
        model = plda.Plda(0.1 * rng.standard_normal(d), q, psi)
        spk = rng.integers(0, max(2, n // 116), n + m)
        cent = rng.standard_normal((max(2, n // 116), d)) * np.sqrt(psi)[None, :]
        x = (cent[spk] + rng.standard_normal((n + m, d))).astype(np.float32) @ q.astype(np.float32) + model.mean.astype(np.float32)
        xd = torch.from_numpy(x).to(dev)
        lab = torch.from_numpy(spk.astype(np.int32)).to(dev)
        ia = torch.from_numpy(rng.integers(0, n, k_pairs).astype(np.int32)).to(dev)
        ib = torch.from_numpy(rng.integers(0, m, k_pairs).astype(np.int32)).to(dev)
        for kind in ("uniform", "mixed"):
            counts = None if kind == "uniform" else rng.integers(1, 31, n)
            e = plda.prepare_enroll(model, xd[:n], num_utts=counts)
            t = plda.prepare_test(model, xd[n:])
            k = e.k
            tau = t.tau(e.uniform_n) if e.uniform_n is not None else None
            ptau = None if tau is None else P(tau)
            lda, ldb = e.packed.shape[1], t.packed.shape[1]
            # the cosine twin: prepared (unit) rows of length K with the same leading dimensions
            ca = scoring.prepare(torch.randn((n, lda), device=dev)[:, :k].contiguous(), as_tensor=True)
            cb = scoring.prepare(torch.randn((m, ldb), device=dev)[:, :k].contiguous(), as_tensor=True)
            mat = torch.empty((n, m), device=dev)
            sc = torch.empty((k_pairs,), device=dev)
            h = torch.zeros((2, nbins), dtype=torch.int64, device=dev)
            hs, hd = C.c_void_p(h.data_ptr()), C.c_void_p(h.data_ptr() + 8 * nbins)
            s_all = plda.llr_matrix(e, t, as_tensor=True)
            lo, hi = float(s_all.min()), float(s_all.max()) + 1.0
            del s_all
            row = {"d": d, "num_utts": kind, "k": k}
            calls = {
                "matrix": (lambda: lib.xv_plda_matrix(0, P(e.packed), lda, n, P(e.bias), P(t.packed), ldb, m, ptau, k, P(mat), m, stream),
                           lambda: lib.xv_score_matrix(0, P(ca), k, n, P(cb), k, m, k, P(mat), m, stream)),
                "pairs": (lambda: lib.xv_plda_pairs(0, P(e.packed), lda, n, P(e.bias), P(t.packed), ldb, m, ptau, k, P(ia), P(ib), k_pairs, P(sc), stream),
                          lambda: lib.xv_score_pairs(0, P(ca), k, n, P(cb), k, m, k, P(ia), P(ib), k_pairs, P(sc), stream)),
                "histogram": (lambda: lib.xv_plda_histogram(0, P(e.packed), lda, n, P(e.bias), P(lab[:n]), P(t.packed), ldb, m, ptau, P(lab[n:]), k,
                                                            lo, hi, nbins, hs, hd, stream),
                              lambda: lib.xv_score_histogram(0, P(ca), k, n, P(lab[:n]), P(cb), k, m, P(lab[n:]), k, 0, nbins, hs, hd, stream)),
            }
            for name, (f_plda, f_cos) in calls.items():
                tp, it = timed(torch, lambda: _lib.check(f_plda()), args.seconds)
                tc, _ = timed(torch, lambda: _lib.check(f_cos()), args.seconds)
                tp2, _ = timed(torch, lambda: _lib.check(f_plda()), args.seconds)       # once more: the spread of one box
                row[name] = {"plda_ms": tp * 1e3, "plda_again_ms": tp2 * 1e3, "cosine_ms": tc * 1e3, "ratio": min(tp, tp2) / tc, "iters": it}
            # prepare: affine product + row kernel, beside xv_score_prepare with the same [d, d + 1] transform and length norm
            aff = plda._affine(model, 0, torch)
            tp, _ = timed(torch, lambda: plda.prepare_test(model, xd[n:]), args.seconds)
            tc, _ = timed(torch, lambda: scoring.prepare(xd[n:], transform=aff, as_tensor=True), args.seconds)
            row["prepare_python"] = {"plda_ms": tp * 1e3, "cosine_ms": tc * 1e3, "ratio": tp / tc, "rows": m}
            out["cases"].append(row)
            del e, t, ca, cb, mat, sc, h
            torch.cuda.empty_cache()
    print(json.dumps(out))


def snorm_leg(args, torch, lib, _lib, scoring):
    """xv_cohort_stats over prepared rows, and over PLDA-shaped operands (both biases), beside the stand-ins of torch."""
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    n, m, d = args.snorm_rows, args.snorm_cohort, args.dim
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    a = scoring.prepare(torch.randn((n, d), device=dev, generator=gen), as_tensor=True)
    b = scoring.prepare(torch.randn((m, d), device=dev, generator=gen), as_tensor=True)
    rho, tau = torch.randn((n,), device=dev, generator=gen), torch.randn((m,), device=dev, generator=gen)
    mean, std = torch.empty((n,), device=dev), torch.empty((n,), device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    least = int(lib.xv_cohort_stats_workspace(n, m, 0))
    whole = (n + 127) // 128 * least
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "cohort": m, "dim": d, "workspace_least_bytes": least, "cases": []}
    mat = torch.empty((n, m), device=dev)
    t, _ = timed(torch, lambda: _lib.check(lib.xv_score_matrix(0, P(a), d, n, P(b), d, m, d, P(mat), m, stream)), args.seconds)
    out["score_matrix_alone_ms"] = t * 1e3
    del mat
    sizes = sorted(set(min(w, whole) for w in (least, 16 * least, 64 << 20, 256 << 20, whole) if w >= least))
    for kind in ("cosine", "plda"):
        rb, cb = (None, None) if kind == "cosine" else (P(rho), P(tau))
        for top_k in (300, 0):
            row = {"kind": kind, "top_k": top_k, "workspace": []}
            for w in sizes:
                ws = torch.empty((w,), dtype=torch.uint8, device=dev)
                t, it = timed(torch, lambda: _lib.check(lib.xv_cohort_stats(0, P(a), d, n, rb, None, P(b), d, m, cb, None, d, top_k, P(mean),
                                                                            P(std), P(cnt), P(ws), w, stream)), args.seconds)
                row["workspace"].append({"bytes": w, "ms": t * 1e3, "iters": it, "tflops": 2.0 * n * m * d / t / 1e12,
                                         "panel_gbytes_per_s": 2.0 * n * m * 4 / t / 1e9})
                del ws
            got_mean, got_std = mean.clone(), std.clone()

            def standin():
                s = torch.matmul(a, b.t())
                if kind == "plda":
                    s = s + rho[:, None] + tau[None, :]
                v = torch.topk(s, top_k, dim=1).values if top_k else s
                return v.mean(1), v.std(1, unbiased=False)
            t, _ = timed(torch, standin, args.seconds, warmup=1)
            tm, ts = standin()
            row["torch_matmul_topk_ms"] = t * 1e3
            row["max_abs_diff_mean_vs_torch"] = float((got_mean - tm).abs().max())
            row["max_abs_diff_std_vs_torch"] = float((got_std - ts).abs().max())
            out["cases"].append(row)
            torch.cuda.empty_cache()
    print(json.dumps(out))


def topk_leg(args, torch, lib, _lib, scoring):
    """xv_score_topk beside xv_score_matrix in row chunks + torch.topk per chunk, same operands, same scratch bytes."""
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    n, m, d = args.topk_queries, args.topk_gallery, args.topk_dim
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)
    a = scoring.prepare(torch.randn((n, d), device=dev, generator=gen), as_tensor=True)
    b = scoring.prepare(torch.randn((m, d), device=dev, generator=gen), as_tensor=True)
    least = int(lib.xv_score_topk_workspace(n, m, 10))
    per_row = least // 128
    whole = (n + 127) // 128 * least
    out = {"device": torch.cuda.get_device_name(0), "queries": n, "gallery": m, "dim": d, "workspace_least_bytes": least,
           "repeats": args.topk_repeats, "cases": []}

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for top_k in (10, 300):
        sc = torch.empty((n, top_k), device=dev)
        ix = torch.empty((n, top_k), dtype=torch.int32, device=dev)
        cnt = torch.empty((n,), dtype=torch.int32, device=dev)
        tv = torch.empty((n, top_k), device=dev)
        ti = torch.empty((n, top_k), dtype=torch.int64, device=dev)
        row = {"top_k": top_k, "workspace": []}
        for w in sorted(set(min(f * least, whole) for f in (1, 4, 8))):
            ws = torch.empty((w,), dtype=torch.uint8, device=dev)
            chunk_rows = w // per_row                                     # the rows xv_score_topk takes per launch
            chunk = ws.view(torch.float32)[:chunk_rows * (per_row // 4)].view(chunk_rows, per_row // 4)

            def ours():
                _lib.check(lib.xv_score_topk(0, P(a), d, n, None, None, P(b), d, m, None, None, d, top_k, P(sc), P(ix), top_k, P(cnt),
                                             P(ws), w, stream))

            def chunked():
                for r0 in range(0, n, chunk_rows):
                    r = min(chunk_rows, n - r0)
                    _lib.check(lib.xv_score_matrix(0, C.c_void_p(a.data_ptr() + 4 * d * r0), d, r, P(b), d, m, d, P(chunk), per_row // 4, stream))
                    torch.topk(chunk[:r, :m], top_k, dim=1, out=(tv[r0:r0 + r], ti[r0:r0 + r]))
            ours()
            chunked()
            torch.cuda.synchronize()
            t_ours, t_chunk = [], []
            for _ in range(args.topk_repeats):                            # alternating: drift of the box hits both alike
                t_ours.append(once(ours))
                t_chunk.append(once(chunked))
            mo, mc = float(np.median(t_ours)), float(np.median(t_chunk))
            row["workspace"].append({"bytes": w, "rows_per_launch": chunk_rows, "score_topk_ms": mo, "score_topk_all_ms": t_ours,
                                     "matrix_chunks_torch_topk_ms": mc, "matrix_chunks_torch_topk_all_ms": t_chunk,
                                     "ratio_chunked_over_score_topk": mc / mo, "tflops": 2.0 * n * m * d / (mo * 1e-3) / 1e12,
                                     "values_equal": bool(torch.equal(sc, tv)),
                                     "indices_equal_fraction": float((ix.long() == ti).float().mean())})
            del ws, chunk
            torch.cuda.empty_cache()
        out["cases"].append(row)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="least device time per measurement")
    ap.add_argument("--sizes", type=str, default="16384,65536,145000", help="self-histogram row counts")
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--plda", action="store_true", help="time the PLDA entry points beside their cosine twins instead")
    ap.add_argument("--plda-rows", type=int, default=8192, help="rows on either side of the PLDA leg")
    ap.add_argument("--snorm", action="store_true", help="time the cohort statistics of score normalisation instead")
    ap.add_argument("--snorm-rows", type=int, default=40000)
    ap.add_argument("--snorm-cohort", type=int, default=10000)
    ap.add_argument("--topk", action="store_true", help="time identification (xv_score_topk) beside matrix chunks + torch.topk instead")
    ap.add_argument("--topk-queries", type=int, default=10000)
    ap.add_argument("--topk-gallery", type=int, default=1000000)
    ap.add_argument("--topk-dim", type=int, default=200)
    ap.add_argument("--topk-repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib, scoring
    if not torch.cuda.is_available():
        raise SystemExit("score_bench needs a GPU")
    lib = _lib.load()
    if args.plda:
        return plda_leg(args, torch, lib, _lib, scoring)
    if args.snorm:
        return snorm_leg(args, torch, lib, _lib, scoring)
    if args.topk:
        return topk_leg(args, torch, lib, _lib, scoring)
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    d = args.dim
    P = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    out = {"device": torch.cuda.get_device_name(0), "dim": d, "peak_f32_matrix_tflops": PEAK_F32_MATRIX / 1e12}

    def rows(n, speakers):
        """n prepared rows: speaker centroid + noise, like a validation set -> (rows, int32 labels)."""
        lab = torch.randint(0, speakers, (n,), device=dev, generator=gen, dtype=torch.int32)
        cent = torch.randn((speakers, d), device=dev, generator=gen)
        x = cent[lab.long()] + 2.0 * torch.randn((n, d), device=dev, generator=gen)
        return scoring.prepare(x, eps=1e-12, as_tensor=True), lab

    # ---- pairs
    n, k = 145000, 500000
    x, _ = rows(n, 1251)
    ia = torch.randint(0, n, (k,), device=dev, generator=gen, dtype=torch.int32)
    ib = torch.randint(0, n, (k,), device=dev, generator=gen, dtype=torch.int32)
    sc = torch.empty((k,), device=dev)
    t, it = timed(torch, lambda: _lib.check(lib.xv_score_pairs(0, P(x), d, n, P(x), d, n, d, P(ia), P(ib), k, P(sc), stream)), args.seconds)
    ial, ibl = ia.long(), ib.long()
    tt, _ = timed(torch, lambda: (x[ial] * x[ibl]).sum(1), args.seconds)
    ref = (x[ial].double() * x[ibl].double()).sum(1)
    out["pairs"] = {"rows": n, "trials": k, "ms": t * 1e3, "iters": it, "gbytes_per_s": k * 2 * d * 4 / t / 1e9,
                    "torch_gather_dot_ms": tt * 1e3, "max_abs_err_vs_f64": float((sc.double() - ref).abs().max())}
    del sc, ref

    # ---- matrix
    n = 8192
    a, b = x[:n], x[n:2 * n]
    m = torch.empty((n, n), device=dev)
    t, it = timed(torch, lambda: _lib.check(lib.xv_score_matrix(0, P(a), d, n, P(b), d, n, d, P(m), n, stream)), args.seconds)
    tt, _ = timed(torch, lambda: torch.matmul(a, b.t()), args.seconds)
    err = float((m - torch.matmul(a.double(), b.double().t()).float()).abs().max())
    out["matrix"] = {"n": n, "m": n, "ms": t * 1e3, "iters": it, "tflops": 2.0 * n * n * d / t / 1e12,
                     "of_peak": 2.0 * n * n * d / t / PEAK_F32_MATRIX, "torch_matmul_ms": tt * 1e3,
                     "torch_matmul_tflops": 2.0 * n * n * d / tt / 1e12, "max_abs_err_vs_f64": err}
    del m, x

    # ---- self histograms
    out["self_histogram"] = []
    for n in [int(s) for s in args.sizes.split(",") if s]:
        x, lab = rows(n, max(2, n // 116))          # ~116 utterances per speaker (VoxCeleb1-like)
        pairs = n * (n - 1) // 2
        row = {"n": n, "pairs": pairs}
        for nbins, name in ((65536, "global_atomics_65536"), (8192, "lds_8192")):
            h = torch.zeros((2, nbins), dtype=torch.int64, device=dev)

            def call():
                _lib.check(lib.xv_score_histogram(0, P(x), d, n, P(lab), P(x), d, n, P(lab), d, 1, nbins, C.c_void_p(h.data_ptr()),
                                                  C.c_void_p(h.data_ptr() + 8 * nbins), stream))
            t, it = timed(torch, call, args.seconds, warmup=1)
            assert int(h.sum().item()) == pairs * (it + 1), "histogram totals"
            eer, thr = scoring.eer_from_histograms(*h.cpu().numpy().view(np.uint64))
            row[name] = {"ms": t * 1e3, "iters": it, "tflops": 2.0 * pairs * d / t / 1e12,
                         "of_peak": 2.0 * pairs * d / t / PEAK_F32_MATRIX, "gscores_per_s": pairs / t / 1e9, "eer": eer}
        if n <= 65536:
            tt, _ = timed(torch, lambda: torch.matmul(x, x.t()), args.seconds, warmup=1)
            row["torch_matmul_full_ms"] = tt * 1e3
        if n <= 16384:
            same = lab[:, None] == lab[None, :]
            upper = torch.ones((n, n), dtype=torch.bool, device=dev).triu(1)
            ms, md = same & upper, (~same) & upper

            def standin():
                s = torch.matmul(x, x.t())
                return torch.histc(s[ms], 65536, -1.0, 1.0), torch.histc(s[md], 65536, -1.0, 1.0)
            tt, _ = timed(torch, standin, args.seconds, warmup=1)
            row["torch_matmul_histc_ms"] = tt * 1e3
            del same, upper, ms, md
        out["self_histogram"].append(row)
        del x, lab
        torch.cuda.empty_cache()

    # ---- the reference-shaped host loop at its own size limit
    n = 1000
    rng = np.random.default_rng(0)
    e = rng.standard_normal((n, d)).astype(np.float32)
    labels = rng.integers(0, 40, n)
    t0 = time.perf_counter()
    e = e / np.sqrt(np.sum(e ** 2, axis=1, keepdims=True) + 1e-12)
    mat = np.dot(e, e.T)
    scores, keys, idx = np.zeros(n * (n - 1) // 2), np.zeros(n * (n - 1) // 2), 0
    for i in range(n - 1):
        for j in range(i + 1, n):
            scores[idx] = mat[i, j]
            keys[idx] = 1 if labels[i] == labels[j] else 0
            idx += 1
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scoring.pairwise_eer(e, labels)
    t_gpu = time.perf_counter() - t0
    out["n1000"] = {"numpy_double_loop_ms": t_host * 1e3, "pairwise_eer_end_to_end_ms": t_gpu * 1e3}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
