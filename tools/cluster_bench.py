"""Timing of speaker clustering (xv_ahc, csrc/cluster.hip) on one MI355X, cosine scores of d = 128 rows:

  batch    --groups recordings (500) of n ~ U[200, 1000] rows in one call: the matrix fill (one xv_score_matrix per recording into
           the packed buffer) and the clustering, timed separately; no threshold, so every recording merges down to one cluster
           (the longest run the rule allows)
  single   one recording of --single rows (8192, the most a workgroup's LDS cache holds): one workgroup on one CU
  host     scipy.cluster.hierarchy.linkage(method="average") on the same matrices copied to the host (distance = max - score),
           when scipy imports: every recording of the batch and the single one; otherwise tests/helpers/ref_cluster.ahc on the
           --subset smallest recordings of the batch, and that is stated in the output.  With scipy the largest difference of
           the merge heights over the first --subset recordings is reported as well (tie-free data: the logs are comparable)

  --target-energy E   instead of the above: the per-recording PLDA adaptation (xv_plda_adapt, csrc/plda_adapt.hip) of the same
           batch plus the single recording in one call, at every --adapt-dims dimension (128 and 200): the time of xv_plda_adapt
           alone, of the whole cluster.plda call with and without the option (wall clock around a synchronised call), the sweeps
           the two Jacobi iterations needed, and the same adaptation by the float64 numpy oracle
           (tests/helpers/ref_plda_adapt.adapt, numpy.linalg.eigh) on the host, one recording after the other

Device times are hipEvent times around one call sequence, after a warm-up run of the same shapes; the working matrix is refilled
before every clustering run because xv_ahc consumes it.  --repeats runs each (3), all reported, the median quoted.  Prints one
JSON line; profiles/clustering.md keeps the numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=500)
    ap.add_argument("--single", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--subset", type=int, default=10, help="recordings compared in detail (and timed with ref_cluster without scipy)")
    ap.add_argument("--no-host", action="store_true", help="skip the host comparison")
    ap.add_argument("--target-energy", type=float, default=None, help="time the per-recording PLDA adaptation instead")
    ap.add_argument("--adapt-dims", type=int, nargs="+", default=[128, 200])
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib, scoring
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench needs a GPU")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    d = args.dim
    rng = np.random.default_rng(1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    out = {"device": torch.cuda.get_device_name(0), "dim": d, "repeats": args.repeats}

    def adapt_leg(dim, sizes):
        """xv_plda_adapt over recordings drawn from a random PLDA model of dimension `dim` (2..8 speakers each)."""
        sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
        import ref_plda
        import ref_plda_adapt
        from tf_kaldi_speaker_amd import cluster, plda
        te = args.target_energy
        mean, transform, psi = ref_plda.random_model(rng, dim)
        model = plda.Plda(mean, transform, psi)
        recs = []
        for n in sizes:
            k = int(rng.integers(2, 9))
            x, _ = ref_plda.draw(rng, mean, transform, psi, k, (n + k - 1) // k)
            recs.append(np.ascontiguousarray(x[rng.permutation(len(x))[:n]], dtype=np.float32))
        x = np.concatenate(recs)
        groups = np.repeat(np.arange(len(sizes)), sizes)
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        xs = torch.from_numpy(x).to(dev)
        plda._adapt_raw(model, xs, offsets, te, want_pca=False)             # warm-up, same shapes
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dim_out, _, _, _, _, sweeps = plda._adapt_raw(model, xs, offsets, te, want_pca=False)
            times.append(1e3 * (time.perf_counter() - t0))                   # the call and its copies back; synchronised by them
        # the kernel alone: hipEvents around one xv_plda_adapt with preallocated outputs
        cnt = len(sizes)
        bufs = [torch.empty(s, dtype=torch.float64, device=dev) for s in ((cnt, dim), (cnt, dim, dim), (cnt, dim, dim + 1), (cnt, dim))]
        dims_dev = torch.empty((cnt,), dtype=torch.int32, device=dev)
        mean_d, ainv_d, psi_d = plda._adapt_device(model, 0, torch)
        size = int(lib.xv_plda_adapt_workspace(cnt, dim)) + (cnt - 1) * int(lib.xv_plda_adapt_slot_bytes(dim))
        ws = torch.empty((size,), dtype=torch.uint8, device=dev)
        kernel = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.xv_plda_adapt(0, P(xs), dim, offsets.ctypes.data_as(C.c_void_p), cnt, dim, P(mean_d), P(ainv_d), P(psi_d), te,
                                         P(dims_dev), P(bufs[0]), P(bufs[1]), P(bufs[2]), P(bufs[3]), P(ws), size, stream))
            e1.record()
            e1.synchronize()
            kernel.append(e0.elapsed_time(e1))
        res = {"dim": dim, "groups": cnt, "rows_total": int(sum(sizes)), "rows_max": int(max(sizes)), "target_energy": te,
               "workspace_mbytes": 1e-6 * size, "adapt_kernel_ms": float(np.median(kernel)), "adapt_kernel_all_ms": kernel,
               "adapt_call_ms": float(np.median(times)), "adapt_call_all_ms": times,
               "kept_dims_min_median_max": [int(dim_out.min()), float(np.median(dim_out)), int(dim_out.max())],
               "fallbacks": int(np.sum(dim_out == 0)),
               "sweeps_pca_min_median_max": [int(sweeps[:, 0].min()), float(np.median(sweeps[:, 0])), int(sweeps[:, 0].max())],
               "sweeps_model_min_median_max": [int(sweeps[:, 1].min()), float(np.median(sweeps[:, 1])), int(sweeps[:, 1].max())]}
        for name, kw in (("cluster_plda_global_ms", {}), ("cluster_plda_adapted_ms", {"target_energy": te})):
            cluster.plda(model, xs, groups, threshold=0.0, normalize=False, **kw)          # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cluster.plda(model, xs, groups, threshold=0.0, normalize=False, **kw)
            res[name] = 1e3 * (time.perf_counter() - t0)
        if not args.no_host:
            t0 = time.perf_counter()
            kept = [ref_plda_adapt.adapt(mean, transform, psi, r, te).dim for r in recs]
            res["host_numpy_ms"] = 1e3 * (time.perf_counter() - t0)
            res["host_what"] = "tests/helpers/ref_plda_adapt.adapt (numpy float64: covariance, eigh, cholesky, eigh), one recording after the other"
            res["kept_dims_equal_to_host"] = int(np.sum(np.asarray(kept) == dim_out))
        return res

    if args.target_energy is not None:
        sizes = [int(v) for v in rng.integers(200, 1001, args.groups)] + [args.single]
        out["adapt"] = [adapt_leg(dim, sizes) for dim in args.adapt_dims]
        print(json.dumps(out))
        return

    def rows_of(n):
        """n prepared rows: 2..8 speaker centroids + noise, like the sub-segments of a conversation."""
        k = int(rng.integers(2, 9))
        cent = torch.randn((k, d), device=dev, generator=gen)
        lab = torch.randint(0, k, (n,), device=dev, generator=gen)
        return scoring.prepare(cent[lab] + 1.5 * torch.randn((n, d), device=dev, generator=gen), as_tensor=True)

    def ld(n):
        return max(4, (n + 3) // 4 * 4)

    def leg(sizes):
        xs = [rows_of(n) for n in sizes]
        rows = np.ascontiguousarray(sizes, dtype=np.int32)
        off = np.concatenate([[0], np.cumsum([n * ld(n) for n in sizes])])
        s = torch.empty((int(off[-1]),), dtype=torch.float32, device=dev)
        total = int(rows.sum())
        labels = torch.empty((total,), dtype=torch.int32, device=dev)
        ma, mb = torch.empty_like(labels), torch.empty_like(labels)
        mh = torch.empty((total,), dtype=torch.float64, device=dev)
        cnt = torch.empty((len(sizes),), dtype=torch.int32, device=dev)
        need = int(lib.xv_ahc_workspace(len(sizes), rows.ctypes.data_as(C.c_void_p)))
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)

        def fill():
            for x, n, o in zip(xs, sizes, off):
                _lib.check(lib.xv_score_matrix(0, P(x), d, n, P(x), d, n, d, C.c_void_p(s.data_ptr() + 4 * int(o)), ld(n), stream))

        def cluster():
            _lib.check(lib.xv_ahc(0, P(s), rows.ctypes.data_as(C.c_void_p), None, len(sizes), float("-inf"), P(labels), P(cnt), P(ma), P(mb),
                                  P(mh), P(ws), need, stream))

        def once(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        fill()
        cluster()                                   # warm-up of both, same shapes
        torch.cuda.synchronize()
        t_fill, t_cluster = [], []
        for _ in range(args.repeats):
            t_fill.append(once(fill))
            t_cluster.append(once(cluster))
        assert int(cnt.min()) == 1 and int(cnt.max()) == 1
        fill()
        torch.cuda.synchronize()
        host = s.cpu().numpy()
        mats = [host[off[i]:off[i + 1]].reshape(n, ld(n))[:, :n] for i, n in enumerate(sizes)]
        res = {"groups": len(sizes), "rows_total": total, "rows_min": int(min(sizes)), "rows_max": int(max(sizes)),
               "matrix_mbytes": 4e-6 * float(off[-1]), "fill_ms": float(np.median(t_fill)), "fill_all_ms": t_fill,
               "cluster_ms": float(np.median(t_cluster)), "cluster_all_ms": t_cluster}
        return res, mats, mh.cpu().numpy(), np.concatenate([[0], np.cumsum(sizes)])

    def scipy_leg(mats, heights, starts, res):
        try:
            from scipy.cluster.hierarchy import linkage
        except ImportError:
            linkage = None
        if linkage is None:
            sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
            import ref_cluster
            order = np.argsort([len(m) for m in mats])[:args.subset]
            t0 = time.perf_counter()
            for i in order:
                ref_cluster.ahc(mats[i])
            res["host"] = {"what": "ref_cluster.ahc on the %d smallest recordings (no scipy)" % len(order),
                           "rows": [int(len(mats[i])) for i in order], "seconds": time.perf_counter() - t0}
            return
        t0 = time.perf_counter()
        worst = 0.0
        for i, m in enumerate(mats):
            n = len(m)
            iu = np.triu_indices(n, 1)
            top = float(m[iu].max())
            z = linkage((top - m[iu]).astype(np.float64), method="average")
            if i < args.subset:
                worst = max(worst, float(np.max(np.abs((top - z[:, 2]) - np.sort(heights[starts[i]:starts[i] + n - 1])[::-1]))))
        res["host"] = {"what": "scipy linkage(method='average') on every recording, one thread, incl. the condensed copy",
                       "seconds": time.perf_counter() - t0, "max_height_diff_first_recordings": worst}

    sizes = [int(v) for v in rng.integers(200, 1001, args.groups)]
    res, mats, heights, starts = leg(sizes)
    if not args.no_host:
        scipy_leg(mats, heights, starts, res)
    out["batch"] = res
    del mats
    torch.cuda.empty_cache()
    res, mats, heights, starts = leg([args.single])
    if not args.no_host:
        scipy_leg(mats, heights, starts, res)
    out["single"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
