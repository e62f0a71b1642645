"""Timing of the VB-HMM resegmentation (xv_vbx, csrc/vbx.hip) on one MI355X, r = --dim (128), rows of a random PLDA model as
speaker mean plus unit noise in runs of 10 rows, a fifth of the initial labels wrong:

  batch    --groups recordings (500) of T ~ U[200, 1000] rows with S ~ U[8, 16] initial speakers (2 .. 6 true ones) in one call
  single   one recording of --single rows (8192, the most the call takes) with 16 initial speakers: one workgroup on one CU
  host     the float64 numpy oracle (tests/helpers/ref_vbx.vb_hmm, a Python loop over the frames twice per iteration) on the
           first --subset recordings of the batch and on the single one, one after the other; the batch figure is the subset's
           time scaled by the share of (rows x iterations) it holds, and that is stated in the output.  The iteration counts
           and labels of the subset are compared with the device's

Both legs run the published defaults (Fa 0.3, Fb 17, loop_prob 0.99, at most 40 iterations, epsilon 1e-6; --epsilon=-inf makes
every recording run all 40 iterations, which shows the cost of an iteration).  Device times are
hipEvent times around one xv_vbx call (the copy of the group table, the projection kernel and the iteration kernel) with
preallocated operands, after a warm-up call of the same shapes; gamma and pi are restored before every call because the call
updates them in place.  --repeats runs each (3), all reported, the median quoted.  Prints one JSON line; profiles/vbx.md keeps
the numbers."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=500)
    ap.add_argument("--single", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--subset", type=int, default=8, help="recordings of the batch the host oracle runs")
    ap.add_argument("--epsilon", type=float, default=1e-6, help="--epsilon=-inf: every recording runs all 40 iterations")
    ap.add_argument("--no-host", action="store_true", help="skip the host comparison")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import ref_vbx as rv
    from tf_kaldi_speaker_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("vbx_bench needs a GPU")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())           # noqa: E731
    r = args.dim
    rng = np.random.default_rng(1)
    a, psi = rv.draw_model(rng, r, extra=0)
    d = a.shape[1] - 1
    a_dev, psi_dev = torch.from_numpy(a).to(dev), torch.from_numpy(psi).to(dev)
    opts = dict(rv.DEFAULTS, epsilon=args.epsilon)
    out = {"device": torch.cuda.get_device_name(0), "dim": r, "repeats": args.repeats, "options": opts}

    def leg(shapes):
        recs, starts = [], []
        for t_len, s in shapes:
            x, init, _ = rv.draw_rows(rng, a, psi, t_len, s, int(rng.integers(2, 7)))
            recs.append(x)
            starts.append(rv.init_gamma(init, s))
        cnt = len(shapes)
        offsets = np.concatenate([[0], np.cumsum([t for t, _ in shapes])]).astype(np.int64)
        spk = np.array([s for _, s in shapes], np.int32)
        xs = torch.from_numpy(np.ascontiguousarray(np.concatenate(recs), dtype=np.float32)).to(dev)
        gamma0 = torch.from_numpy(np.concatenate([g0.reshape(-1) for g0, _ in starts])).to(dev)
        pi0 = torch.from_numpy(np.concatenate([p0 for _, p0 in starts])).to(dev)
        gamma, pi = gamma0.clone(), pi0.clone()
        labels = torch.empty((int(offsets[-1]),), dtype=torch.int32, device=dev)
        elbo = torch.empty((cnt, opts["max_iters"]), dtype=torch.float64, device=dev)
        iters = torch.empty((cnt,), dtype=torch.int32, device=dev)
        size = int(lib.xv_vbx_workspace(cnt, offsets.ctypes.data_as(C.c_void_p), spk.ctypes.data_as(C.c_void_p), r))
        ws = torch.empty((size,), dtype=torch.uint8, device=dev)
        times = []
        for rep in range(args.repeats + 1):          # the first call is the warm-up
            gamma.copy_(gamma0)
            pi.copy_(pi0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.xv_vbx(0, P(xs), d, offsets.ctypes.data_as(C.c_void_p), spk.ctypes.data_as(C.c_void_p), cnt, d, P(a_dev),
                                  P(psi_dev), r, P(gamma), P(pi), opts["fa"], opts["fb"], opts["loop_prob"], opts["max_iters"],
                                  opts["epsilon"], P(labels), P(elbo), P(iters), P(ws), size, stream))
            e1.record()
            e1.synchronize()
            if rep:
                times.append(e0.elapsed_time(e1))
        it = iters.cpu().numpy()
        lab = labels.cpu().numpy()
        work = np.array([t for t, _ in shapes], np.float64) * it
        res = {"groups": cnt, "rows_total": int(offsets[-1]), "rows_max": int(max(t for t, _ in shapes)),
               "speakers_min_max": [int(spk.min()), int(spk.max())], "workspace_mbytes": 1e-6 * size,
               "vbx_ms": float(np.median(times)), "vbx_all_ms": times,
               "iterations_min_median_max": [int(it.min()), float(np.median(it)), int(it.max())]}
        if not args.no_host:
            sub = min(args.subset, cnt)
            t0 = time.perf_counter()
            refs = [rv.vb_hmm(recs[i], a, psi, starts[i][0], starts[i][1], **opts) for i in range(sub)]
            host = 1e3 * (time.perf_counter() - t0)
            share = float(work[:sub].sum() / work.sum())
            res.update({"host_subset": sub, "host_subset_ms": host, "host_subset_share_of_rows_x_iterations": share,
                        "host_scaled_ms": host / share,
                        "host_what": "tests/helpers/ref_vbx.vb_hmm (numpy float64), one recording after the other",
                        "iterations_equal_to_host": int(sum(int(it[i]) == refs[i].iters for i in range(sub))),
                        "labels_equal_to_host": int(sum(np.array_equal(lab[offsets[i]:offsets[i + 1]], refs[i].labels) for i in range(sub)))})
        return res

    out["batch"] = leg([(int(rng.integers(200, 1001)), int(rng.integers(8, 17))) for _ in range(args.groups)])
    out["single"] = leg([(args.single, 16)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
