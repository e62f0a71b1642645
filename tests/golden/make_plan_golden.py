#!/usr/bin/env python
"""Record tests/golden/plan_info.json: what the batch planner decides, case by case (tests/test_gpu_plan_golden.py compares
for equality).  Per case it stores

  * the xv_plan_info fields frame_level, out_rows, out_cols, workspace_bytes (= the top of the workspace arena) and flops;
  * after one profiled forward, the steps in order as [name, launches, flops, bytes].

Together they fix the step order, every fusion decision (a fused step reports other bytes / flops than the plain one, a
reordered value layer shows in the order) and the arena layout.  The file is recorded on a build of the PARENT of a change
to the planner, never on the code under test:

  python tests/golden/make_plan_golden.py [--lib /path/to/libxvec_hip.so of the parent build]      (needs a GPU)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "plan_info.json")
INFO_FIELDS = ("frame_level", "out_rows", "out_cols", "workspace_bytes", "flops")

RAGGED = [31, 64, 127, 129, 200]
ATT_HEADS = {                      # the three settings of tests/test_gpu_variants.py
    "h1": {},
    "h3": {"att_num_heads": 3, "att_split_key": False, "att_split_value": False},
    "h5": {"att_num_heads": 5, "num_nodes_pooling_layer": 1600, "att_key_num_nodes": [1500, 1600]},
}


def _batches(dim, which):
    """name -> (lengths, feature seed).  'base' is the 256 x 300 batch of test_gpu_variants._baseline_batch: the smallest
    geometry at which gemm_bf16x3_tail_plan is known to give a tail."""
    all_ = {"ragged": (RAGGED, 71), "base": ([300] * 256, 5), "u4x64": ([64] * 4, 72), "res": ([33, 64, 101], 73)}
    return {k: all_[k] for k in which}


def groups():
    """One group = one model at one precision (one set of uploaded weights).  Yields (group id, spec); spec["runs"] lists
    (trainer options set before the weights are loaded, [(plan options, batch, node), ...])."""
    from tf_kaldi_speaker_amd import synth
    toggles = lambda names: [{}] + [{n: 0} for n in names]
    for prec in ("f32", "bf16x3", "f16f6"):
        plans = [(o, b, n) for o in toggles(("pool_fusion", "tail_split")) for b in ("ragged", "base")
                 for n in ("tdnn6_dense", "pooling", "tdnn5_relu", "tdnn3_conv")]
        yield "tdnn_stat/" + prec, dict(params=dict(synth.TDNN_STAT_PARAMS), dim=30, seed=0, precision=prec, runs=[({}, plans)])
    for heads, kw in ATT_HEADS.items():
        for prec in ("bf16x3", "f32"):
            plans = [(o, b, n) for o in toggles(("att_fusion",))
                     for b, n in (("ragged", "tdnn6_dense"), ("u4x64", "tdnn6_dense"), ("u4x64", "attention_weights"))]
            yield "tdnn_att_%s/%s" % (heads, prec), dict(params=dict(synth.TDNN_ATT_PARAMS, **kw), dim=30, seed=6,
                                                          precision=prec, runs=[({}, plans)])
    for prec in ("f16f6", "f16x3"):         # in_f6 / out_f6 chaining and the one-tap producer rule
        params = dict(synth.TDNN_STAT_PARAMS, network_type="extended_tdnn", embedding_node="tdnn12_dense")
        plans = [({}, b, "tdnn12_dense") for b in ("ragged", "base")]
        yield "etdnn/" + prec, dict(params=params, dim=30, seed=0, precision=prec, runs=[({}, plans)])
    for tag, kw in (("plain", {}), ("ts_max", {"resnet_time_stride": True, "resnet_maxpooling": True})):
        for prec in ("f32", "bf16x3", "f16f6"):
            plans = [(o, "res", n) for o in toggles(("grid_compact",)) for n in ("tdnn6_dense", "conv3a")]
            runs = [({}, plans)]
            if prec == "f16f6":             # read at finalize: a trainer of its own
                runs.append(({"grid_f6": 0}, [({}, "res", n) for n in ("tdnn6_dense", "conv3a")]))
            yield "resnet_%s/%s" % (tag, prec), dict(params=dict(synth.RESNET_PARAMS, **kw), dim=40, seed=1, precision=prec,
                                                      resnet=True, runs=runs)


def _key(opts):
    return ",".join("%s=%d" % kv for kv in sorted(opts.items())) or "default"


def run_group(spec, on_output=None):
    """Run every plan of a group; returns {case key: {"info": {...}, "steps": [[name, launches, flops, bytes], ...]}}.
    on_output(case key, CUDA tensor) sees each forward's result (the recorder itself does not use it)."""
    import torch
    from tf_kaldi_speaker_amd import synth
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, dim = spec["params"], spec["dim"]
    weights = synth.synth_resnet_weights(params, seed=spec["seed"]) if spec.get("resnet") else synth.synth_weights(params, dim, seed=spec["seed"])
    names = sorted({b for _, plans in spec["runs"] for _, b, _ in plans})
    data = {}
    for name, (lens, seed) in _batches(dim, names).items():
        feats = torch.from_numpy(np.concatenate(synth.synth_features(len(lens), lens, dim, seed=seed))).cuda()
        data[name] = (feats, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    res = {}
    for pre, plans in spec["runs"]:
        tr = Trainer(Params(**dict(params)), None, dim, single_cpu=True, device=0, precision=spec["precision"], range_fallback=False)
        tr.build("predict")
        for k, v in pre.items():
            tr.set_option(k, v)
        tr.load_weights(weights)
        current = {}
        for opts, batch, node in plans:
            for k in set(current) | set(opts):              # one toggle at a time: everything else back to its default
                if current.get(k, 1) != opts.get(k, 1):
                    tr.set_option(k, opts.get(k, 1))
            current = dict(opts)
            feats, offs = data[batch]
            info = tr.plan_info(offs, node)
            tr.profile_begin()
            out = tr.predict_packed(feats, offs, node)
            torch.cuda.synchronize()
            recs, nfwd = tr.profile_end()
            assert nfwd == 1
            key = "%s/%s/%s" % (_key(dict(pre, **opts)), batch, node)
            res[key] = {"info": {f: int(info[f]) for f in INFO_FIELDS},
                        "steps": [[r["name"], r["launches"], r["flops"], r["bytes"]] for r in recs]}
            if on_output is not None:
                on_output(key, out)
        tr.close()
    return res


def write_golden(path, golden):
    """Step lists are stored once each (most cases share one with a neighbour) and named by index; one case per line, so a
    change of one plan is one line of diff."""
    lists = sorted({json.dumps(rec["steps"], separators=(",", ":")) for rec in golden.values()})
    cases = ["%s: %s" % (json.dumps(k), json.dumps([rec["info"][f] for f in INFO_FIELDS] +
                                                   [lists.index(json.dumps(rec["steps"], separators=(",", ":")))], separators=(",", ":")))
             for k, rec in sorted(golden.items())]
    with open(path, "w") as f:
        f.write('{"info_fields": %s,\n"step_lists": [\n%s\n],\n"cases": {\n%s\n}}\n' % (json.dumps(list(INFO_FIELDS)), ",\n".join(lists), ",\n".join(cases)))


def load_golden(path=GOLDEN):
    """-> {case key: {"info": {...}, "steps": [...]}}, the form run_group() returns."""
    with open(path) as f:
        g = json.load(f)
    return {k: {"info": dict(zip(g["info_fields"], v[:-1])), "steps": g["step_lists"][v[-1]]} for k, v in g["cases"].items()}


def main():
    sys.path.insert(0, ROOT)
    from tf_kaldi_speaker_amd import _lib
    if "--lib" in sys.argv:
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    golden = {}
    for gid, spec in groups():
        for key, rec in run_group(spec).items():
            golden["%s/%s" % (gid, key)] = rec
        print("recorded", gid, flush=True)
    write_golden(out, golden)
    print("wrote %s: %d cases with %s" % (out, len(golden), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
