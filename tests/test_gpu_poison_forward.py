"""GPU: every forward path over a workspace and an output full of defined garbage.

The library clears almost nothing; it relies on every byte a kernel reads from the caller's workspace or output having been
written earlier in the same call ("The workspace contract").  Trainer allocates both with torch.empty, so in a
test process they are fresh or benign.  Here each case -- one Trainer, one packed ragged batch, a tuple of nodes --

 1. runs every node once on the case's batch and on its history batch, so that the workspace has its final size;
 2. for each byte of poison.FILLS fills the whole workspace and a caller-provided `out=` with it and runs the node,
    with check_overflow() == 0 behind every run;
 (a) requires the three results bit-identical (which also proves that every element of `out` was written);
 (b) holds the 0xFF result to the suite's bar against the float64 oracle (oracle/ref_numpy: relative L2 <= 1e-4, BASELINE.json,
     as in test_gpu_parity.py), per utterance for segment-level nodes and per node for frame-level ones;
 (c) history: runs a DIFFERENT ragged batch first -- more frames in all, one long utterance whose interior rows or grid positions
     lie where the case's batch has its utterance borders, tails and padding rows -- and then the case's batch without touching
     the workspace: the same bits again.  This is what a ragged ark stream does to every batch.

The oracle runs once per model and batch (module cache) through ref_numpy.entire_network, which is what ref_numpy.predict
returns its node from, one utterance at a time."""
import os
import sys

import numpy as np
import pytest

from oracle import ref_numpy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import poison                                                                   # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
PRECISIONS = ["f32", "bf16x3", "f16x3", "f16f6"]

TDNN_LENS = [300, 64, 200, 15, 129, 333]        # the shortest legal utterance, partial 128-row tiles; borders at 300 364 564 579 708 1041
TDNN_HISTORY = [700, 15, 350, 100]              # 1165 frames: the first utterance's interior covers 300 .. 579, the third's 708 .. 1065
ETDNN_LENS = [300, 64, 200, 23, 129, 333]       # 23 = the extended TDNN's context + 1
ETDNN_HISTORY = [700, 23, 350, 100]
RESNET_LENS = [120, 37, 64, 41, 16, 203]        # borders at 120 157 221 262 278 481
RESNET_HISTORY = [290, 7, 230]                  # 527 frames: interiors over 120 .. 278 and over 481; another number of grids


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(b.shape)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _trainer(params, weights, dim, precision, options=(), late_options=()):
    """`options` are set before the weights are finalised (grid_f6 decides the weight formats), `late_options` behind the load."""
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    tr = Trainer(Params(**dict(params)), None, dim, single_cpu=True, device=0, precision=precision, range_fallback=False)
    tr.build("predict")
    for name, value in options:
        tr.set_option(name, value)
    tr.load_weights(weights)
    for name, value in late_options:
        tr.set_option(name, value)
    return tr


def _batch(lens, dim, seed):
    import torch
    from tf_kaldi_speaker_amd import synth
    utts = synth.synth_features(len(lens), lens, dim, seed=seed)
    feats = torch.from_numpy(np.concatenate(utts)).cuda()
    return utts, feats, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


_models, _oracle = {}, {}


def _model(key, make):
    if key not in _models:
        _models[key] = make()
    return _models[key]


def _endpoints(key, utts, weights, params):
    """Float64 endpoints of every utterance on its own, computed once per (model, batch) and never modified."""
    if key not in _oracle:
        eps = [ref_numpy.entire_network(u[None], weights, params)[1] for u in utts]
        for e in eps:
            for v in e.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _oracle[key] = eps
    return _oracle[key]


def _run(tr, feats, offs, node, out):
    import torch
    got = tr.predict_packed(feats, offs, node, out=out)
    assert got is out
    res = out.cpu().numpy().copy()
    torch.cuda.synchronize()
    return res


def _sweep(tr, nodes, feats, offs, eps, history=None, label=""):
    """Steps 1, 2 and (a), (b), (c) of the module docstring for one trainer and one batch.  -> {node: the 0xFF result}."""
    import torch
    for node in nodes:                                      # 1. final workspace size: the case's batch and its history
        tr.predict_packed(feats, offs, node)
        if history is not None:
            tr.predict_packed(history[0], history[1], node)
    ws = tr._ws
    assert ws is not None and ws.numel() > 0
    tr.check_overflow()                                     # (what the sizing runs met in a workspace nobody filled is not judged)
    results = {}
    for node in nodes:
        shape = tuple(tr.predict_packed(feats, offs, node).shape)
        got = {}
        for byte in poison.FILLS:                           # 2.
            poison.fill(tr._ws, byte)
            out = poison.fill(torch.empty(shape, dtype=torch.float32, device="cuda"), byte)
            got[byte] = _run(tr, feats, offs, node, out)
            assert tr.check_overflow() == 0, (label, node, hex(byte))
        for byte in poison.FILLS[1:]:                       # (a)
            same = got[byte].view(np.uint32) == got[0x00].view(np.uint32)
            assert same.all(), (label, node, "fill %#x changes the result: %d of %d elements, first at %s"
                                % (byte, (~same).sum(), same.size, tuple(int(i) for i in np.argwhere(~same)[0])))
        res = got[0xFF]
        assert np.isfinite(res).all(), (label, node)
        if eps is not None:                                 # (b)
            ref0 = np.asarray(eps[0][node])
            if res.shape[0] == len(eps) and ref0.ndim == 2:             # segment level: [1, E] per utterance
                for i, e in enumerate(eps):
                    err = _rel(res[i], np.asarray(e[node])[0])
                    assert err <= TOL, (label, node, "utterance", i, err)
            else:                                                       # frame level: packed rows in utterance order
                ref = np.concatenate([np.asarray(e[node]).reshape(-1, e[node].shape[-1]) for e in eps], axis=0)
                assert res.shape == ref.shape, (label, node, res.shape, ref.shape)
                err = _rel(res, ref)
                print("%s %s: rel-L2 %.3e" % (label, node, err))
                assert err <= TOL, (label, node, err)
        if history is not None:                             # (c)
            hshape = tuple(tr.predict_packed(history[0], history[1], node).shape)
            hout = poison.fill(torch.empty(hshape, dtype=torch.float32, device="cuda"), 0xFF)
            _run(tr, history[0], history[1], node, hout)
            out = poison.fill(torch.empty(shape, dtype=torch.float32, device="cuda"), 0x7B)
            after = _run(tr, feats, offs, node, out)
            assert tr.check_overflow() == 0, (label, node, "history")
            same = after.view(np.uint32) == res.view(np.uint32)
            assert same.all(), (label, node, "the previous batch changes the result: %d of %d elements, first at %s"
                                % ((~same).sum(), same.size, tuple(int(i) for i in np.argwhere(~same)[0])))
        results[node] = res
    assert tr._ws is ws, "the workspace was reallocated during the sweep"
    return results


# ------------------------------------------------------------------------------------------------ TDNN, statistics pooling
def _stat_model(channels):
    from tf_kaldi_speaker_amd import synth

    def make():
        params = dict(synth.TDNN_STAT_PARAMS)
        return params, synth.synth_weights(params, 30, seed=0, channels=channels)
    return _model(("stat", channels), make)


STAT_NODES = ("tdnn1_relu", "tdnn2_conv", "tdnn3_relu", "tdnn5_relu", "tdnn6_dense")


@pytest.mark.parametrize("channels,precision", [(512, p) for p in PRECISIONS] + [(64, "f16f6"), (128, "f16f6")])
def test_tdnn_statistics_pooling(channels, precision):
    """The frame-level tdnn5_relu forces the unfused pooling, the embedding run takes the fused one.  64 channels: the two-unit
    layers fall back to f16x3; 128 channels: one quad of channel blocks, the peeled body alone."""
    params, weights = _stat_model(channels)
    utts, feats, offs = _batch(TDNN_LENS, 30, seed=41)
    eps = _endpoints(("stat", channels), utts, weights, params)
    history = _batch(TDNN_HISTORY, 30, seed=42)[1:]
    tr = _trainer(params, weights, 30, precision)
    _sweep(tr, STAT_NODES, feats, offs, eps, history, "tdnn%d %s" % (channels, precision))
    tr.close()


# ------------------------------------------------------------------------------------------------ self-attention
ATT_VARIANTS = {
    "one_head": {},
    "five_split_heads": {"att_num_heads": 5, "num_nodes_pooling_layer": 1600, "att_key_num_nodes": [1500, 1600]},
}


def _att_model(variant):
    from tf_kaldi_speaker_amd import synth

    def make():
        params = dict(synth.TDNN_ATT_PARAMS, **ATT_VARIANTS[variant])
        weights = synth.synth_weights(params, 30, seed=6)
        weights["tdnn/attention/query"] = weights["tdnn/attention/query"] * 30.0       # peaky attention
        return params, weights
    return _model(("att", variant), make)


@pytest.mark.parametrize("variant,fusion", [("one_head", 1), ("one_head", 0), ("five_split_heads", 1)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_self_attention(precision, variant, fusion):
    """Attentive pooling fused into the key / value epilogues and unfused (xv_set_option "att_fusion" 0), the shipped one-head
    config and five split heads of 320 channels.  attention_weights [b, h, l] exists for batches of equal length only, so
    that node runs on a uniform batch of its own (three utterances of 129 frames: a partial tile each)."""
    params, weights = _att_model(variant)
    utts, feats, offs = _batch(TDNN_LENS, 30, seed=43)
    eps = _endpoints(("att", variant, "ragged"), utts, weights, params)
    history = _batch(TDNN_HISTORY, 30, seed=44)[1:]
    tr = _trainer(params, weights, 30, precision, late_options=[("att_fusion", fusion)])
    label = "att %s fusion %d %s" % (variant, fusion, precision)
    _sweep(tr, ("tdnn6_dense", "att_key1_relu"), feats, offs, eps, history, label)
    uutts, ufeats, uoffs = _batch([129, 129, 129], 30, seed=45)
    ueps = _endpoints(("att", variant, "uniform"), uutts, weights, params)
    got = _sweep(tr, ("attention_weights",), ufeats, uoffs, None, None, label)["attention_weights"]
    ref = np.concatenate([np.asarray(e["attention_weights"]) for e in ueps], axis=0)
    assert got.size == ref.size
    assert _rel(got, ref) <= TOL, (label, "attention_weights", _rel(got, ref))
    tr.close()


# ------------------------------------------------------------------------------------------------ extended TDNN
@pytest.mark.parametrize("precision", ["f16f6", "bf16x3"])
def test_extended_tdnn(precision):
    from tf_kaldi_speaker_amd import synth

    def make():
        params = dict(synth.TDNN_STAT_PARAMS, network_type="extended_tdnn", embedding_node="tdnn12_dense")
        return params, synth.synth_weights(params, 30, seed=4)
    params, weights = _model("etdnn", make)
    utts, feats, offs = _batch(ETDNN_LENS, 30, seed=46)
    eps = _endpoints("etdnn", utts, weights, params)
    history = _batch(ETDNN_HISTORY, 30, seed=47)[1:]
    tr = _trainer(params, weights, 30, precision)
    _sweep(tr, ("tdnn3_conv", "tdnn7_relu", "tdnn12_dense"), feats, offs, eps, history, "etdnn " + precision)
    tr.close()


# ------------------------------------------------------------------------------------------------ ResNet-18, full width
RESNET_KW = {"plain": {}, "time_stride": {"resnet_time_stride": True},
             "maxpool_time_stride": {"resnet_maxpooling": True, "resnet_time_stride": True}}
RESNET_NODES = ("conv1a", "conv2b_0", "conv3a", "conv4b_0", "conv5_relu", "tdnn6_dense")


def _resnet_case(kw):
    from tf_kaldi_speaker_amd import synth

    def make():
        params = dict(synth.RESNET_PARAMS, **RESNET_KW[kw])
        return params, synth.synth_resnet_weights(params, seed=2)
    params, weights = _model(("resnet", kw), make)
    utts, feats, offs = _batch(RESNET_LENS, 40, seed=33)
    eps = _endpoints(("resnet", kw), utts, weights, params)
    return params, weights, feats, offs, eps, _batch(RESNET_HISTORY, 40, seed=34)[1:]


@pytest.mark.parametrize("compact", [1, 0])
@pytest.mark.parametrize("kw", list(RESNET_KW))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_resnet18_grid_paths(precision, kw, compact):
    """Full width (the two-unit grid form needs cin % 128 == 0): compact rows and the full enumeration, time stride, max-pool,
    the three-tap two-unit form with its shifted output pointer (f16f6)."""
    params, weights, feats, offs, eps, history = _resnet_case(kw)
    tr = _trainer(params, weights, 40, precision, late_options=[("grid_compact", compact)])
    _sweep(tr, RESNET_NODES, feats, offs, eps, history, "resnet %s compact %d %s" % (kw, compact, precision))
    tr.close()


def test_resnet18_f16f6_without_the_two_unit_grid_form():
    """Option grid_f6 off, set before the weights are finalised as the option requires: the grid convolutions of the f16f6
    precision on the f16x3 kernels."""
    params, weights, feats, offs, eps, history = _resnet_case("plain")
    tr = _trainer(params, weights, 40, "f16f6", options=[("grid_f6", 0)])
    _sweep(tr, RESNET_NODES, feats, offs, eps, history, "resnet grid_f6 0")
    tr.close()


# ------------------------------------------------------------------------------------------------ K-split tail
TAIL_B, TAIL_T = 84, 300


@pytest.mark.parametrize("precision", ["bf16x3", "f16f6"])
def test_ksplit_tail(precision):
    """The K-split of the last, nearly empty round of tiles keeps its partial sums in the workspace and a reduce kernel adds
    them up.  Batch: TAIL_B x TAIL_T frames, the smallest uniform batch of 300-frame utterances for which the tail_split 1 and 0
    runs of tdnn3_conv differ in bits.  gemm_bf16x3_tail_plan splits only behind more than 768 tiles (256 CUs x 3 workgroups):
    84 utterances give tdnn1 84 x 296 = 24 864 rows = 195 M tiles x 4 N tiles = 780 tiles, a last round of 12, and what tdnn1 and
    tdnn2 sum in another order reaches tdnn3_conv; 83 utterances give 192 M tiles = 768 tiles, one full round, and no layer splits.
    Found on the MI355X with B = 78 .. 95: bit-identical with and without tail_split up to B = 83, different from B = 84 on, in
    both precisions (from B = 86 on tdnn3_conv has a split tail of its own)."""
    params, weights = _stat_model(512)
    utts, feats, offs = _batch([TAIL_T] * TAIL_B, 30, seed=5)
    nodes = ("tdnn3_conv", "tdnn6_dense")
    ref = _tail_oracle(utts, weights, params, nodes)
    tr = _trainer(params, weights, 30, precision)
    tail = _sweep(tr, nodes, feats, offs, None, None, "tail " + precision)
    tr.set_option("tail_split", 0)
    plain = {n: tr.predict_packed(feats, offs, n).cpu().numpy() for n in nodes}
    tr.close()
    assert not np.array_equal(tail["tdnn3_conv"], plain["tdnn3_conv"])       # the path really was taken
    # (b) every utterance of the embedding, the whole frame-level node (the tail tiles hold the LAST rows)
    assert tail["tdnn6_dense"].shape == ref["tdnn6_dense"].shape
    for i in range(TAIL_B):
        err = _rel(tail["tdnn6_dense"][i], ref["tdnn6_dense"][i])
        assert err <= TOL, (precision, "tdnn6_dense", "utterance", i, err)
    conv = ref["tdnn3_conv"].reshape(-1, ref["tdnn3_conv"].shape[-1])
    assert tail["tdnn3_conv"].shape == conv.shape
    err = _rel(tail["tdnn3_conv"], conv)
    print("tail %s tdnn3_conv: rel-L2 %.3e" % (precision, err))
    assert err <= TOL, (precision, "tdnn3_conv", err)


def _tail_oracle(utts, weights, params, nodes):
    """Float64 endpoints `nodes` of the uniform tail batch, once for both precisions: twelve utterances a call (the oracle treats
    the utterances of a rank-3 batch independently), only the two nodes kept."""
    key = ("stat", 512, "tail")
    if key not in _oracle:
        parts = [ref_numpy.entire_network(np.stack(utts[i:i + 12]), weights, params)[1] for i in range(0, len(utts), 12)]
        _oracle[key] = {n: np.concatenate([np.asarray(p[n]) for p in parts], axis=0) for n in nodes}
        for v in _oracle[key].values():
            v.setflags(write=False)
    return _oracle[key]


# ------------------------------------------------------------------------------------------------ segment head in one launch
@pytest.mark.parametrize("precision", ["f32", "f16f6"])
@pytest.mark.parametrize("batch", [1, 2, 33])
def test_segment_head_one_launch(batch, precision):
    params, weights = _stat_model(512)
    utts, feats, offs = _batch([20] * batch, 30, seed=24)
    eps = _endpoints(("stat", 512, "seg", batch), utts, weights, params)
    history = _batch([20] * (batch + 3), 30, seed=25)[1:]                      # more segment rows than the case has
    tr = _trainer(params, weights, 30, precision)
    _sweep(tr, ("tdnn6_dense",), feats, offs, eps, history, "segment B %d %s" % (batch, precision))
    tr.close()


# ------------------------------------------------------------------------------------------------ plan recycling
@pytest.mark.parametrize("precision", ["bf16x3", "f16f6"])
def test_recycled_plan_arrays(precision):
    """One trainer runs 130 distinct batch geometries -- more than its plan cache of 128 holds, so the device arrays of evicted
    plans go back to the library's pool and are handed to the next plan -- on one workspace that nothing clears in between, and
    then the first ones again, whose plans are gone by then.  Every result must have the bits that a trainer which has seen
    nothing else computes for that geometry."""
    import torch
    from tf_kaldi_speaker_amd import synth
    params, weights = _stat_model(64)
    rng = np.random.default_rng(7)
    geoms = []
    while len(geoms) < 130:
        g = tuple(int(t) for t in rng.integers(15, 41, size=int(rng.integers(1, 4))))
        if g not in geoms:
            geoms.append(g)
    pool = torch.from_numpy(np.concatenate(synth.synth_features(3, 40, 30, seed=48))).cuda()
    seen = _trainer(params, weights, 30, precision)
    assert seen._plan_cache_size == 128 < len(geoms)
    got = []
    for g in geoms + geoms[:8]:
        offs = np.concatenate([[0], np.cumsum(g)]).astype(np.int32)
        got.append(seen.predict_packed(pool[:int(offs[-1])], offs).cpu().numpy())
    assert len(seen._plans) == 128 and seen.check_overflow() == 0
    seen.close()
    for i, g in enumerate(geoms):
        offs = np.concatenate([[0], np.cumsum(g)]).astype(np.int32)
        fresh = _trainer(params, weights, 30, precision)
        want = fresh.predict_packed(pool[:int(offs[-1])], offs).cpu().numpy()
        fresh.close()
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (precision, i, g)
        if i < 8:
            assert np.array_equal(got[len(geoms) + i].view(np.uint32), want.view(np.uint32)), (precision, i, g, "second visit")
