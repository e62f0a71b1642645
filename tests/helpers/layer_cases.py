"""Models, layers and batches of the isolated layer tests (tests/test_layer_bars_host.py, tests/test_gpu_layer_isolated.py).

The smallest models that still reach every code path of the TDNN / extended-TDNN layer GEMMs:

    c128    TDNN, 128 channels, 23-dim features, tdnn5 96 wide    one quad of channel blocks: only the peeled last quad of the
                                                                  two-unit body; a partial N tile
    c256    TDNN, 256 channels, 30-dim features                   two quads: the looped body and the peeled quad
    c512w   TDNN, 512 channels, tdnn5 1500 wide, layers 3 and 5   four quads; 1500 = 11 x 128 + 92
    e128    extended TDNN, 128 channels                           9 taps; dense layers between the convolutions, which write
                                                                  the two-unit block format for their reader

in two regimes: "plain" (the synthetic batch normalisation) and "classes": the six channel classes of pool_cases (ordinary,
near-constant, near-constant and large, dead, constant, sparse; interleaved c mod 6) in the batch normalisation of every layer
that has a reader under test, calibrated layer by layer on the layer's own measured pre-activation, so that layer L reads them
from layer L - 1.

Batches: the frame layers see pool_cases.PACK_ORDERS as their OUTPUT lengths (1 .. 300 frames, 1049 rows: utterance borders at
tile offsets 0, 1 and 63, a one-frame utterance, more than 512 rows), i.e. features of n + context(L) frames; the segment layers
one batch of nine utterances."""
import numpy as np

import pool_cases as pc
import ref_layer as rl

LENGTHS = pc.LENGTHS
PACK_ORDERS = pc.PACK_ORDERS
REGIMES = ("plain", "classes")

MODELS = {
    "c128": dict(net="tdnn", channels=128, dim=23, pool=96, last=40, layers=None, seed=21),
    "c256": dict(net="tdnn", channels=256, dim=30, pool=160, last=64, layers=None, seed=22),
    "c512w": dict(net="tdnn", channels=512, dim=30, pool=1500, last=64, layers=(3, 5), seed=23),
    "e128": dict(net="extended_tdnn", channels=128, dim=30, pool=96, last=40, layers=None, seed=24),
}


class Layer(object):
    """One affine layer: index (1-based), endpoint prefix 'tdnnN', variable names, shape, and where it sits."""

    def __init__(self, scope, name, index, w, cin, cout, frame_level, ctx):
        self.index, self.w, self.cin, self.cout, self.frame_level, self.ctx = index, w, cin, cout, frame_level, ctx
        self.prefix = "tdnn%d" % index
        self.kind = "conv" if w > 1 else "dense"
        self.affine = name                                         # endpoint, and the step name the profiler reports
        self.kernel_name = "%s/%s/kernel" % (scope, name)
        self.bias_name = "%s/%s/bias" % (scope, name)
        self.bn_scope = "%s/%s_bn" % (scope, self.prefix)
        self.first = index == 1
        self.cin_pad = (cin + 31) // 32 * 32 if frame_level else cin

    def endpoint(self, stage):
        return {"affine": self.affine, "bn": self.prefix + "_bn", "relu": self.prefix + "_relu"}[stage]


def model(name):
    """(params, weights, feature dim, layers [all of the graph, in order])."""
    from tf_kaldi_speaker_amd import synth
    m = MODELS[name]
    params = dict(synth.TDNN_STAT_PARAMS, network_type=m["net"], num_nodes_pooling_layer=m["pool"], num_nodes_last_layer=m["last"])
    if m["net"] == "extended_tdnn":
        params["embedding_node"] = "tdnn12_dense"
    weights = dict(synth.synth_weights(params, m["dim"], seed=m["seed"], channels=m["channels"]))
    return params, weights, m["dim"], layers(name)


def layers(name):
    from tf_kaldi_speaker_amd import synth
    m = MODELS[name]
    params = dict(network_type=m["net"], num_nodes_pooling_layer=m["pool"], num_nodes_last_layer=m["last"],
                  pooling_type="statistics_pooling")
    scope, widths, _, seg = synth.net_spec(params)
    out, ctx = [], 0
    for i, (lname, w, cin, cout) in enumerate(synth.tdnn_layer_dims(params, m["dim"], m["channels"]), start=1):
        frame = i <= len(widths)
        ctx += (w - 1) if frame else 0
        out.append(Layer(scope, lname, i if frame else seg[i - len(widths) - 1], w, cin, cout, frame, ctx if frame else 0))
    return out


def tested_layers(name):
    """The layers of `name` that are measured."""
    want = MODELS[name]["layers"]
    return [L for L in layers(name) if want is None or L.index in want]


def total_context(name):
    return max(L.ctx for L in layers(name))


def producer(name, L):
    """The layer whose '_relu' endpoint is L's input: None for the first layer (features) and the first segment layer
    ('pooling')."""
    ls = layers(name)
    i = [x.index for x in ls].index(L.index)
    if i == 0 or (not L.frame_level and ls[i - 1].frame_level):
        return None
    return ls[i - 1]


def input_node(name, L):
    p = producer(name, L)
    if p is not None:
        return p.endpoint("relu")
    return None if L.first else "pooling"


def two_unit_eligible(L):
    """choose_kernels: the 5-, 7- and 9-tap layers over whole quads of 32-channel blocks, not the first layer."""
    return L.frame_level and not L.first and L.w in (5, 7, 9) and L.cin % 128 == 0 and L.cout % 4 == 0


def expected_kernel(L, precision, two_unit, rows):
    """The kernel the library's dispatch gives this layer (csrc/api_forward.hip run_gemm, launch_gemm_bf16x3, launch_gemm_f32):
    the profiler reports a plan's steps by layer; the kernel of a step follows from these rules and Trainer.runs_two_unit."""
    arith = rl.arithmetic(precision, L.frame_level, two_unit)
    if arith == "f32":
        return "gemm_f32_seg_kernel" if (L.w == 1 and rows <= 512 and not L.first) else "gemm_f32_kernel"
    if arith == "f16f6":
        return "gemm_f6v2_kernel<%d>" % L.w
    return "gemm_bf16x3_w1p3_kernel" if L.w == 1 else "gemm_bf16x3_w14p2_kernel"


# -------------------------------------------------------------------------------------------------------------- batches
def batch(name, L, order, seed):
    """(features [sum T, dim], input offsets int32) with L's output lengths = PACK_ORDERS[order] (frame layers) or the nine
    utterances of PACK_ORDERS[0] at full context (segment layers)."""
    ctx = L.ctx if L.frame_level else total_context(name)
    lens = [n + ctx for n in PACK_ORDERS[order if L.frame_level else 0]]
    feats = np.concatenate(pc.features(lens, MODELS[name]["dim"], seed))
    return feats, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def orders(L):
    return (0, 1) if L.frame_level else (0,)


def layer_offsets(in_offsets, ctx_in):
    """Offsets of the rows of a frame-level value of context `ctx_in` from the feature offsets."""
    lens = np.diff(np.asarray(in_offsets, dtype=np.int64)) - ctx_in
    return np.concatenate([[0], np.cumsum(lens)])


def checked_elements():
    """The number of elements the GPU bar tests compare (three stage endpoints of every case): N of the Hoeffding bound."""
    n = 0
    for name in MODELS:
        for L in tested_layers(name):
            rows = sum(sum(PACK_ORDERS[o]) if L.frame_level else len(PACK_ORDERS[0]) for o in orders(L))
            n += 3 * rows * L.cout * len(rl.PRECISIONS) * len(REGIMES)
    return n


# -------------------------------------------------------------------------------------------------------------- classes
def class_weights(weights, L, z):
    """The six classes in L's batch normalisation, on the standardised pre-activation: moving mean / variance from the
    measured '_conv' / '_dense' endpoint z [rows, cout] (pool_cases.calibrated does the same through a probe normalisation; a
    layer has the endpoint itself)."""
    z = np.asarray(z, dtype=np.float64)
    w = dict(weights)
    g, b = pc.class_affine(w[L.bn_scope + "/gamma"], w[L.bn_scope + "/beta"])
    w[L.bn_scope + "/gamma"] = g.astype(np.float32)
    w[L.bn_scope + "/beta"] = b.astype(np.float32)
    w[L.bn_scope + "/moving_mean"] = z.mean(axis=0).astype(np.float32)
    w[L.bn_scope + "/moving_variance"] = np.maximum(z.var(axis=0), 1e-6).astype(np.float32)
    return w


def calibrated(name, weights, measure):
    """The "classes" weights of model `name`: every layer but the last, in graph order, gets the classes on the pre-activation
    it shows once the layers in front of it carry theirs.  `measure(weights, node, feats, offsets)` returns a node's rows."""
    ls = layers(name)
    last = ls[-1]
    feats, offs = batch(name, last, 0, 70)
    w = dict(weights)
    for L in ls[:-1]:
        w = class_weights(w, L, measure(w, L.affine, feats, offs))
    return w


# ------------------------------------------------------------------------------------------------------------ reference
def reference(weights, name, L, precision, two_unit, x, in_offsets_rows, in_exp=None, kernel=None, quantiser=rl.q6_rne):
    """Everything the GPU test compares of layer L on its own input x [rows_in, cin] (fp32, rows packed per `in_offsets_rows`):
    the term pairs, and per stage (model value, pre-activation, scale vector)."""
    arith = rl.arithmetic(precision, L.frame_level, two_unit)
    k3 = rl.kernel_matrix(weights[L.kernel_name] if kernel is None else kernel, L.cin_pad if arith != "f32" else None)
    wts = rl.split_weights(k3, arith)
    if in_exp is None:
        p = producer(name, L)
        in_exp = 0
        if arith in ("f16x3", "f16f6") and p is not None:
            in_exp = rl.act_exponent(weights, p.bn_scope)
    xin = rl.pad32(x) if arith != "f32" else np.asarray(x)
    acts = rl.split_acts(xin, arith, in_exp, quantiser)
    rows, out_offs = rl.gather_rows(in_offsets_rows, L.w)
    tms = rl.terms(acts, wts, arith, rows)
    vec = rl.epilogue_vectors(weights, L.kernel_name, L.bias_name, L.bn_scope, wts["ws"], in_exp)
    return dict(arith=arith, terms=tms, vectors=vec, out_offsets=out_offs, in_exp=in_exp, ws=wts["ws"], acts=acts, wts=wts, rows=rows)
