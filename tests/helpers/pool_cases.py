"""Models and batches for the isolated pooling tests (tests/test_pool_bars_host.py, tests/test_gpu_pool_isolated.py).

Channel classes, interleaved c mod 6 so that the four adjacent columns of one lane hold different classes.  They are written
into the batch normalisation of the layer that feeds the pooling (tdnn5 -- which is also the attention value -- or dense2),
on a standardised pre-activation z (moving mean / variance set from measured statistics, `calibrated`):

    0 ordinary               gamma, beta as synthesised
    1 near_constant          gamma * 2^-10, beta 4
    2 near_constant_large    gamma * 2^-6,  beta 200
    3 dead                   beta -1e3 (exactly zero under ReLU)
    4 constant               gamma 0, beta 3
    5 sparse                 beta = -2.326 gamma: about 1 % of the frames are non-zero

The function the network computes changes; that does not matter, the reference is the pooling of the GPU's own frames."""
import numpy as np

CLASS_NAMES = ("ordinary", "near_constant", "near_constant_large", "dead", "constant", "sparse")
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 300)
# utterance borders at tile offsets 63 (first slot of the 300: one frame) and 43 .. / 0 (64 | 65: last slot one frame), 1, 0
PACK_ORDERS = ((63, 300, 1, 2, 64, 65, 127, 128, 129), (64, 65, 63, 1, 127, 2, 300, 128, 129))
LONG = (12000, 1)
QUERY_FACTOR = {"moderate": 20.0, "peaked": 30000.0}


def class_of(C):
    return np.arange(C) % 6


def class_affine(gamma, beta):
    """Per-channel (gamma, beta) of the six classes from ordinary ones."""
    gamma = np.asarray(gamma, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    cls = class_of(gamma.shape[0])
    g = np.select([cls == 1, cls == 2, cls == 4], [gamma * 2.0 ** -10, gamma * 2.0 ** -6, 0.0 * gamma], gamma)
    b = np.select([cls == 1, cls == 2, cls == 3, cls == 4, cls == 5], [4.0 + 0 * beta, 200.0 + 0 * beta, -1e3 + 0 * beta,
                                                                      3.0 + 0 * beta, -2.326 * gamma], beta)
    return g, b


def border_offsets():
    """Tile offsets (row mod 64) at which utterances begin, over both pack orders, and the sizes of first / last slots."""
    offs, first, last = set(), set(), set()
    for order in PACK_ORDERS:
        r = 0
        for n in order:
            offs.add(r & 63)
            first.add(min(n, 64 - (r & 63)))
            last.add(((r + n - 1) & 63) + 1 if (r >> 6) != ((r + n - 1) >> 6) else n)
            r += n
    return offs, first, last


# --------------------------------------------------------------------------------------------------------------- models
def features(lens, dim, seed):
    from tf_kaldi_speaker_amd import synth
    return synth.synth_features(len(lens), list(lens), dim, seed=seed)


def _tdnn(kw, channels, dim, seed):
    from tf_kaldi_speaker_amd import synth
    base = synth.TDNN_ATT_PARAMS if kw.get("pooling_type") == "self_attention" else synth.TDNN_STAT_PARAMS
    params = dict(base, **kw)
    return params, dict(synth.synth_weights(params, dim, seed=seed, channels=channels)), dim


NARROW = dict(num_nodes_pooling_layer=96, num_nodes_last_layer=40)
STAT_MODELS = {
    "narrow": lambda: _tdnn(dict(NARROW), 64, 23, 4),
    "narrow_prelu": lambda: _tdnn(dict(NARROW, network_relu_type="prelu"), 64, 23, 5),
    "full": lambda: _tdnn({}, 512, 30, 0),
}
_ATT = dict(NARROW, pooling_type="self_attention", att_key_num_nodes=[64, 48])
ATT_MODELS = {
    "heads1": dict(_ATT),
    "heads3_unsplit": dict(_ATT, att_num_heads=3, att_split_key=False, att_split_value=False),
    "heads2_split": dict(_ATT, att_num_heads=2, num_nodes_pooling_layer=128),       # dv / H = 64: the fused path is eligible
}


def stat_model(name):
    """(params, weights, feature dim)."""
    params, weights, dim = STAT_MODELS[name]()
    return params, weights, dim


def resnet_model():
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.RESNET_PARAMS, num_nodes_pooling_layer=96, resnet_time_stride=True)
    return params, dict(synth.synth_resnet_weights(params, seed=7, width=32)), 40


def att_model(name, regime):
    params, weights, dim = _tdnn(dict(ATT_MODELS[name]), 64, 23, 4)
    weights["tdnn/attention/query"] = (weights["tdnn/attention/query"] * QUERY_FACTOR[regime]).astype(np.float32)
    return params, weights, dim


def key_node(params):
    return "att_key%d_relu" % (len(params["att_key_num_nodes"]) - 1)


def att_scale(params, dk):
    if not params.get("att_use_scale"):
        return 1.0
    return 1.0 / np.sqrt(float(dk // int(params["att_num_heads"]) if params.get("att_split_key") else dk))


def pool_bn_scope(params):
    return "resnet_18/dense2_bn" if params["network_type"] == "resnet_18" else "tdnn/tdnn5_bn"


def pool_input_node(params):
    return "dense2_relu" if params["network_type"] == "resnet_18" else "tdnn5_relu"


PROBE_SHIFT = 64.0


def probe_weights(weights, scope):
    """Weights whose pooling input is z + 64 (identity batch normalisation, shifted clear of the activation), from which
    `calibrated` measures the pre-activation's mean and variance."""
    w = dict(weights)
    n = w[scope + "/gamma"].shape[0]
    w[scope + "/gamma"] = np.ones(n, dtype=np.float32)
    w[scope + "/beta"] = np.full(n, PROBE_SHIFT, dtype=np.float32)
    w[scope + "/moving_mean"] = np.zeros(n, dtype=np.float32)
    w[scope + "/moving_variance"] = np.ones(n, dtype=np.float32)
    return w


def calibrated(weights, scope, probe_frames):
    """Write the six classes into batch normalisation `scope`; `probe_frames` [rows, C] is the pooling input under
    probe_weights."""
    z = np.asarray(probe_frames, dtype=np.float64) - PROBE_SHIFT
    assert (np.asarray(probe_frames) > 0).all(), "the probe shift did not clear the activation"
    w = dict(weights)
    g, b = class_affine(w[scope + "/gamma"], w[scope + "/beta"])
    w[scope + "/gamma"] = g.astype(np.float32)
    w[scope + "/beta"] = b.astype(np.float32)
    w[scope + "/moving_mean"] = z.mean(axis=0).astype(np.float32)
    w[scope + "/moving_variance"] = np.maximum(z.var(axis=0), 1e-6).astype(np.float32)
    return w


# -------------------------------------------------------------------------------------------------------------- batches
def tdnn_batch(out_lens, dim, seed, context=14):
    """(packed features [sum T, dim], input offsets [B + 1], output offsets [B + 1]) for output lengths `out_lens`."""
    lens = [n + context for n in out_lens]
    feats = np.concatenate(features(lens, dim, seed))
    return feats, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate([[0], np.cumsum(out_lens)]).astype(np.int64)


def resnet_batch(out_lens, dim, seed):
    """Three stride-2 stages under 'same' padding: T -> ceil(T / 8); even and odd T."""
    lens = [8 * n - (i % 8) for i, n in enumerate(out_lens)]
    feats = np.concatenate(features(lens, dim, seed))
    return feats, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate([[0], np.cumsum(out_lens)]).astype(np.int64)
