"""GPU: per-channel scale spread against the block scales of the two-unit split (XV_PREC_F16F6).

The cross terms of the two-unit product (csrc/gemm_f6v2.hip) are fp6 e2m3 under ONE power-of-two scale per 32 channels along K:
per (frame, 32-channel block) for the activations, per (32-channel block, tap, output column) for the weights.  A channel much
smaller than the largest of its block is quantised against that largest value and its cross terms fall towards plain fp16
(2^-11).  The synthetic models of the other tests never reach that case (Glorot kernels, gamma ~ U(0.5, 1.5), N(0,1) features);
a trained checkpoint can: it is free to split magnitude between a batch-normalisation scale and the next kernel's rows.

Every case compares all four precisions with the float64 oracle (TOL on every listed endpoint); f16f6 in addition holds the
frame-level endpoints of the reader layers to 5e-5 against the exact fp32 path and the embedding to 5e-5 against the oracle
(the bars of test_f16f6_two_unit_split).  A compensated rescaling (layer L's gamma / beta x 2^u_c, the reader's input rows x 2^-u_c)
is the same function: the oracle of the rescaled model must equal the oracle of the base model.  xv_layer_two_unit shows which
kernel each reader ran on: the library demotes a layer whose blocks the fp6 cross terms cannot hold to the f16x3 kernels."""
import numpy as np
import pytest

from oracle import ref_numpy

pytestmark = pytest.mark.gpu
TOL = 1e-4
PRECISIONS = ("f32", "bf16x3", "f16x3", "f16f6")
LENS = [300, 64, 15, 129]                 # ragged, with the shortest legal TDNN utterance
ETDNN_LENS = [300, 64, 23, 129]           # extended TDNN: 22 frames of context


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(b.shape)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _trainer(params, weights, dim, precision, **kw):
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    tr = Trainer(Params(**dict(params)), None, dim, single_cpu=True, device=0, precision=precision, **kw)
    tr.build("predict")
    tr.load_weights(weights)
    return tr


def _forward(params, weights, dim, utts, precision, ref):
    """node -> list of per-utterance float64 results shaped like the oracle's `ref[node]` (one packed forward per node)."""
    import torch
    feats = torch.from_numpy(np.concatenate(utts)).cuda()
    offs = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int32)
    tr = _trainer(params, weights, dim, precision)
    out = {}
    for node, refs in ref.items():
        got = tr.predict_packed(feats, offs, node).cpu().numpy().astype(np.float64)
        rows = np.cumsum([0] + [r.size // r.shape[-1] for r in refs])
        assert got.shape[0] == rows[-1], (node, got.shape, rows[-1])
        out[node] = [got[rows[i]:rows[i + 1]].reshape(refs[i].shape) for i in range(len(refs))]
    tr.close()
    return out


def _two_unit(params, weights, dim, endpoints):
    tr = _trainer(params, weights, dim, "f16f6")
    res = {e: tr.runs_two_unit(e) for e in endpoints}
    tr.close()
    return res


def _oracle(params, weights, dim, utts, nodes):
    eps = [ref_numpy.entire_network(u[None], weights, params)[1] for u in utts]          # one forward per utterance
    return {n: [ep[n][0] for ep in eps] for n in nodes}


def _spread(weights, bn_scope, reader_kernel, u):
    """Channel c of `bn_scope` x 2^u_c (gamma and beta), input row c of `reader_kernel` x 2^-u_c: the same function (ReLU is
    positively homogeneous), other per-channel magnitudes inside every 32-channel block."""
    w = dict(weights)
    f = 2.0 ** np.asarray(u, dtype=np.float64)
    for nm in ("gamma", "beta"):
        w[bn_scope + "/" + nm] = (w[bn_scope + "/" + nm] * f).astype(np.float32)
    k = np.asarray(w[reader_kernel], dtype=np.float64)
    w[reader_kernel] = (k / f[:, None]).astype(np.float32)            # kernels are [..., cin, cout]
    return w


def _exponents(n, s, seed):
    return np.random.RandomState(seed).uniform(-s, s, n)              # independent per channel: every block holds the full spread


def _check(params, weights, dim, utts, nodes, frame_nodes, base=None):
    """Runs the four precisions; returns the list of failed bars (empty = all met)."""
    emb = params["embedding_node"]
    nodes = tuple(nodes) + (emb,)
    ref = _oracle(params, weights, dim, utts, nodes)
    bad = []
    if base is not None:                                              # the rescaled model is the same function
        ref0 = _oracle(params, base, dim, utts, nodes)
        for n in nodes:
            for i in range(len(utts)):
                e = _rel(ref[n][i], np.asarray(ref0[n][i], dtype=np.float64))
                assert e <= 1e-6, ("model check", n, i, e)
    res = {p: _forward(params, weights, dim, utts, p, ref) for p in PRECISIONS}
    for p in PRECISIONS:
        for n in nodes:
            for i in range(len(utts)):
                e = _rel(res[p][n][i], ref[n][i])
                if e > TOL:
                    bad.append("%s %s utt %d: %.3e vs oracle > %.0e" % (p, n, i, e, TOL))
    for i in range(len(utts)):
        e = _rel(res["f16f6"][emb][i], ref[emb][i])
        if e > 5e-5:
            bad.append("f16f6 %s utt %d: %.3e vs oracle > 5e-5" % (emb, i, e))
    for n in frame_nodes:
        a = np.concatenate([x.reshape(-1) for x in res["f16f6"][n]])
        b = np.concatenate([x.reshape(-1) for x in res["f32"][n]])
        e = float(np.linalg.norm(a - b) / np.linalg.norm(b))
        if e > 5e-5:
            bad.append("f16f6 %s: %.3e vs the f32 path > 5e-5" % (n, e))
    return bad


def _tdnn(att=False, etdnn=False):
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.TDNN_ATT_PARAMS if att else synth.TDNN_STAT_PARAMS)
    if etdnn:
        params.update(network_type="extended_tdnn", embedding_node="tdnn12_dense")
    return params, dict(synth.synth_weights(params, 30, seed=0))


def _stages(i, kind):
    return tuple("tdnn%d_%s" % (i, s) for s in (kind, "bn", "relu"))


# ------------------------------------------------------------------------------------- a. compensated spread
@pytest.mark.parametrize("s", [2, 4, 6])
@pytest.mark.parametrize("layer", [1, 2, 3])
def test_compensated_spread_tdnn(layer, s):
    """TDNN statistics pooling: layer L's gamma / beta x 2^u_c, u_c ~ U(-s, s), tdnn(L+1)'s input rows x 2^-u_c.  L = 1, 2: the
    readers are the 5- and 7-tap two-unit convolutions; L = 3: the reader is the dense tdnn4 (three units: the control)."""
    from tf_kaldi_speaker_amd import synth
    params, base = _tdnn()
    reader = layer + 1
    kind = "conv" if reader <= 3 else "dense"
    weights = _spread(base, "tdnn/tdnn%d_bn" % layer, "tdnn/tdnn%d_%s/kernel" % (reader, kind), _exponents(512, s, 100 + layer))
    utts = synth.synth_features(len(LENS), LENS, 30, seed=43)
    readers = _stages(reader, kind)
    bad = _check(params, weights, 30, utts, readers, readers, base=base)
    assert not bad, (layer, s, bad)
    two = _two_unit(params, weights, 30, ("tdnn2_conv", "tdnn3_conv", "tdnn4_dense"))
    assert not two["tdnn4_dense"]                                     # dense layers never run two-unit
    if layer == 3:
        assert two["tdnn2_conv"] and two["tdnn3_conv"], two          # nothing they read was changed
    else:
        other = "tdnn%d_conv" % (5 - reader)
        assert two[other], (two, "a layer that reads benign activations was demoted")
        if s >= 4:
            assert not two[readers[0]], (two, "the reader of the spread channels kept the two-unit kernel")


@pytest.mark.parametrize("s", [2, 4, 6])
def test_compensated_spread_etdnn(s):
    """Extended TDNN: the dense layers tdnn2 / 4 / 6 (which write the block format themselves) feed the 5-, 7- and 9-tap
    convolutions tdnn3 / 5 / 7; all three get an independent spread."""
    from tf_kaldi_speaker_amd import synth
    params, base = _tdnn(etdnn=True)
    weights = base
    for layer in (2, 4, 6):
        weights = _spread(weights, "etdnn/tdnn%d_bn" % layer, "etdnn/tdnn%d_conv/kernel" % (layer + 1), _exponents(512, s, 200 + layer))
    utts = synth.synth_features(len(ETDNN_LENS), ETDNN_LENS, 30, seed=44)
    readers = _stages(3, "conv") + _stages(5, "conv") + _stages(7, "conv")
    bad = _check(params, weights, 30, utts, readers, readers, base=base)
    assert not bad, (s, bad)
    if s >= 4:
        two = _two_unit(params, weights, 30, ("tdnn3_conv", "tdnn5_conv", "tdnn7_conv"))
        assert not any(two.values()), two


@pytest.mark.parametrize("s", [4, 6])
def test_compensated_spread_self_attention(s):
    """TDNN with the shipped self-attention pooling: tdnn2 -> tdnn3 (7 taps, two-unit) rescaled; the attention layers behind it
    see the same function."""
    from tf_kaldi_speaker_amd import synth
    params, base = _tdnn(att=True)
    weights = _spread(base, "tdnn/tdnn2_bn", "tdnn/tdnn3_conv/kernel", _exponents(512, s, 302))
    utts = synth.synth_features(len(LENS), LENS, 30, seed=45)
    readers = _stages(3, "conv")
    bad = _check(params, weights, 30, utts, readers + ("tdnn5_relu",), readers, base=base)
    assert not bad, (s, bad)
    two = _two_unit(params, weights, 30, ("tdnn2_conv", "tdnn3_conv"))
    assert two == {"tdnn2_conv": True, "tdnn3_conv": False}, two


def test_compensated_spread_resnet():
    """ResNet-18 at the reference width (stage 3: 256 channels): the BN between the two 3 x 3 convolutions of block conv3a (the
    only kind of BN that can be rescaled without changing the function: the others feed a residual add), 2^U(-6, 6)."""
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.RESNET_PARAMS)
    base = dict(synth.synth_resnet_weights(params, seed=0))
    weights = _spread(base, "resnet_18/conv3a_bn0", "resnet_18/conv3a_conv1/kernel", _exponents(256, 6, 400))
    lens = [120, 37, 64]
    utts = synth.synth_features(len(lens), lens, 40, seed=46)
    bad = _check(params, weights, 40, utts, ("conv3a", "conv4a"), ("conv3a",), base=base)
    assert not bad, bad
    two = _two_unit(params, weights, 40, ("conv3a", "conv3b_0"))         # block outputs = their second convolution
    assert two == {"conv3a": False, "conv3b_0": True}, two


# ------------------------------------------------------------------------------------- b. / c. other statistics
@pytest.mark.parametrize("layer", [1, 2])
def test_uncompensated_spread(layer):
    """gamma / beta x 2^U(-4, 4) per channel and nothing else: a different function, the same bars."""
    from tf_kaldi_speaker_amd import synth
    params, weights = _tdnn()
    f = 2.0 ** _exponents(512, 4, 500 + layer)
    for nm in ("gamma", "beta"):
        key = "tdnn/tdnn%d_bn/%s" % (layer, nm)
        weights[key] = (weights[key] * f).astype(np.float32)
    utts = synth.synth_features(len(LENS), LENS, 30, seed=47)
    readers = _stages(layer + 1, "conv")
    bad = _check(params, weights, 30, utts, readers, readers)
    assert not bad, (layer, bad)


def test_moving_statistics_that_do_not_match_the_data():
    """moving_variance x 2^U(-6, 6) and moving_mean shifted by +-3 sqrt(var) per channel on tdnn1 and tdnn2: the normalised
    outputs are no longer ~N(beta, gamma^2), in either direction (act_exponent derives its power of two from that assumption)."""
    from tf_kaldi_speaker_amd import synth
    params, weights = _tdnn()
    rs = np.random.RandomState(600)
    for layer in (1, 2):
        sc = "tdnn/tdnn%d_bn/" % layer
        var = weights[sc + "moving_variance"].astype(np.float64) * 2.0 ** rs.uniform(-6, 6, 512)
        weights[sc + "moving_variance"] = var.astype(np.float32)
        weights[sc + "moving_mean"] = (weights[sc + "moving_mean"] + rs.choice([-3.0, 3.0], 512) * np.sqrt(var)).astype(np.float32)
    utts = synth.synth_features(len(LENS), LENS, 30, seed=48)
    readers = _stages(2, "conv") + _stages(3, "conv")
    bad = _check(params, weights, 30, utts, readers, readers)
    assert not bad, bad


# ------------------------------------------------------------------------------------- d. features
def test_heavy_tailed_features_with_a_scale_per_coefficient():
    """Student-t (nu = 3) features, coefficient j scaled by 2^(-5 j / 29): heavy tails and a 32x spread inside the one block."""
    params, weights = _tdnn()
    rs = np.random.RandomState(700)
    scale = 2.0 ** np.linspace(0.0, -5.0, 30)
    utts = [(rs.standard_t(3, size=(t, 30)) * scale).astype(np.float32) for t in LENS]
    readers = _stages(1, "conv") + _stages(2, "conv") + _stages(3, "conv")
    bad = _check(params, weights, 30, utts, readers, readers[3:])
    assert not bad, bad


@pytest.mark.parametrize("tiny", [1, 2])
def test_one_tiny_utterance_in_a_ragged_batch(tiny):
    """One utterance at 2^-14 x N(0,1) among N(0,1) ones (the 64-frame one, or the shortest legal one).  tdnn1's bias, beta and
    moving_mean are zero, so that its output is driven by the features alone (in the synthetic model the bias dominates a tiny
    utterance's tdnn1 output and would hide what happens to its features).  The batch's largest feature is in range; the guard is
    per utterance: the fp16 precisions refuse the batch (range_fallback=False) and, by default, run it again in bf16x3.  Every
    utterance, the small one included, meets the bar on tdnn1's stage endpoints and on the embedding."""
    from tf_kaldi_speaker_amd import synth
    params, weights = _tdnn()
    for key in ("tdnn/tdnn1_conv/bias", "tdnn/tdnn1_bn/beta", "tdnn/tdnn1_bn/moving_mean"):
        weights[key] = np.zeros_like(weights[key])
    utts = synth.synth_features(len(LENS), LENS, 30, seed=49)
    utts[tiny] = (utts[tiny] * 2.0 ** -14).astype(np.float32)
    nodes = _stages(1, "conv") + (params["embedding_node"],)
    ref = _oracle(params, weights, 30, utts, nodes)
    bad = []
    for p in PRECISIONS:
        if p in ("f16x3", "f16f6"):
            tr = _trainer(params, weights, 30, p, range_fallback=False)
            with pytest.raises(FloatingPointError, match="below 2\\^-8"):
                tr.predict_list(utts)
            tr.close()
        tr = _trainer(params, weights, 30, p)
        for n in nodes:
            got = tr.predict_list(utts, node=n)
            for i in range(len(utts)):
                e = _rel(got[i], ref[n][i])
                if e > TOL:
                    bad.append("%s %s utt %d: %.3e" % (p, n, i, e))
        tr.close()
    assert not bad, bad


# ------------------------------------------------------------------------------------- e. peaky attention
_PEAKY = {}


def _peaky_case(wseed, fseed):
    from tf_kaldi_speaker_amd import synth
    if (wseed, fseed) not in _PEAKY:
        params = dict(synth.TDNN_ATT_PARAMS)
        weights = dict(synth.synth_weights(params, 30, seed=wseed))
        weights["tdnn/attention/query"] = weights["tdnn/attention/query"] * 1000.0
        feats = np.stack(synth.synth_features(4, 300, 30, seed=fseed))
        _PEAKY[(wseed, fseed)] = (params, weights, feats, ref_numpy.entire_network(feats, weights, params)[1])
    return _PEAKY[(wseed, fseed)]


# the one entry measured above the bar: f16f6, weights 1, features 13, utterance 2, attention_weights 1.13e-4 (the 1000x query's
# softmax amplifies the two-unit layers' ~1e-5 error); checked on its own below, expected to fail, strictly
_KNOWN_OVER = ("f16f6", 1, 13, 2, "attention_weights")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("wseed", [0, 1, 2, 3, 4])
def test_peaky_attention_across_seeds(wseed, precision):
    """query x 1000 (one frame takes nearly all the attention weight) over weight seeds 0-4 and feature seeds 12 / 13:
    attention_weights and the embedding within TOL of the oracle, per utterance (every entry but _KNOWN_OVER)."""
    bad = []
    for fseed in (12, 13):
        params, weights, feats, ep = _peaky_case(wseed, fseed)
        tr = _trainer(params, weights, 30, precision)
        for n in ("attention_weights", "tdnn6_dense"):
            tr.set_embedding(n)
            got = tr.predict(feats)
            for i in range(feats.shape[0]):
                e = _rel(got[i], ep[n][i])
                if e > TOL and (precision, wseed, fseed, i, n) != _KNOWN_OVER:
                    bad.append("%s feats %d utt %d: %.3e" % (n, fseed, i, e))
        tr.close()
    assert not bad, (wseed, precision, bad)


@pytest.mark.xfail(strict=True, reason="f16f6 attention_weights 1.13e-4 > 1e-4 on this entry: the bar stays; a pass means it was fixed")
def test_peaky_attention_known_exceedance():
    precision, wseed, fseed, i, n = _KNOWN_OVER
    params, weights, feats, ep = _peaky_case(wseed, fseed)
    tr = _trainer(params, weights, 30, precision)
    tr.set_embedding(n)
    got = tr.predict(feats)
    tr.close()
    e = _rel(got[i], ep[n][i])
    assert e <= TOL, (_KNOWN_OVER, e)


# ------------------------------------------------------------------------------------- the decision itself
def test_synthetic_models_keep_every_two_unit_layer():
    """Benign statistics (every seed the tests and bench.py use) demote nothing: the default precision keeps its speed."""
    from tf_kaldi_speaker_amd import synth
    for seed in (0, 1, 2, 3, 4, 5, 6, 7):
        params, _ = _tdnn()
        two = _two_unit(params, synth.synth_weights(params, 30, seed=seed), 30, ("tdnn1_conv", "tdnn2_conv", "tdnn3_conv", "tdnn4_dense"))
        assert two == {"tdnn1_conv": False, "tdnn2_conv": True, "tdnn3_conv": True, "tdnn4_dense": False}, (seed, two)
    params, _ = _tdnn(etdnn=True)
    two = _two_unit(params, synth.synth_weights(params, 30, seed=0), 30, ("tdnn3_conv", "tdnn5_conv", "tdnn7_conv", "tdnn4_dense"))
    assert two == {"tdnn3_conv": True, "tdnn5_conv": True, "tdnn7_conv": True, "tdnn4_dense": False}, two
    params, _ = _tdnn(att=True)
    for seed in (2, 6):
        two = _two_unit(params, synth.synth_weights(params, 30, seed=seed), 30, ("tdnn2_conv", "tdnn3_conv", "att_key1_relu"))
        assert two == {"tdnn2_conv": True, "tdnn3_conv": True, "att_key1_relu": False}, (seed, two)
    params = dict(synth.RESNET_PARAMS)
    names = ("conv2b_0", "conv3a", "conv3b_0", "conv4a", "conv4b_0", "conv1a")
    two = _two_unit(params, synth.synth_resnet_weights(params, seed=0), 40, names)
    assert two == dict(zip(names, (True,) * 5 + (False,))), two     # stage 1: 64 channels, no quad of blocks
    tr = _trainer(params, synth.synth_resnet_weights(params, seed=0), 40, "f16x3")
    assert not tr.runs_two_unit("conv3a")                            # only f16f6 has a two-unit kernel
    with pytest.raises(KeyError):
        tr.runs_two_unit("pooling")
    tr.close()
