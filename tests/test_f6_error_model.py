"""CPU: the numpy emulation of the two-unit split (tests/analysis/f16f8_error_model.py) as a checked artefact.

* its fp6 quantiser against the rules of csrc/xv_f6.h: in half-up mode bit for bit against e2m3_code / e8m0_of (mirrored below; the
  weight packer host_e2m3 is the same code): E8M0 scale 2^ceil(log2(amax / 7.5)), saturation at 7.5, subnormal steps of 1/8,
  magnitudes rounded half up; the activations go through the hardware converters, which round to nearest even (rne=True, hand-picked
  ties only; the converters themselves run in tests/test_gpu_layer_isolated.py, whose exact selection cases compare their codes
  with this rule bit for bit on the GPU);
* the hazard the library's demotion exists for: a compensated per-channel spread inside the 32-channel blocks (same function) pushes
  the two-unit reader beyond 1e-4, and the same model with that reader on f16x3 is back at the benign figure."""
import importlib.util
import os

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def em():
    spec = importlib.util.spec_from_file_location("f16f8_error_model", os.path.join(_HERE, "analysis", "f16f8_error_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _kernel_q6(block):
    """e8m0_of + e2m3_code of csrc/xv_f6.h on a float32 block of 32, decoded back to values."""
    x = np.asarray(block, np.float32)
    amax = np.float32(np.abs(x).max())
    if not amax > 0:
        return np.zeros(32)
    r = np.float32(amax * np.float32(1.0 / 7.5))
    e = int((int(r.view(np.uint32)) + 0x7FFFFF) >> 23) - 127
    inv = np.uint32((127 - e) << 23).view(np.float32)
    out = np.zeros(32)
    for i, xv in enumerate(x):
        v = min(np.float32(abs(xv) * inv), np.float32(7.5))
        sub = v < 1.0
        t = np.float32(v + np.float32(1.0)) if sub else np.float32(v)
        c = ((int(t.view(np.uint32)) + 0x80000) >> 20) - (126 << 3) - (8 if sub else 0)
        c = min(c, 31)
        ef, m = c >> 3, c & 7
        mag = m / 8.0 if ef == 0 else (1.0 + m / 8.0) * 2.0 ** (ef - 1)
        out[i] = -mag * 2.0 ** e if xv < 0 else mag * 2.0 ** e
    return out


def test_q6_hand_picked_values(em):
    v = np.zeros(32)
    v[:10] = [7.5, 0.0625, 0.05, 1.0625, 2.0625, 2.125, -2.125, 7.4, 3.3, -0.1875]
    want = np.zeros(32)
    want[:10] = [7.5, 0.125, 0.0, 1.125, 2.0, 2.25, -2.25, 7.5, 3.25, -0.25]       # half up on the magnitude; steps 1/8 below 1
    np.testing.assert_array_equal(em.q6_blocks(v, 0), want)
    np.testing.assert_array_equal(em.q6_blocks(v * 2.0 ** -5, 0), want * 2.0 ** -5)  # the scale is a power of two
    np.testing.assert_array_equal(em.q6_blocks(v * 2.0 ** 9, 0), want * 2.0 ** 9)
    want_rne = want.copy()
    want_rne[[1, 3, 5, 6]] = [0.0, 1.0, 2.0, -2.0]                                 # ties to the even code instead
    np.testing.assert_array_equal(em.q6_blocks(v, 0, rne=True), want_rne)


def test_q6_scale_and_saturation(em):
    v = np.zeros(32)
    v[0], v[1] = 7.6, 0.1                              # amax / 7.5 just above 1: scale 2, the largest becomes 3.8 -> 3.75 x 2
    q = em.q6_blocks(v, 0)
    assert q[0] == 7.5 and q[1] == 0.0                  # 0.05 < 1/16 of the scale: flushed
    v[0] = 15.0                                         # exactly 7.5 x 2: no saturation loss
    assert em.q6_blocks(v, 0)[0] == 15.0
    rs = np.random.RandomState(0)
    for k in range(200):
        b = rs.standard_normal(32) * 2.0 ** rs.uniform(-20, 20)
        amax = np.abs(b).max()
        s = 2.0 ** np.ceil(np.log2(amax / 7.5))
        q = em.q6_blocks(b, 0)
        assert np.abs(q).max() <= 7.5 * s
        assert np.all(np.abs(q / s * 8 - np.round(q / s * 8)) == 0)   # on the e2m3 grid (multiples of 1/8 of the scale at least)


def test_q6_matches_the_kernel_rules(em):
    rs = np.random.RandomState(1)
    blocks = [rs.standard_normal(32).astype(np.float32) * np.float32(2.0 ** rs.uniform(-30, 30)) for _ in range(300)]
    grid = (np.arange(32) - 16).astype(np.float32) / np.float32(16)        # ties of every subnormal / normal step
    blocks += [grid * np.float32(7.5 / 1.0), grid * np.float32(2.0 ** -12)]
    blocks += [(rs.standard_normal(32) * 2.0 ** rs.uniform(-8, 0, 32)).astype(np.float32) for _ in range(100)]   # spread in a block
    for b in blocks:
        np.testing.assert_array_equal(em.q6_blocks(b.astype(np.float64), 0), _kernel_q6(b))


def test_f16_split_keeps_22_bits(em):
    rs = np.random.RandomState(2)
    x = (rs.choice([-1.0, 1.0], 4096) * 2.0 ** rs.uniform(-3, 15.9, 4096)).astype(np.float32).astype(np.float64)   # |x| in [2^-3, 65504)
    hi = em.f16(x)
    lo = em.f16(x - hi)                                # what the f16x3 kernels and the emulation use
    assert np.all(np.abs(x - hi - lo) <= 2.0 ** -21 * np.abs(x))


# ----------------------------------------------------------------------------------------------- the hazard
def _spread_tdnn(s, seed=0):
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.TDNN_STAT_PARAMS)
    base = dict(synth.synth_weights(params, 30, seed=seed))
    w = dict(base)
    if s:
        f = 2.0 ** np.random.RandomState(102).uniform(-s, s, 512)
        for nm in ("gamma", "beta"):
            w["tdnn/tdnn2_bn/" + nm] = (w["tdnn/tdnn2_bn/" + nm] * f).astype(np.float32)
        w["tdnn/tdnn3_conv/kernel"] = (w["tdnn/tdnn3_conv/kernel"] / f[:, None]).astype(np.float32)
    feats = np.stack(synth.synth_features(2, 64, 30, seed=5))
    return params, w, feats


def _err(ep, ex, node):
    return float(np.linalg.norm(ep[node] - ex[node]) / np.linalg.norm(ex[node]))


def test_block_scale_hazard_and_the_f16x3_fallback(em):
    from oracle import ref_numpy
    params, w, feats = _spread_tdnn(0)
    _, ex = ref_numpy.entire_network(feats, w, params)
    ep = em.network(feats, w, params)
    for node in ("tdnn2_conv", "tdnn3_conv"):
        assert _err(ep, ex, node) <= 2e-5, (node, "benign", _err(ep, ex, node))
    params, w, feats = _spread_tdnn(6)
    _, ex6 = ref_numpy.entire_network(feats, w, params)
    assert _err(ex6, ex, "tdnn3_conv") <= 1e-6                      # the same function
    ep = em.network(feats, w, params)
    assert _err(ep, ex6, "tdnn3_conv") > 1e-4, _err(ep, ex6, "tdnn3_conv")
    ep = em.network(feats, w, params, demote=("tdnn/tdnn3_conv/kernel",))
    for node in ("tdnn2_conv", "tdnn3_conv", "tdnn3_relu"):
        assert _err(ep, ex6, node) <= 2e-5, (node, "demoted", _err(ep, ex6, node))


def test_emulation_selects_the_two_unit_layers(em):
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.TDNN_STAT_PARAMS)
    w = synth.synth_weights(params, 30, seed=0)
    assert [em.two_unit_eligible(w["tdnn/tdnn%d_conv/kernel" % i]) for i in (1, 2, 3)] == [False, True, True]
    assert not em.two_unit_eligible(w["tdnn/tdnn4_dense/kernel"])
    w128 = synth.synth_weights(params, 30, seed=0, channels=64)
    assert not em.two_unit_eligible(w128["tdnn/tdnn2_conv/kernel"])
