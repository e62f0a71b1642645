"""Host: the per-element bars of the ResNet convolutions (tests/helpers/ref_grid.py, grid_cases.py) are worth having.

One convolution at a time on a ragged batch of even and odd lengths -- stride-1 3 x 3 with a residual, 3 x 3 under frequency and
time stride 2, the 1 x 1 projection shortcut, conv5 -- in the four arithmetics:

  * with "f32" arithmetic the gathered terms ARE oracle/ref_numpy.conv2d, to float64 rounding, for every (stride, parity)
    combination, the shortcut and conv5: window placement and TensorFlow's parity-dependent 'same' padding;
  * every honest fp32 emulation of the accumulation (one rounding per 32-block or per product, K forwards or backwards) followed by
    the fp32 epilogue (fmaf, the residual add, the activation) stays inside the bar on every element;
  * each fault a grid kernel, a row map, a packer or an epilogue could really have leaves the bar on at least one element of the
    same inputs: the window one bin off where the stride-2 padding is asymmetric, a tap taken from the neighbouring utterance's row
    instead of the zero border, the residual added behind the activation, one 32-channel block's cross term dropped, one 32-channel
    K block dropped, a block scale exponent off by one, and half-up instead of nearest-even fp6 codes on a batch of ties;
  * conv0_direct_kernel's model (nine fmaf, worst-case bar) holds its own fp32 emulation and loses a shifted window;
  * the max-pool reference keeps the zero border out of the maximum, and one that lets it in is caught on negative activations.

lambda is the GPU file's own (ref_layer.hoeffding_lambda of grid_cases.checked_elements()).  No GPU."""
import os
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "helpers"))
import ref_layer as rl                                                           # noqa: E402
import ref_grid as rg                                                            # noqa: E402
import grid_cases as gc                                                          # noqa: E402
from oracle import ref_numpy                                                     # noqa: E402

LAM = rl.hoeffding_lambda(gc.checked_elements())
LENS = (1, 2, 3, 4, 5, 6)
#        kind       kh kw cin cout st sw F_in act      residual
KINDS = {"s1_res": ("conv3x3", 3, 3, 128, 16, 1, 1, 6, "prelu", True),
         "s1": ("conv3x3", 3, 3, 32, 16, 1, 1, 6, "lrelu", False),
         "f2": ("conv3x3", 3, 3, 32, 16, 1, 2, 6, "prelu", False),
         "t2f2": ("conv3x3", 3, 3, 64, 16, 2, 2, 6, "lrelu", False),
         "short": ("short", 1, 1, 64, 16, 2, 2, 6, None, False),
         "conv5": ("conv5", 1, 5, 64, 16, 1, 1, 5, "lrelu", False)}
_cache = {}


def _layer(kind):
    k, kh, kw, cin, cout, st, sw, F, act, res = KINDS[kind]
    return gc.Conv("c", k, kh, kw, cin, cout, st, sw, F, 0, "in", "out", "c_bn", act, "c_relu", res_node="r" if res else None,
                   bias=k == "conv5", prod_bn="p_bn")


def _weights(L, rng):
    lim = np.sqrt(6.0 / (L.ntaps * (L.cin + L.cout)))
    w = {L.kernel_name: rng.uniform(-lim, lim, (L.kh, L.kw, L.cin, L.cout)).astype(np.float32),
         L.bn_scope + "/gamma": rng.uniform(0.5, 1.5, L.cout).astype(np.float32),
         L.bn_scope + "/beta": (0.1 * rng.standard_normal(L.cout)).astype(np.float32),
         L.bn_scope + "/moving_mean": (0.1 * rng.standard_normal(L.cout)).astype(np.float32),
         L.bn_scope + "/moving_variance": rng.uniform(0.5, 1.5, L.cout).astype(np.float32),
         L.prod_bn + "/gamma": rng.uniform(0.5, 1.5, L.cin).astype(np.float32),
         L.prod_bn + "/beta": (0.1 * rng.standard_normal(L.cin)).astype(np.float32)}
    if L.bias_name:
        w[L.bias_name] = (0.1 * rng.standard_normal(L.cout)).astype(np.float32)
    if L.alpha_name:
        w[L.alpha_name] = (0.01 + 0.2 * rng.uniform(0, 1, L.cout)).astype(np.float32)
    return w


def _case(kind, arith, ties=False):
    """(Conv, weights, reference dict, x, R): one layer on the ragged batch; `ties`: every activation an fp6 tie."""
    key = (kind, arith, ties)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(sum(map(ord, kind)))
    L = _layer(kind)
    w = _weights(L, rng)
    rows = sum(LENS) * L.F_in
    g, b = w[L.prod_bn + "/gamma"].astype(np.float64), w[L.prod_bn + "/beta"].astype(np.float64)
    z = g * rng.standard_normal((rows, L.cin)) + b
    x = np.where(z > 0, z, 0.1 * z).astype(np.float32)                       # a leaky producer: negative inputs too
    in_exp = gc.input_exponent(w, L, arith)
    if ties:
        # 1.0625 and 1.5625 under a block maximum of 1.5625 (scale 2^-2): 4.25 and 6.25, halfway between the e2m3 neighbours
        # 4 | 4.5 and 6 | 6.5 with the even code below -- nearest-even rounds every one down, half-up every one up
        x = rng.choice(np.array([1.0625, 1.5625], np.float32), size=(rows, L.cin))
        x[:, ::32] = 1.5625
        in_exp = 0
    ref = gc.reference(w, L, arith, x, LENS, in_exp)
    n_out = sum(ref["out_lens"]) * ref["F_out"]
    R = (0.7 * rng.standard_normal((n_out, L.cout))).astype(np.float32) if L.res_node else None
    _cache[key] = (L, w, ref, x, R)
    return _cache[key]


def _bars(L, ref, R):
    acc = rl.model_acc(ref["terms"])
    bacc = rl.bar_acc(rl.sum_sq_partials(ref["terms"]), LAM)
    sc, sh = ref["vectors"]
    val, v, s = rg.residual_stage(acc, sc, sh, R, L.act, ref["alpha"])
    return acc, bacc, val, rg.residual_bar(bacc, sc, v, s, R, L.act, ref["alpha"])


def _out(L, ref, R, tms, val, bar, after=False):
    """elements of the fp32 emulation of `tms` outside the bar"""
    sc, sh = ref["vectors"]
    got = rg.emulate_residual(rl.emulate(tms, per_product=False), sc, sh, R, L.act, ref["alpha"], after=after)
    return np.abs(got.astype(np.float64) - val) > bar


# -------------------------------------------------------------------------------------------------- the gather is the oracle
def _oracle(L, w, x, lens):
    out, pos = [], 0
    for n in lens:
        u = np.asarray(x[pos:pos + n * L.F_in], np.float64).reshape(1, n, L.F_in, L.cin)
        y = ref_numpy.conv2d(u, w[L.kernel_name], strides=(L.st, L.sw), padding=L.padding)
        out.append(y.reshape(-1, L.cout))
        pos += n * L.F_in
    return np.concatenate(out)


@pytest.mark.parametrize("F", [5, 6])
@pytest.mark.parametrize("sw", [1, 2])
@pytest.mark.parametrize("st", [1, 2])
@pytest.mark.parametrize("k", [3, 1])
def test_gather_equals_the_oracle(k, st, sw, F):
    """Every (stride, parity) combination along time (lengths 1 .. 6) and frequency (5 and 6 bins), 3 x 3 and the 1 x 1 shortcut."""
    rng = np.random.default_rng(100 * k + 10 * st + sw + F)
    L = gc.Conv("c", "conv3x3" if k == 3 else "short", k, k, 8, 5, st, sw, F, 0, "in", "out", "c_bn", None)
    w = _weights(gc.Conv("c", L.kind, k, k, 8, 5, st, sw, F, 0, "in", "out", "c_bn", None, prod_bn="p_bn"), rng)
    x = rng.standard_normal((sum(LENS) * F, 8)).astype(np.float32)
    ref = gc.reference(w, L, "f32", x, LENS)
    want = _oracle(L, w, x, LENS)
    got = rl.model_acc(ref["terms"])
    assert ref["out_lens"] == [-(-n // st) for n in LENS] and ref["F_out"] == -(-F // sw)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # 'same' under stride 2: an even size pads 0 in front, an odd size 1
    assert rg.same_pad(6, 3, 2) == (3, 0) and rg.same_pad(5, 3, 2) == (3, 1) and rg.same_pad(6, 3, 1) == (6, 1) and rg.same_pad(6, 1, 2) == (3, 0)


def test_gather_of_conv5_equals_the_oracle():
    L, w, ref, x, _ = _case("conv5", "f32")
    want = _oracle(L, w, x, LENS)
    got = rl.model_acc(ref["terms"])
    assert ref["F_out"] == 1 and ref["out_lens"] == list(LENS) and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert (ref["idx"] >= 0).all()                                            # 'valid': no padding at all


# -------------------------------------------------------------------------------------------------------- honest emulations
@pytest.mark.parametrize("arith", rl.PRECISIONS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_emulations_stay_inside(kind, arith):
    L, _, ref, _, R = _case(kind, arith)
    acc, bacc, val, bar = _bars(L, ref, R)
    sc, sh = ref["vectors"]
    worst = 0.0
    for per_product in (False, True):
        for reverse in (False, True):
            emu = rl.emulate(ref["terms"], per_product, reverse)
            assert (np.abs(emu - acc) <= bacc).all(), (kind, arith, per_product, reverse)
            got = rg.emulate_residual(emu, sc, sh, R, L.act, ref["alpha"])
            ratio = np.abs(got.astype(np.float64) - val) / np.maximum(bar, 1e-300)
            assert (ratio <= 1).all(), (kind, arith, per_product, reverse, ratio.max())
            worst = max(worst, ratio.max())
    print("%s %s: worst emulation error / bar %.3f (lambda %.2f)" % (kind, arith, worst, LAM))
    assert worst < 0.6          # not vacuous


# ------------------------------------------------------------------------------------------------------------------ faults
def _block_cols(L, blk, cin_pad):
    return np.concatenate([np.arange(t * cin_pad + 32 * blk, t * cin_pad + 32 * blk + 32) for t in range(L.ntaps)])


def _copy(tms):
    return [(A.copy(), W.copy()) for A, W in tms]


# zeros in front (time, frequency) as a kernel with symmetric padding would place them.  f2: time 1 is right, frequency 1 is wrong
# (6 bins: TensorFlow pads 0 / 1); t2f2: frequency 0 is right, time 1 is wrong for the even utterances; the shortcut pads nothing.
WRONG_PADS = {"f2": [(1, 1)], "t2f2": [(1, 0)], "short": [(0, 1), (1, 0)]}


@pytest.mark.parametrize("arith", rl.PRECISIONS)
@pytest.mark.parametrize("kind", sorted(WRONG_PADS))
def test_shifted_window_leaves_the_bar(kind, arith):
    """The window one bin (one frame) off where the stride-2 padding is asymmetric; for the 1 x 1 shortcut, the centre one off."""
    L, w, ref, x, R = _case(kind, arith)
    acc, bacc, val, bar = _bars(L, ref, R)
    for pad in WRONG_PADS[kind]:
        mut = gc.reference(w, L, arith, x, LENS, ref["in_exp"], pad_before=pad)
        assert mut["idx"].shape == ref["idx"].shape and not np.array_equal(mut["idx"], ref["idx"])
        out = _out(L, ref, R, mut["terms"], val, bar)
        assert out.any(), (kind, arith, pad)
        print("%s %s pad %s: %.0f %% outside" % (kind, arith, pad, 100 * out.mean()))


@pytest.mark.parametrize("arith", rl.PRECISIONS)
@pytest.mark.parametrize("kind", ["s1_res", "s1", "t2f2"])
def test_neighbour_utterance_instead_of_the_border_leaves_the_bar(kind, arith):
    L, w, ref, x, R = _case(kind, arith)
    acc, bacc, val, bar = _bars(L, ref, R)
    mut = gc.reference(w, L, arith, x, LENS, ref["in_exp"], clip_time=False)
    assert ((mut["idx"] >= 0) & (ref["idx"] < 0)).any()
    assert _out(L, ref, R, mut["terms"], val, bar).any(), (kind, arith)


@pytest.mark.parametrize("arith", rl.PRECISIONS)
def test_residual_behind_the_activation_leaves_the_bar(arith):
    L, _, ref, _, R = _case("s1_res", arith)
    acc, bacc, val, bar = _bars(L, ref, R)
    assert not _out(L, ref, R, ref["terms"], val, bar).any()
    out = _out(L, ref, R, ref["terms"], val, bar, after=True)
    assert out.any(), arith
    print("%s: %.0f %% outside" % (arith, 100 * out.mean()))


@pytest.mark.parametrize("arith", ["bf16x3", "f16x3", "f16f6"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_dropped_cross_term_leaves_the_bar(kind, arith):
    """a_lo w_hi of ONE 32-channel block (q6(a_lo) q6(w_hi) in f16f6) missing."""
    L, _, ref, _, R = _case(kind, arith)
    acc, bacc, val, bar = _bars(L, ref, R)
    mut = _copy(ref["terms"])
    mut[1 if arith == "f16f6" else 0][1][_block_cols(L, 0, L.cin)] = 0
    out = _out(L, ref, R, mut, val, bar)
    assert out.any(), (kind, arith)
    print("%s %s: %.0f %% outside" % (kind, arith, 100 * out.mean()))


@pytest.mark.parametrize("arith", rl.PRECISIONS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_dropped_k_block_leaves_the_bar(kind, arith):
    """one K step -- 32 channels of one tap -- lost"""
    L, _, ref, _, R = _case(kind, arith)
    acc, bacc, val, bar = _bars(L, ref, R)
    mut = _copy(ref["terms"])
    k0 = 32 * (ref["terms"][0][0].shape[1] // 64)             # a block of the centre tap: no output has padding there
    for A, _ in mut:
        A[:, k0:k0 + 32] = 0
    assert (rl.model_acc(mut) != acc).all()
    assert _out(L, ref, R, mut, val, bar).mean() > 0.5, (kind, arith)


@pytest.mark.parametrize("kind", ["s1_res", "s1"])
def test_block_scale_exponent_leaves_the_bar(kind):
    """one 32-channel block of q6(a_hi) under a scale one exponent too small"""
    L, _, ref, _, R = _case(kind, "f16f6")
    acc, bacc, val, bar = _bars(L, ref, R)
    mut = _copy(ref["terms"])
    mut[0][0][:, _block_cols(L, 0, L.cin)] *= 0.5
    out = _out(L, ref, R, mut, val, bar)
    assert out.any(), kind
    print("%s: %.0f %% outside" % (kind, 100 * out.mean()))


@pytest.mark.parametrize("kind", ["s1_res", "s1"])
def test_half_up_fp6_codes_leave_the_bar_on_ties(kind):
    L, w, ref, x, R = _case(kind, "f16f6", ties=True)
    acc, bacc, val, bar = _bars(L, ref, R)
    assert not np.array_equal(rl.q6_rne(rl.pad32(x)), rl.q6_half_up(rl.pad32(x))), "the batch holds no tie"
    assert not _out(L, ref, R, ref["terms"], val, bar).any()
    mut = gc.reference(w, L, "f16f6", x, LENS, 0, quantiser=rl.q6_half_up)
    out = _out(L, ref, R, mut["terms"], val, bar)
    assert out.any(), kind
    print("%s: %.0f %% outside" % (kind, 100 * out.mean()))


# ------------------------------------------------------------------------------------------------------------------- conv0
def _conv0_case(act):
    rng = np.random.default_rng(9)
    L = gc.Conv("conv0_1", "conv0", 3, 3, 1, 16, 1, 1, 8, 0, None, "conv0_relu", "conv0_bn", act, "conv0_relu")
    w = _weights(gc.Conv("conv0_1", "conv0", 3, 3, 1, 16, 1, 1, 8, 0, None, "o", "conv0_bn", act, "conv0_relu", prod_bn="p_bn"), rng)
    x = rng.standard_normal(sum(LENS) * 8).astype(np.float32)
    return L, w, x


@pytest.mark.parametrize("act", ["prelu", "lrelu"])
def test_conv0_direct_model(act):
    """The direct kernel's model holds its fp32 emulation, equals the im2col model's exact product, and loses a shifted window."""
    L, w, x = _conv0_case(act)
    idx, out_lens, F_out = rg.gather_windows(LENS, L.F_in, 3, 3, 1, 1)
    sc, sh = rg.vectors(w, L.bn_scope, L.cout)
    alpha = w[L.alpha_name] if L.alpha_name else None
    val, bar = rg.conv0_direct(x, idx, w[L.kernel_name], sc, sh, act, alpha)
    emu = rg.emulate_conv0_direct(x, idx, w[L.kernel_name], sc, sh, act, alpha)
    ratio = np.abs(emu.astype(np.float64) - val) / np.maximum(bar, 1e-300)
    assert (ratio <= 1).all() and ratio.max() > 0.05, ratio.max()
    ref = gc.reference(w, L, "f32", x, LENS)
    assert ref["terms"][0][0].shape[1] == 32 and (ref["terms"][0][0][:, 9:] == 0).all()          # nine taps in a K of 32
    exact = rg.residual_stage(rl.model_acc(ref["terms"]), sc, sh, None, act, alpha)[0]
    assert np.abs(exact - val).max() <= 1e-13 * np.abs(val).max()
    bad, _, _ = rg.gather_windows(LENS, L.F_in, 3, 3, 1, 1, pad_before=(1, 0))
    emu = rg.emulate_conv0_direct(x, bad, w[L.kernel_name], sc, sh, act, alpha)
    assert (np.abs(emu.astype(np.float64) - val) > bar).mean() > 0.5
    # the interval a max over such outputs must lie in holds the max of the emulation, and not one with the border in it
    lo, hi = rg.maxpool_interval(val - bar, val + bar, LENS, L.F_in)
    got = rg.maxpool3x3(rg.emulate_conv0_direct(x, idx, w[L.kernel_name], sc, sh, act, alpha), LENS, L.F_in)
    assert ((got >= lo) & (got <= hi)).all()
    wrong = rg.maxpool3x3(rg.emulate_conv0_direct(x, idx, w[L.kernel_name], sc, sh, act, alpha), LENS, L.F_in, border_takes_part=True)
    assert ((wrong < lo) | (wrong > hi)).any()


# ---------------------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("act", ["prelu", "lrelu"])
def test_maxpool_reference_keeps_the_border_out(act):
    rng = np.random.default_rng(3)
    F, C = 6, 8
    x = rng.standard_normal((sum(LENS) * F, C))
    x = np.where(x > 0, x, (0.2 if act == "lrelu" else 0.11) * x) - 0.5        # mostly negative, as a leaky activation leaves them
    got = rg.maxpool3x3(x, LENS, F)
    want, pos = [], 0
    for n in LENS:
        want.append(ref_numpy.max_pool_3x3_same(x[pos:pos + n * F].reshape(1, n, F, C)).reshape(-1, C))
        pos += n * F
    assert np.array_equal(got, np.concatenate(want))
    wrong = rg.maxpool3x3(x, LENS, F, border_takes_part=True)
    assert (wrong != got).any() and (wrong >= got).all()
    inner = rg.gather_windows(LENS, F, 3, 3, 1, 1)[0].min(axis=1) >= 0          # windows that touch no border agree
    assert np.array_equal(wrong[inner], got[inner]) and (wrong[~inner] == 0).any()


def test_cases_and_lambda():
    gc.check_batches()
    n = gc.checked_elements()
    assert 1e6 < n < 1e9 and abs(LAM - np.sqrt(2 * np.log(2 * n / 1e-6))) < 1e-12 and 7.0 < LAM < 8.5
    for model in gc.MODELS:
        for setting in gc.SETTINGS:
            ls = gc.layers(model, setting)
            assert len(ls) == 1 + 4 * 3 + 3 * 2 + 3
            for order in (0, 1):
                for L in ls:
                    gc.gemm_rows(L, setting, order)
    two = [L.name for L in gc.layers("r32", "plain") if gc.two_unit_eligible(L)]
    assert two == ["conv3a_conv1", "conv3b_0_conv0", "conv3b_0_conv1", "conv4a_conv1", "conv4b_0_conv0", "conv4b_0_conv1"]
    assert not any(gc.two_unit_eligible(L) for L in gc.layers("r8", "plain"))
