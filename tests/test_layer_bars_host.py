"""Host: the per-element layer bars of tests/helpers/ref_layer.py are worth having.

One layer at a time (5 taps x 32 channels, 7 x 128, 7 x 512 and a dense layer: K = 160 .. 3584), inputs of the six channel
classes a trained model shows, in the four arithmetics.  Every faithful fp32 emulation of the accumulation -- one rounding per
32-block or one per product, K forwards or backwards -- must meet the bar on every element of every stage endpoint; every
mutant of the computation (a fault a kernel, a packer or an epilogue could really have) must leave the bar on more than half of
the elements it touches.  lambda is the GPU file's own (ref_layer.hoeffding_lambda of layer_cases.checked_elements()).
The restated number formats are compared with tests/analysis/f16f8_error_model.py, and the exact selection cases of the GPU test
are predicted here, where a half-up activation quantiser must change the prediction.  No GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "helpers"))
import ref_layer as rl                                                           # noqa: E402
import layer_cases as lc                                                         # noqa: E402
import pool_cases as pc                                                          # noqa: E402

LAM = rl.hoeffding_lambda(lc.checked_elements())
SHAPES = {"k160": (5, 32, 16), "k896": (7, 128, 16), "k3584": (7, 512, 8), "dense128": (1, 128, 16)}
OUT_LENS = (1, 2, 7)
_cache = {}


def _layer_case(shape, arith):
    """One layer on class inputs: (Layer, weights, reference dict, x, in_offsets)."""
    if (shape, arith) in _cache:
        return _cache[shape, arith]
    w, cin, cout = SHAPES[shape]
    rng = np.random.default_rng(sum(map(ord, shape)))
    L = lc.Layer("t", "tdnn2_%s" % ("conv" if w > 1 else "dense"), 2, w, cin, cout, True, w - 1)
    lim = np.sqrt(6.0 / (w * (cin + cout)))
    weights = {L.kernel_name: rng.uniform(-lim, lim, (w, cin, cout)).astype(np.float32),
               L.bias_name: (0.1 * rng.standard_normal(cout)).astype(np.float32),
               L.bn_scope + "/gamma": rng.uniform(0.5, 1.5, cout).astype(np.float32),
               L.bn_scope + "/beta": (0.1 * rng.standard_normal(cout)).astype(np.float32),
               L.bn_scope + "/moving_mean": (0.1 * rng.standard_normal(cout)).astype(np.float32),
               L.bn_scope + "/moving_variance": rng.uniform(0.5, 1.5, cout).astype(np.float32)}
    g, b = pc.class_affine(rng.uniform(0.5, 1.5, cin), 0.1 * rng.standard_normal(cin))
    offs = np.concatenate([[0], np.cumsum([n + w - 1 for n in OUT_LENS])])
    x = np.maximum(g * rng.standard_normal((offs[-1], cin)) + b, 0.0).astype(np.float32)
    prod = {"p/gamma": g.astype(np.float32), "p/beta": b.astype(np.float32)}
    in_exp = rl.act_exponent(prod, "p") if arith in ("f16x3", "f16f6") else 0
    ref = lc.reference(weights, None, L, {"f16f6": "f16f6"}.get(arith, arith), arith == "f16f6", x, offs, in_exp=in_exp)
    assert ref["arith"] == arith
    _cache[shape, arith] = (L, weights, ref, x, offs)
    return _cache[shape, arith]


def _bars(ref):
    acc = rl.model_acc(ref["terms"])
    bacc = rl.bar_acc(rl.sum_sq_partials(ref["terms"]), LAM)
    out = {}
    for st, vec, act in (("affine", "affine", None), ("bn", "bn", None), ("relu", "bn", "relu")):
        sc, sh = ref["vectors"][vec]
        val, pre = rl.stage(acc, sc, sh, act)
        out[st] = (val, rl.stage_bar(bacc, sc, pre, act), sc, sh, act)
    return acc, bacc, out


@pytest.mark.parametrize("arith", rl.PRECISIONS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_emulations_stay_inside(shape, arith):
    _, _, ref, _, _ = _layer_case(shape, arith)
    acc, bacc, stages = _bars(ref)
    worst = 0.0
    for per_product in (False, True):
        for reverse in (False, True):
            emu = rl.emulate(ref["terms"], per_product, reverse)
            assert (np.abs(emu - acc) <= bacc).all(), (shape, arith, per_product, reverse)
            worst = max(worst, (np.abs(emu - acc) / np.maximum(bacc, 1e-300)).max())
            for st, (val, bar, sc, sh, act) in stages.items():
                got = rl.emulate_stage(emu, sc, sh, act)
                assert (np.abs(got - val) <= bar).all(), (shape, arith, st, per_product, reverse)
    print("%s %s: worst emulation error / bar %.3f (lambda %.2f)" % (shape, arith, worst, LAM))
    assert worst < 0.6          # not vacuous: Hoeffding's lambda ~ 8 over ~1 sigma-ish worst of a few hundred elements


# ---------------------------------------------------------------------------------------------------------------- mutants
def _block_cols(L, blk):
    """the columns of one 32-channel block over all taps: one K block of the kernels, which walk channel blocks with the taps inside"""
    return np.concatenate([np.arange(t * L.cin_pad + 32 * blk, t * L.cin_pad + 32 * blk + 32) for t in range(L.w)])


def _copy(tms):
    return [(A.copy(), W.copy()) for A, W in tms]


def _retake(L, ref, rows):
    return rl.terms(ref["acts"], ref["wts"], ref["arith"], rows)


def m_drop_hi_lo(L, ref, x, offs):
    """one K block's a_hi w_lo dropped (a stale weight fragment)"""
    t = _copy(ref["terms"])
    i = 0 if ref["arith"] == "f16f6" else 1
    t[i][1][_block_cols(L, 0)] = 0
    return t


def m_drop_last_lo_hi(L, ref, x, offs):
    """the last block's a_lo w_hi dropped (the peeled copy of the last quad)"""
    t = _copy(ref["terms"])
    i = 1 if ref["arith"] == "f16f6" else 0
    t[i][1][_block_cols(L, L.cin_pad // 32 - 1)] = 0
    return t


def m_tap_row(L, ref, x, offs):
    """one tap reading row t + j + 1"""
    rows = ref["rows"].copy()
    rows[:, L.w // 2] = np.minimum(rows[:, L.w // 2] + 1, x.shape[0] - 1)
    return _retake(L, ref, rows)


def m_stale_slab(L, ref, x, offs):
    """block c reading block c - 1's activations"""
    t = _copy(ref["terms"])
    for A, _ in t:
        A[:, _block_cols(L, 1)] = A[:, _block_cols(L, 0)]
    return t


def m_scale_exponent(L, ref, x, offs):
    """one block's activation scale one exponent too small"""
    t = _copy(ref["terms"])
    t[0][0][:, _block_cols(L, 0)] *= 0.5
    return t


def m_last_row_next_utt(L, ref, x, offs):
    """an utterance's last output row taking the next utterance's first frame"""
    rows = ref["rows"].copy()
    for b in range(len(offs) - 2):
        rows[ref["out_offsets"][b + 1] - 1] += 1
    return _retake(L, ref, rows)


TERM_MUTANTS = {"drop_a_hi_w_lo": (m_drop_hi_lo, ("bf16x3", "f16x3", "f16f6")),
                "drop_last_a_lo_w_hi": (m_drop_last_lo_hi, ("bf16x3", "f16x3", "f16f6")),
                "tap_row_plus_one": (m_tap_row, rl.PRECISIONS),
                "stale_slab": (m_stale_slab, rl.PRECISIONS),
                "block_scale_exponent": (m_scale_exponent, ("f16f6",)),
                "last_row_next_utterance": (m_last_row_next_utt, rl.PRECISIONS)}
# What the bar cannot separate, by name (DESIGN.md section 2 lists the same).  At K = 3584 on class inputs one block's cross term
# is 1/16 of 2^-9 of a sum whose accumulation noise the bar must allow lambda = 8.2 standard deviations of: the last block's
# a_lo w_hi leaves the bar on 29 - 34 % of the elements (constant and near-constant channels have a small or zero a_lo), the halved
# block scale on 50 %.  They are run and printed, not asserted.
NOT_CAUGHT = {("drop_last_a_lo_w_hi", "k3584", "bf16x3"), ("drop_last_a_lo_w_hi", "k3584", "f16x3"),
              ("drop_last_a_lo_w_hi", "k3584", "f16f6"), ("block_scale_exponent", "k3584", "f16f6")}


def _needs(name, shape):
    return name != "stale_slab" or SHAPES[shape][1] >= 64          # (a stale slab needs a second channel block)


@pytest.mark.parametrize("arith", rl.PRECISIONS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(TERM_MUTANTS))
def test_term_mutant_leaves_the_bar(name, shape, arith):
    fn, ariths = TERM_MUTANTS[name]
    if arith not in ariths or not _needs(name, shape):
        return                                            # the fault does not exist in this arithmetic / shape
    L, _, ref, x, offs = _layer_case(shape, arith)
    acc, bacc, stages = _bars(ref)
    mut = fn(L, ref, x, offs)
    touched = rl.model_acc(mut) != acc
    assert touched.any(), (name, shape, arith, "the mutant changes nothing")
    emu = rl.emulate(mut, per_product=False)
    for st in ("affine", "bn"):
        val, bar, sc, sh, act = stages[st]
        out = np.abs(rl.emulate_stage(emu, sc, sh, act) - val) > bar
        frac = out[touched].mean()
        print("%s %s %s %s: outside the bar on %.0f %% of %d touched elements" % (name, shape, arith, st, 100 * frac, touched.sum()))
        if (name, shape, arith) in NOT_CAUGHT:
            continue
        assert frac > 0.5, (name, shape, arith, st, frac)


@pytest.mark.parametrize("arith", rl.PRECISIONS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_epilogue_mutants_leave_the_bar(shape, arith):
    """scale / shift of channel n ^ 1; 2^e (and the weights' power of two) not undone."""
    L, _, ref, _, _ = _layer_case(shape, arith)
    acc, bacc, stages = _bars(ref)
    emu = rl.emulate(ref["terms"], per_product=False)
    val, bar, sc, sh, act = stages["bn"]
    swap = np.arange(L.cout) ^ 1
    out = np.abs(rl.emulate_stage(emu, sc[swap], sh[swap]) - val) > bar
    assert out.mean() > 0.5, (shape, arith, "neighbour's scale / shift", out.mean())
    if arith in ("f16x3", "f16f6"):
        assert ref["in_exp"] != 0, "the class inputs should need an exponent"
        out = np.abs(rl.emulate_stage(emu, sc * np.float32(2.0 ** ref["in_exp"]), sh) - val) > bar
        assert out.mean() > 0.5, (shape, arith, "2^e not undone", out.mean())


# ------------------------------------------------------------------------------------------------------- restated rules
@pytest.fixture(scope="module")
def em():
    spec = importlib.util.spec_from_file_location("f16f8_error_model", os.path.join(_HERE, "analysis", "f16f8_error_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_number_formats_agree_with_the_error_model(em):
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((40, 96)) * 2.0 ** rng.integers(-12, 12, (40, 96))).astype(np.float32)
    v[3, :32] = 0
    v[5, 40] = 7.5 * 2.0 ** 9                                     # a block maximum exactly at the saturation value
    ties = np.tile(np.array([7.5, 1.0625, 1.1875, 2.125, 2.375, 0.0625, 0.1875, 3.25, 3.75, 5.5, 6.5], np.float32), 3)[:32]
    v[7, :32] = ties                                              # halves of every binade: half-up and half-even part here
    assert np.array_equal(rl.q6_half_up(v), em.q6_blocks(v, 1, rne=False))
    assert np.array_equal(rl.q6_rne(v), em.q6_blocks(v, 1, rne=True))
    assert not np.array_equal(rl.q6_rne(v)[7], rl.q6_half_up(v)[7])
    assert np.array_equal(rl.rn_f16(v), em.f16(v))
    hi = rl.rn_bf16(v)
    assert (np.abs(v - hi) <= np.abs(v) * 2.0 ** -8).all() and np.array_equal(rl.rn_bf16(hi), hi)
    assert rl.rn_bf16(np.float32(1 + 2.0 ** -8)) == 1.0 and rl.rn_bf16(np.float32(1 + 3 * 2.0 ** -8)) == 1 + 2.0 ** -6     # ties to even


def test_wscale_and_act_exponent():
    rng = np.random.default_rng(6)
    for scale in (0.03, 1.0, 37.0, 3e3):
        k = (scale * rng.standard_normal((5, 32, 8))).astype(np.float32)
        ws = rl.wscale(k)
        assert 8192 <= np.abs(k).max() * ws < 16384 and np.log2(ws) == np.round(np.log2(ws))
        w = {"s/gamma": (scale * rng.uniform(0.5, 1.5, 64)).astype(np.float32), "s/beta": (scale * rng.standard_normal(64)).astype(np.float32)}
        e = rl.act_exponent(w, "s")
        rms = np.sqrt(np.mean(w["s/gamma"].astype(np.float64) ** 2 + w["s/beta"].astype(np.float64) ** 2))
        assert 2.0 ** 3.5 <= rms * 2.0 ** e < 2.0 ** 4.5
    assert rl.wscale(np.zeros((1, 32, 4))) == 1.0 and rl.wscale(np.full((1, 32, 4), 1e-30)) == 2.0 ** 24
    assert rl.act_exponent({}, None) == 0 and rl.act_exponent({"s/gamma": np.zeros(4), "s/beta": np.zeros(4)}, "s") == 0
    assert rl.act_exponent({"s/gamma": np.full(4, 1e9), "s/beta": np.zeros(4)}, "s") == -20


def test_lambda_is_the_files_own():
    n = lc.checked_elements()
    assert 1e7 < n < 1e9 and abs(LAM - np.sqrt(2 * np.log(2 * n / 1e-6))) < 1e-12 and 7.5 < LAM < 8.5


# ------------------------------------------------------------------------------------------------------ exact selection
@pytest.mark.parametrize("arith", rl.PRECISIONS)
@pytest.mark.parametrize("value", [1.0, 1.0 + 2.0 ** -12])
def test_selection_cases_are_predictable(arith, value):
    """One non-zero weight per output: every (tap, block) pair and every position of a block is read by some output, the
    products are fp32 numbers, and in f16f6 the prediction depends on the activation quantiser's rounding rule."""
    L, weights, _, x, offs = _layer_case("k896", arith)
    k, used = rl.selection_kernel(L.w, L.cin, 64, value)
    assert {(t, b) for t, b, _ in used} == {(t, b) for t in range(L.w) for b in range(L.cin // 32)}
    assert {p for _, _, p in used} == set(range(32))
    L2 = lc.Layer("t", L.affine, 2, L.w, L.cin, 64, True, L.w - 1)
    ref = lc.reference(weights, None, L2, arith, arith == "f16f6", x, offs, in_exp=-2, kernel=k)
    pred = rl.selection_predictions(ref["terms"], exact_products=arith != "f32")[0]     # (fp32: one fmaf rounds x w)
    allp = rl.selection_predictions(ref["terms"], orders="any", exact_products=arith != "f32")
    assert np.isfinite(pred).all() and (pred != 0).any()
    if value == 1.0 and arith != "f16f6":          # two terms, a_lo + a_hi: x to the bits the split carries, whatever the order
        want = np.concatenate([rl.pad32(x)[ref["rows"][:, t], 32 * b + p][:, None] for t, b, p in used], axis=1).astype(np.float64)
        scale = ref["ws"] * 2.0 ** ref["in_exp"] if arith in ("f16x3", "f16f6") else 1.0
        bits = {"f32": 60, "bf16x3": 16, "f16x3": 21}[arith]      # (fp16: the low half goes subnormal below 2^-3: 2^-25 absolute)
        assert (np.abs(pred / scale - want) <= np.abs(want) * 2.0 ** -bits + 2.0 ** -25 / 2.0 ** ref["in_exp"] * (arith == "f16x3")).all()
        assert (allp == pred).all()
    if arith == "f16f6" and value != 1.0:          # q6(a_hi) shows through w_lo = 2: ties of an 11-bit number on a 4-bit grid
        ref_up = lc.reference(weights, None, L2, arith, True, x, offs, in_exp=-2, kernel=k, quantiser=rl.q6_half_up)
        assert not np.array_equal(rl.selection_predictions(ref_up["terms"])[0], pred), "half-up activations predict the same bits"
