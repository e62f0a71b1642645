"""Host: the per-element pooling bars of tests/helpers/ref_pool.py are worth having.

Frames of the six channel classes a trained model shows (ordinary, near-constant, near-constant and large, dead, exactly
constant, sparse) are generated directly, at the utterance lengths and tile offsets of the GPU test.  Every faithful fp32
emulation of a pooling kernel must meet every bar on every element; every mutant of one must leave a bar on at least one
element of a class named here.  No GPU, no model (but for the one check that the moderate query scale of
tests/helpers/pool_cases.py keeps E_s below 1e-3 on the oracle's key)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_pool as rp                                                            # noqa: E402
import pool_cases                                                                # noqa: E402

LENGTHS = pool_cases.LENGTHS
C = 24                                                                           # four channels of each class
CLS = pool_cases.class_of(C)
NAMES = pool_cases.CLASS_NAMES


def _frames(rng, n):
    """[n, C] fp32 frames: ReLU of gamma z + beta with the class parameters of pool_cases.class_affine."""
    z = rng.standard_normal((n, C))
    g = rng.uniform(0.5, 1.5, C)
    gamma, beta = pool_cases.class_affine(g, 0.1 * rng.standard_normal(C))
    return np.maximum(gamma * z + beta, 0.0).astype(np.float32)


def _batches(seed):
    """Both pack orders: (frames [n, C], packed row of the first frame, previous utterance's last frame)."""
    rng = np.random.default_rng(seed)
    out = []
    for order in pool_cases.PACK_ORDERS:
        r0, prev = 0, None
        for n in order:
            x = _frames(rng, n)
            out.append((x, r0, prev))
            r0 += n
            prev = x[-1]
    return out


BATCH = _batches(1)
STAT_EMUS = {"stat_pool_kernel": lambda x, r0, **m: rp.emu_stat_pool(x, **m),
             "tile8": lambda x, r0, **m: rp.emu_stat_fused(x, r0, 8, **m),
             "tile4": lambda x, r0, **m: rp.emu_stat_fused(x, r0, 4, **m),
             "tile16": lambda x, r0, **m: rp.emu_stat_fused(x, r0, 16, **m)}


def _weights(rng, n, H, spread):
    s = spread * rng.standard_normal((n, H))
    e = np.exp(s - s.max(axis=0))
    return (e / e.sum(axis=0)).astype(np.float32)


def _misses(rm, rs):
    """class name -> True where some element of the class leaves a bar."""
    bad = (rm > 1) | (rs > 1)
    return {NAMES[c] for c in range(6) if bad[CLS == c].any()}


# ------------------------------------------------------------------------------------------------------ the classes
def test_classes_are_what_they_claim():
    x = _frames(np.random.default_rng(0), 4000).astype(np.float64)
    m, sd = x.mean(axis=0), x.std(axis=0)
    for c in range(C):
        k = NAMES[CLS[c]]
        if k == "near_constant":
            assert 2 ** 10 <= m[c] / sd[c] <= 2 ** 14, (c, m[c] / sd[c])
        elif k == "near_constant_large":
            assert 2 ** 10 <= m[c] / sd[c] <= 2 ** 15 and m[c] > 150
        elif k == "dead":
            assert (x[:, c] == 0).all()
        elif k == "constant":
            assert (x[:, c] == 3).all()
        elif k == "sparse":
            assert 0.002 <= (x[:, c] > 0).mean() <= 0.03
        else:
            assert 0.3 <= abs(m[c]) / sd[c] <= 3
    assert len({CLS[c] for c in range(4)}) == 4                                  # one lane's four columns: four classes


def test_pack_orders_put_borders_where_the_tiles_can_go_wrong():
    offs, first, last = pool_cases.border_offsets()
    assert {0, 1, 63} <= offs
    assert 1 in first and 1 in last              # slots of one frame (n_i = 1, M2_i = 0) at either end of an utterance
    for order in pool_cases.PACK_ORDERS:
        assert sorted(order) == sorted(LENGTHS)


# ------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("emu", sorted(STAT_EMUS))
def test_faithful_statistics_emulations_meet_every_bar(emu):
    worst = 0.0
    for x, r0, _ in BATCH + [(_frames(np.random.default_rng(5), 12000), 37, None)]:
        mean, std = STAT_EMUS[emu](x, r0)
        rm, rs = rp.stat_check(x, r0, mean, std)
        assert (rm <= 1).all() and (rs <= 1).all(), (emu, x.shape[0], r0, rm.max(), rs.max())
        worst = max(worst, rm.max(), rs.max())
        dead = CLS == NAMES.index("dead")
        assert (mean[dead] == 0).all() and (std[dead] == np.sqrt(np.float32(1e-12))).all()
    assert worst > 0                                                             # the emulations do round


def _stat_mutant_misses(emu, mutate):
    """Classes on which the mutant leaves a bar anywhere in the batch."""
    missed = set()
    for x, r0, prev in BATCH:
        got = mutate(STAT_EMUS[emu], x, r0, prev)
        if got is None:
            continue
        missed |= _misses(*rp.stat_check(x, r0, *got))
    return missed


@pytest.mark.parametrize("emu", sorted(STAT_EMUS))
def test_statistics_mutants_leave_a_bar(emu):
    fused = emu != "stat_pool_kernel"
    if not fused:                                # one-pass variance: where |mean| / std is large
        miss = _stat_mutant_misses(emu, lambda f, x, r0, p: f(x, r0, one_pass=True))
        assert {"near_constant", "near_constant_large"} <= miss, miss
    else:                                        # merge without n_i d^2: wherever the slot means differ
        miss = _stat_mutant_misses(emu, lambda f, x, r0, p: f(x, r0, no_between=True))
        assert {"ordinary", "sparse", "near_constant", "near_constant_large"} <= miss, miss
        assert not miss & {"dead", "constant"}
    miss = _stat_mutant_misses(emu, lambda f, x, r0, p: f(x[:-1], r0) if x.shape[0] > 1 else None)
    assert {"ordinary", "sparse"} <= miss, miss                                   # last frame dropped
    miss = _stat_mutant_misses(emu, lambda f, x, r0, p: f(np.vstack([p[None], x[1:]]), r0) if p is not None else None)
    assert {"ordinary", "near_constant", "near_constant_large"} <= miss, miss     # first frame from the neighbour
    # variance not floored (a one-frame utterance has no variance in any class; a short one none in a sparse channel)
    miss = _stat_mutant_misses(emu, lambda f, x, r0, p: f(x, r0, no_floor=True) if x.shape[0] > 1 else None)
    assert {"dead", "constant"} <= miss and not miss & {"near_constant", "near_constant_large"}, miss


# -------------------------------------------------------------------------------------------------------- attention
def _att_cases(spread, H, seed):
    rng = np.random.default_rng(seed)
    return [(x, r0, prev, _weights(rng, x.shape[0], H, spread)) for x, r0, prev in BATCH]


ATT_EMUS = {"att_pool_kernel": lambda x, w, r0, **m: rp.emu_att_pool(x, w, **m),
            "fused": lambda x, w, r0, **m: rp.emu_att_fused(x, w, r0, **m)}
SPREADS = {"moderate": 1.5, "peaked": 200.0}


def _att_run(emu, x, w, r0, split, head_shift=0, **m):
    fn = ATT_EMUS[emu]
    return rp.emu_att_heads(lambda xc, wh, **kw: fn(xc, wh, r0, **kw), x, w, split, head_shift, **m)


def _zero_slots(w, r0):
    """64-row slots of the utterance whose fp32 weights sum to exactly zero."""
    n, i, z = w.shape[0], 0, 0
    for _, ni in rp._segments(r0, n):
        z += int((w[i:i + ni].sum(axis=0) == 0).any())
        i += ni
    return z


@pytest.mark.parametrize("regime", sorted(SPREADS))
@pytest.mark.parametrize("H,split", [(1, True), (3, False), (2, True)])
@pytest.mark.parametrize("emu", sorted(ATT_EMUS))
def test_faithful_attention_emulations_meet_every_bar(emu, H, split, regime):
    zero_slots = 0
    for x, r0, _, w in _att_cases(SPREADS[regime], H, 7):
        mean, std = _att_run(emu, x, w, r0, split)
        rm, rs = rp.att_check(x, w, split, r0, mean, std)
        assert (rm <= 1).all() and (rs <= 1).all(), (emu, x.shape[0], r0, rm.max(), rs.max())
        if x.shape[0] >= 300:
            zero_slots += _zero_slots(w, r0)
        if x.shape[0] == 1:                      # one frame: weight exactly 1, mean = the frame, std at the floor
            assert (w == 1).all() and (std == np.sqrt(np.float32(1e-12))).all()
            assert np.array_equal(mean, np.tile(x[0], 1 if split else H))
    if regime == "peaked":
        assert zero_slots > 0                    # what reaches the w > 0 branch of att_pool_finalize_kernel


def _subnormal_slot_case():
    """A 300-frame utterance whose third slot carries nothing but subnormal weights (scores 92 .. 100 below the maximum)."""
    rng = np.random.default_rng(11)
    x = _frames(rng, 300)
    s = rng.uniform(-8.0, 0.0, (300, 1))
    s[128:192] = rng.uniform(-100.0, -92.0, (64, 1))
    e = np.exp(s - s.max())
    w = (e / e.sum()).astype(np.float32)
    assert (w[128:192] > 0).all() and w[128:192].sum() < 2.0 ** -128
    return x, w


def test_a_slot_of_subnormal_weights_stays_finite():
    """The reciprocal of a subnormal slot weight overflows: `s1 * (1 / s0)` as the value epilogue first had it gives an
    infinite slot mean and a NaN variance.  The epilogue takes the reciprocal of normal sums only (csrc/xv_epilogue_n32.h); the
    emulation of the earlier form is kept as a mutant and must fail."""
    x, w = _subnormal_slot_case()
    mean, std = rp.emu_att_heads(lambda xc, wh: rp.emu_att_fused(xc, wh, 0), x, w, True)
    rm, rs = rp.att_check(x, w, True, 0, mean, std)
    assert (rm <= 1).all() and (rs <= 1).all(), (rm.max(), rs.max())
    mean, std = rp.emu_att_heads(lambda xc, wh: rp.emu_att_fused(xc, wh, 0, safe_inverse=False), x, w, True)
    rm, rs = rp.att_check(x, w, True, 0, mean, std)
    assert not np.isfinite(std).all() and (rs > 1).any()
    mean, std = rp.emu_att_heads(lambda xc, wh: rp.emu_att_pool(xc, wh), x, w, True)          # the unfused kernel never divides
    rm, rs = rp.att_check(x, w, True, 0, mean, std)
    assert (rm <= 1).all() and (rs <= 1).all()


def _att_mutant_misses(emu, H, split, spread, mutate):
    missed = set()
    for x, r0, prev, w in _att_cases(spread, H, 7):
        got = mutate(x, w, r0, prev)
        if got is None:
            continue
        rm, rs = rp.att_check(x, w, split, r0, *got)
        bad = (rm > 1) | (rs > 1)
        cls = CLS if split else np.tile(CLS, H)
        missed |= {NAMES[c] for c in range(6) if bad[cls == c].any()}
    return missed


@pytest.mark.parametrize("emu", sorted(ATT_EMUS))
def test_attention_mutants_leave_a_bar(emu):
    H, split, spread = 2, True, SPREADS["moderate"]
    run = lambda x, w, r0, **m: _att_run(emu, x, w, r0, split, **m)              # noqa: E731
    if emu == "att_pool_kernel":
        miss = _att_mutant_misses(emu, H, split, spread, lambda x, w, r0, p: run(x, w, r0, one_pass=True))
        assert {"near_constant", "near_constant_large"} <= miss, miss
    else:
        miss = _att_mutant_misses(emu, H, split, spread, lambda x, w, r0, p: run(x, w, r0, no_between=True))
        assert {"ordinary", "sparse", "near_constant", "near_constant_large"} <= miss, miss
        # without the w > 0 branch a slot of zero weight divides 0 by 0
        miss = _att_mutant_misses(emu, H, split, SPREADS["peaked"], lambda x, w, r0, p: run(x, w, r0, no_zero_branch=True))
        assert {"ordinary", "near_constant", "constant"} <= miss, miss
    miss = _att_mutant_misses(emu, H, split, spread, lambda x, w, r0, p: run(x[:-1], w[:-1], r0) if x.shape[0] > 1 else None)
    assert {"ordinary", "sparse"} <= miss, miss
    miss = _att_mutant_misses(emu, H, split, spread,
                              lambda x, w, r0, p: run(np.vstack([p[None], x[1:]]), w, r0) if p is not None else None)
    assert {"ordinary", "near_constant", "near_constant_large"} <= miss, miss
    miss = _att_mutant_misses(emu, H, split, spread, lambda x, w, r0, p: run(x, w, r0, no_floor=True) if x.shape[0] > 1 else None)
    assert {"dead", "constant"} <= miss and not miss & {"near_constant", "near_constant_large"}, miss
    for hh, sp in ((2, True), (3, False)):       # the weights of head h on the columns of head h + 1
        miss = _att_mutant_misses(emu, hh, sp, spread, lambda x, w, r0, p: _att_run(emu, x, w, r0, sp, head_shift=1))
        assert {"ordinary", "sparse", "near_constant", "near_constant_large"} <= miss, (hh, miss)


# ---------------------------------------------------------------------------------------------------------- weights
def test_weight_bar_holds_for_an_fp32_softmax_and_catches_a_wrong_head():
    rng = np.random.default_rng(3)
    n, dk, H = 300, 48, 3
    key = np.maximum(rng.standard_normal((n, dk)), 0).astype(np.float32)
    query = (0.4 * rng.standard_normal((H, dk))).astype(np.float32)
    scale = 1.0 / np.sqrt(dk)
    ref = rp.softmax_weights(key, query, scale, H, False)
    bar = rp.weight_bar(n, rp.score_bar(key, query, scale, H, False))
    s = np.zeros((n, H), dtype=np.float32)       # att_scores_kernel: 64 lanes stride the key, then a butterfly
    for h in range(H):
        lanes = np.zeros((n, 64), dtype=np.float32)
        lanes[:, :dk] = rp._fma(key, query[h], 0.0)
        while lanes.shape[1] > 1:
            half = lanes.shape[1] // 2
            lanes = lanes[:, :half] + lanes[:, half:]
        s[:, h] = lanes[:, 0] * np.float32(scale)
    e = np.exp(s - s.max(axis=0))
    got = e * (np.float32(1.0) / e.sum(axis=0, dtype=np.float32))
    assert (rp.weight_ratio(got, ref, bar) <= 1).all()
    assert (rp.weight_ratio(np.roll(got, 1, axis=1), ref, bar) > 1).any()
    assert (rp.weight_ratio(np.roll(got, 1, axis=0), ref, bar) > 1).any()         # one frame late


def test_moderate_query_scale_keeps_the_score_bar_small():
    """E_s <= 1e-3 for the moderate regime of the GPU test, on the oracle's key (narrow model, one short batch)."""
    from oracle import ref_numpy
    for name in pool_cases.ATT_MODELS:
        params, weights, dim = pool_cases.att_model(name, "moderate")
        feats = np.stack(pool_cases.features([60, 60], dim, seed=2))
        key = ref_numpy.predict(feats, weights, params, dim, node=pool_cases.key_node(params))
        H, split = int(params["att_num_heads"]), bool(params["att_split_key"])
        q = weights["tdnn/attention/query"]
        for b in range(2):
            e_s = rp.score_bar(key[b], q, pool_cases.att_scale(params, key.shape[-1]), H, split)
            assert e_s.max() <= 1e-3, (name, e_s)
