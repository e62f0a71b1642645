"""GPU: xv_att_pool_forward / xv_att_pool_backward (csrc/att_pool_grad.hip) through the raw C ABI on the batches of
tests/helpers/att_pool_cases.py: twelve utterances of 1 .. 1025 frames behind three rows that no utterance owns, H in 1, 2, 3,
5, per-head widths 1 .. 65 on both sides, all four split combinations, with and without the scale.

Every element of weights, pooled, var, gvalue, gkey and gquery within the bound derived in the header of csrc/att_pool_grad.hip
(tests/helpers/ref_att_pool.py) of the float64 rule; no element is left out; the largest error / bound is printed.  Then the
binding properties of include/xvec_hip.h: the bit-exact cases (one frame, a constant value channel, a zero query), scores near
+-200 and one frame 80 above the rest, an utterance alone / in the batch / in the reversed batch, repeat, pitch, shifted base,
larger total_rows, every fill of poison.FILLS under the outputs and the workspace, the least and the full workspace, empty
utterances, batch = 0, and every error status with the outputs' poison intact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import att_pool_cases as ac                                         # noqa: E402
import poison                                                       # noqa: E402
import ref_att_pool as ra                                           # noqa: E402
import ref_pool_grad as rpg                                         # noqa: E402

pytestmark = pytest.mark.gpu

OUT_FILL = 0x5A
OUTS = ("weights", "pooled", "var", "gvalue", "gkey", "gquery")
STD_FLOOR = np.sqrt(np.float32(1e-12))
_CASES = {}


def case_of(cfg):
    if repr(cfg) not in _CASES:
        _CASES[repr(cfg)] = ac.make(cfg)
    return _CASES[repr(cfg)]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pitch(width, pad, extra):
    return width if pad == "tight" else (width + 3) // 4 * 4 + 4 * extra


def poisoned(arr, byte=OUT_FILL):
    return bool(np.all(np.ascontiguousarray(arr).view(np.uint8) == byte))


def att_call(cfg, key, value, query, offsets, gp, pad="padded", shift=0, fill=OUT_FILL, extra_rows=0, ws="full", ws_bytes=None,
             heads=None, key_dim=None, value_dim=None, batch=None, total_rows=None, ld=None, null=None, backward=True):
    """Both calls; every operand on the pitch `pad` asks for, the padding of every input NaN, every output and the workspace
    filled bytewise with `fill` first; `shift` moves the base pointers of key, value, query, weights, gkey and gvalue by that
    many floats.  -> (rc forward, rc backward, dict of numpy outputs cut to their widths, the raw padded arrays)."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    rows, B, H, P = key.shape[0], len(offsets) - 1, cfg.H, cfg.P
    total = rows + extra_rows
    lds = dict(k=_pitch(cfg.Dk, pad, 1), v=_pitch(cfg.Dv, pad, 2), q=_pitch(cfg.dq, pad, 1), w=_pitch(H, pad, 1),
               p=_pitch(2 * P, pad, 1), var=_pitch(P, pad, 3), gp=_pitch(2 * P, pad, 2), gk=_pitch(cfg.Dk, pad, 2),
               gv=_pitch(cfg.Dv, pad, 1), gq=_pitch(cfg.dq, pad, 3))
    use = dict(lds)
    use.update(ld or {})

    def buf(r, ld_, byte, off=0):
        flat = poison.fill(torch.empty(max(r, 1) * ld_ + off, dtype=torch.float32, device="cuda"), byte)
        return flat, flat[off:off + max(r, 1) * ld_].view(max(r, 1), ld_)

    def filled(r, ld_, src, off=0):
        _, t = buf(r, ld_, 0xFF, off)                                     # NaN wherever the case writes nothing
        if src.size:
            t[:src.shape[0], :src.shape[1]] = torch.from_numpy(np.ascontiguousarray(src)).cuda()
        return t

    t = dict(k=filled(total, lds["k"], key, shift), v=filled(total, lds["v"], value, shift), q=filled(H, lds["q"], query, shift),
             gp=filled(B, lds["gp"], gp))
    flats, views = {}, {}
    for name, r, off in (("w", total, shift), ("p", B, 0), ("var", B, 0), ("gk", total, shift), ("gv", total, shift), ("gq", H, 0)):
        flats[name], views[name] = buf(r, lds[name], fill, off)
    t.update(views)
    t["o"] = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int32)).cuda()
    nb = B if batch is None else batch
    tr = total if total_rows is None else total_rows
    hh, kd, vd = (H if heads is None else heads), (cfg.Dk if key_dim is None else key_dim), (cfg.Dv if value_dim is None else value_dim)
    size = lib.xv_att_pool_workspace if ws == "full" else lib.xv_att_pool_workspace_min
    need = size(nb, tr, hh, kd, vd, int(cfg.split_k), int(cfg.split_v))
    wsb = max(int(need), 0) if ws_bytes is None else ws_bytes
    t["ws"] = poison.fill(torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda"), fill)
    if null:
        t[null] = None
    sk, sv, sc = int(cfg.split_k), int(cfg.split_v), C.c_float(cfg.scale)
    rc_f = lib.xv_att_pool_forward(0, _p(t["k"]), use["k"], kd, _p(t["v"]), use["v"], vd, _p(t["q"]), use["q"], hh, sk, sv, sc, _p(t["o"]),
                                   nb, tr, _p(t["w"]), use["w"], _p(t["p"]), use["p"], _p(t["var"]), use["var"], None)
    rc_b = 0
    if backward:
        rc_b = lib.xv_att_pool_backward(0, _p(t["gp"]), use["gp"], _p(t["k"]), use["k"], kd, _p(t["v"]), use["v"], vd, _p(t["q"]), use["q"],
                                        hh, sk, sv, sc, _p(t["o"]), nb, tr, _p(t["w"]), use["w"], _p(t["p"]), use["p"], _p(t["var"]),
                                        use["var"], _p(t["gk"]), use["gk"], _p(t["gv"]), use["gv"], _p(t["gq"]), use["gq"], _p(t["ws"]),
                                        wsb, None)
    torch.cuda.synchronize()
    names = dict(weights="w", pooled="p", var="var", gvalue="gv", gkey="gk", gquery="gq")
    raw = {k: views[v].cpu().numpy() for k, v in names.items()}
    raw["front"] = {k: flats[names[k]][:shift].cpu().numpy() for k in ("weights", "gkey", "gvalue")}
    got = dict(weights=raw["weights"][:rows, :H], pooled=raw["pooled"][:B, :2 * P], var=raw["var"][:B, :P],
               gvalue=raw["gvalue"][:rows, :cfg.Dv], gkey=raw["gkey"][:rows, :cfg.Dk], gquery=raw["gquery"][:H, :cfg.dq])
    return rc_f, rc_b, got, raw


def ok_call(*a, **k):
    from tf_kaldi_speaker_amd import _lib
    rc_f, rc_b, got, raw = att_call(*a, **k)
    _lib.check(rc_f)
    _lib.check(rc_b)
    return got, raw


def batch_call(case, **k):
    return ok_call(case["cfg"], case["key"], case["value"], case["query"], case["offsets"], case["gp"], **k)


def owned(case, got, name):
    o = case["offsets"]
    return got[name][o[0]:o[-1]]


def same_bits(case, got, base, what, gquery=True):
    for k in ("pooled", "var") + (("gquery",) if gquery else ()):
        assert got[k].tobytes() == base[k].tobytes(), (what, k)
    for k in ("weights", "gvalue", "gkey"):
        assert owned(case, got, k).tobytes() == owned(case, base, k).tobytes(), (what, k)


def untouched(raw, fill=OUT_FILL):
    return all(poisoned(raw[k], fill) for k in OUTS)


@pytest.mark.parametrize("index", range(len(ac.CASES)), ids=[repr(c) for c in ac.CASES])
def test_every_element_within_its_bound(index):
    cfg = ac.CASES[index]
    case = case_of(cfg)
    off, P = case["offsets"], cfg.P
    pad = "padded" if index % 2 else "tight"
    got, raw = batch_call(case, pad=pad, extra_rows=2, ws="min" if index % 3 == 0 else "full")
    assert all(np.all(np.isfinite(owned(case, got, k))) for k in ("weights", "gvalue", "gkey"))
    assert all(np.all(np.isfinite(got[k])) for k in ("pooled", "var", "gquery"))
    worst = ra.check_batch(cfg, case["key"], case["value"], case["query"], off, case["gp"], got)
    print("%r %s: error / bound " % (cfg, pad) + " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst
    # one frame (utterance 0): w = 1, var = 0, gkey exactly 0, and gvalue = gm where one head writes the column
    r = off[0]
    assert np.all(got["weights"][r] == 1) and np.all(got["var"][0] == 0) and np.all(got["gkey"][r] == 0)
    assert np.array_equal(got["pooled"][0, :P].reshape(cfg.H, cfg.dv), np.stack([cfg.value_head(case["value"][r:r + 1], h)[0]
                                                                               for h in range(cfg.H)]))
    if cfg.split_v or cfg.H == 1:
        assert np.array_equal(got["gvalue"][r], case["gp"][0, :P])
    if case["const"] is not None:                                        # the constant value column is floored in every head
        j = case["const"]
        cols = [j] if cfg.split_v else [h * cfg.dv + j for h in range(cfg.H)]
        assert np.all(got["var"][:, cols] <= np.float32(1e-12)) and np.all(got["pooled"][:, [P + c for c in cols]] == STD_FLOOR)
    # rows nobody owns and the padding columns keep what they held
    for k, width in (("weights", cfg.H), ("gvalue", cfg.Dv), ("gkey", cfg.Dk)):
        assert poisoned(raw[k][:ac.LEAD]) and poisoned(raw[k][off[-1]:]) and poisoned(raw[k][:, width:]), k
    assert poisoned(raw["pooled"][:, 2 * P:]) and poisoned(raw["var"][:, P:]) and poisoned(raw["gquery"][:, cfg.dq:])


@pytest.mark.parametrize("cfg", [ra.Cfg(1, 5, 65, 0, 0, 1), ra.Cfg(3, 4, 5, 1, 0, 0), ra.Cfg(2, 65, 3, 0, 1, 1)], ids=repr)
def test_a_zero_query_is_statistics_pooling(cfg):
    case = dict(case_of(cfg))
    case["query"] = np.zeros_like(case["query"])
    got, _ = batch_call(case)
    off = case["offsets"]
    worst = 0.0
    for u, n in enumerate(ac.LENGTHS):
        assert np.all(got["weights"][off[u]:off[u + 1]] == np.float32(1.0 / n)), n          # exp(0) / n, rounded once
        for h in range(cfg.H):
            x = cfg.value_head(case["value"][off[u]:off[u + 1]], h)
            pc = cfg.pcols(h)
            rm, rv, rs = rpg.forward_ratios(x, got["pooled"][u, :cfg.P][pc], got["var"][u, pc], got["pooled"][u, cfg.P:][pc])
            worst = max(worst, float(np.max(rm)), float(np.max(rv)), float(np.max(rs)))
    print("%r zero query: error / bar of the plain statistics pooling %.3f" % (cfg, worst))
    assert worst <= 1.0
    assert np.all(owned(case, got, "gkey") == 0)                          # q = 0: no gradient reaches the key


@pytest.mark.parametrize("cfg", [ra.Cfg(1, 64, 5, 0, 0, 0), ra.Cfg(2, 65, 4, 1, 1, 0)], ids=repr)
def test_large_scores_and_one_dominant_frame(cfg):
    """Scores near +-200 before the max is subtracted (exp(200) overflows float32 and exp(-200) underflows it: without the
    subtraction the weights are NaN or 0 / 0), then one frame 80 above the rest (the other weights underflow towards 0)."""
    case = dict(case_of(cfg))
    off = case["offsets"]
    rows = case["key"].shape[0]
    q = case["query"].astype(np.float64)
    key = case["key"].copy()
    unit = q / (q * q).sum(axis=1, keepdims=True)                           # key = a unit gives the score a (per head)
    sign = np.where(np.arange(rows) % 2 == 0, 200.0, -200.0)
    for h in range(cfg.H):
        ks = slice(h * cfg.dq, (h + 1) * cfg.dq) if cfg.split_k else slice(0, cfg.dq)
        if cfg.split_k or h == 0:
            key[:, ks] = (key[:, ks] * 0.01 + sign[:, None] * unit[h][None, :]).astype(np.float32)
    key[:ac.LEAD] = np.nan
    case["key"] = key
    got, _ = batch_call(case)
    s = ra.scores(cfg, key[off[0]:], case["query"])
    assert np.max(s[:, 0]) > 150 and np.min(s[:, 0]) < -150
    assert all(np.all(np.isfinite(owned(case, got, k))) for k in ("weights", "gvalue", "gkey")) and np.all(np.isfinite(got["pooled"]))
    worst = ra.check_batch(cfg, key, case["value"], case["query"], off, case["gp"], got)
    print("%r scores near +-200: error / bound " % cfg + " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst
    # one frame 80 above the rest, in every utterance
    key = (case_of(cfg)["key"] * 0.01).astype(np.float32)
    for u in range(len(ac.LENGTHS)):
        for h in range(cfg.H):
            ks = slice(h * cfg.dq, (h + 1) * cfg.dq) if cfg.split_k else slice(0, cfg.dq)
            if cfg.split_k or h == 0:
                key[off[u], ks] += (80.0 * unit[h]).astype(np.float32)
    case["key"] = key
    got, _ = batch_call(case)
    assert not any(np.any(np.isnan(owned(case, got, k))) for k in ("weights", "gvalue", "gkey"))
    assert not np.any(np.isnan(got["pooled"])) and not np.any(np.isnan(got["gquery"]))
    assert np.all(got["weights"][off[:-1], 0] > 0.99)
    worst = ra.check_batch(cfg, key, case["value"], case["query"], off, case["gp"], got)
    print("%r one frame 80 above: error / bound " % cfg + " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("cfg", [ra.Cfg(2, 5, 64, 0, 0, 1), ra.Cfg(3, 64, 5, 1, 1, 0), ra.Cfg(5, 3, 4, 1, 0, 1)], ids=repr)
def test_an_utterance_does_not_depend_on_its_batch(cfg):
    case = case_of(cfg)
    off = case["offsets"]
    base, _ = batch_call(case)
    order = list(range(len(ac.LENGTHS)))[::-1]                           # the batch in reversed order, packed from row 0
    sel = np.concatenate([np.arange(off[u], off[u + 1]) for u in order])
    offr = np.concatenate([[0], np.cumsum([ac.LENGTHS[u] for u in order])]).astype(np.int32)
    rev, _ = ok_call(cfg, case["key"][sel], case["value"][sel], case["query"], offr, case["gp"][order])
    for k, u in enumerate(order):
        assert rev["pooled"][k].tobytes() == base["pooled"][u].tobytes() and rev["var"][k].tobytes() == base["var"][u].tobytes(), u
        for name in ("weights", "gvalue", "gkey"):
            assert rev[name][offr[k]:offr[k + 1]].tobytes() == base[name][off[u]:off[u + 1]].tobytes(), (name, u)
    # gquery sums the utterances in their order: the reversed batch agrees within the bound, not to the bit
    assert np.allclose(rev["gquery"], base["gquery"], rtol=1e-5, atol=1e-6 * np.max(np.abs(base["gquery"])))
    for u in (0, 3, 4, 8, 11):                                             # alone, at row 0
        sl = ac.rows_of(case, u)
        alone, _ = ok_call(cfg, case["key"][sl], case["value"][sl], case["query"], np.array([0, ac.LENGTHS[u]], dtype=np.int32),
                           case["gp"][u:u + 1])
        assert alone["pooled"][0].tobytes() == base["pooled"][u].tobytes() and alone["var"][0].tobytes() == base["var"][u].tobytes(), u
        for name in ("weights", "gvalue", "gkey"):
            assert alone[name].tobytes() == base[name][sl].tobytes(), (name, u)


@pytest.mark.parametrize("cfg", [ra.Cfg(1, 4, 65, 0, 0, 1), ra.Cfg(2, 64, 4, 1, 0, 0), ra.Cfg(3, 5, 63, 0, 1, 1)], ids=repr)
def test_bits_do_not_depend_on_repeat_layout_total_rows_workspace_or_poison(cfg):
    case = case_of(cfg)
    off = case["offsets"]
    base, _ = batch_call(case)
    same_bits(case, batch_call(case)[0], base, "repeat")
    same_bits(case, batch_call(case, pad="tight")[0], base, "pitch = width")
    same_bits(case, batch_call(case, extra_rows=200)[0], base, "a larger total_rows")
    same_bits(case, batch_call(case, ws="min")[0], base, "the least workspace")
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    sizes = [f(12, case["key"].shape[0], cfg.H, cfg.Dk, cfg.Dv, int(cfg.split_k), int(cfg.split_v))
             for f in (lib.xv_att_pool_workspace_min, lib.xv_att_pool_workspace)]
    assert 0 < sizes[0] < sizes[1]
    same_bits(case, batch_call(case, ws_bytes=(sizes[0] + sizes[1]) // 2)[0], base, "a workspace between the least and the full")
    same_bits(case, batch_call(case, ws_bytes=2 * sizes[1])[0], base, "a workspace beyond the full")
    for pad in ("tight", "padded"):
        got, raw = batch_call(case, pad=pad, shift=1)                  # a base off by one float: 4-byte accesses, the same bits
        same_bits(case, got, base, "base pointer off by one float, %s" % pad)
        assert all(poisoned(v) for v in raw["front"].values())         # the float in front of each shifted buffer
    for fill in poison.FILLS:
        for ws in ("min", "full"):
            got, raw = batch_call(case, fill=fill, extra_rows=1, ws=ws)
            same_bits(case, got, base, "fill %#x, %s workspace" % (fill, ws))
            for k, width in (("weights", cfg.H), ("gvalue", cfg.Dv), ("gkey", cfg.Dk)):
                assert poisoned(raw[k][:ac.LEAD], fill) and poisoned(raw[k][off[-1]:], fill) and poisoned(raw[k][:, width:], fill), k


def test_empty_utterances_and_batch_zero():
    cfg = ra.Cfg(2, 3, 5, 1, 0, 1)
    case = case_of(cfg)
    sl = ac.rows_of(case, 4)                                              # 17 frames
    key, value, q = case["key"][sl], case["value"][sl], case["query"]
    offs = np.array([0, 0, 17, 17], dtype=np.int32)
    gp = case["gp"][:3]
    got, _ = ok_call(cfg, key, value, q, offs, gp)
    alone, _ = ok_call(cfg, key, value, q, np.array([0, 17], dtype=np.int32), gp[1:2])
    assert got["pooled"][1].tobytes() == alone["pooled"][0].tobytes()
    assert all(got[k].tobytes() == alone[k].tobytes() for k in ("weights", "gvalue", "gkey", "gquery"))
    for u in (0, 2):                                                      # n = 0: m = 0, var = 0, std = sqrtf(1e-12f)
        assert np.all(got["pooled"][u, :cfg.P] == 0) and np.all(got["var"][u] == 0) and np.all(got["pooled"][u, cfg.P:] == STD_FLOOR)
    empty = np.zeros(4, dtype=np.int32)                                   # a batch without a frame: gquery is a clean zero
    got, raw = ok_call(cfg, key, value, q, empty, gp)
    assert np.all(got["gquery"] == 0) and all(poisoned(raw[k]) for k in ("weights", "gvalue", "gkey"))
    rc_f, rc_b, _, raw = att_call(cfg, key, value, q, offs, gp, batch=0)
    assert rc_f == 0 and rc_b == 0 and untouched(raw)
    rc_f, rc_b, _, raw = att_call(cfg, key, value, q, offs, gp, batch=0, null="k")      # batch = 0 touches nothing, pointers included
    assert rc_f == 0 and rc_b == 0 and untouched(raw)


def test_error_statuses_and_limits():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    cfg = ra.Cfg(2, 3, 5, 1, 0, 1)
    case = case_of(cfg)
    sl = ac.rows_of(case, 4)
    key, value, q = case["key"][sl], case["value"][sl], case["query"]
    offs = np.array([0, 17], dtype=np.int32)
    gp = case["gp"][:1]

    def call(**k):
        return att_call(cfg, key, value, q, offs, gp, **k)

    for bad in (dict(heads=0), dict(heads=17), dict(key_dim=0), dict(key_dim=4097), dict(value_dim=0), dict(value_dim=4097),
                dict(total_rows=(1 << 24) + 1), dict(batch=(1 << 20) + 1)):
        rc_f, rc_b, _, raw = call(**bad)
        assert rc_f == _lib.XV_ERR_UNSUPPORTED and rc_b == _lib.XV_ERR_UNSUPPORTED and untouched(raw), bad
    for bad in (dict(batch=-1), dict(total_rows=-1), dict(key_dim=7), dict(ld=dict(k=5)), dict(ld=dict(v=4)), dict(ld=dict(q=2)),
                dict(ld=dict(w=1)), dict(ld=dict(p=19)), dict(ld=dict(var=9)), dict(null="k"), dict(null="v"), dict(null="q"),
                dict(null="o"), dict(null="w"), dict(null="p"), dict(null="var")):
        rc_f, rc_b, _, raw = call(**bad)
        assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and untouched(raw), bad
    split_v = ra.Cfg(2, 3, 5, 1, 1, 1)                                    # value_dim = 5 on a split value: 2 does not divide it
    rc_f, rc_b, _, raw = att_call(split_v, key, np.zeros((17, 10), dtype=np.float32), q, offs, np.zeros((1, 20), dtype=np.float32),
                                  value_dim=5)
    assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and untouched(raw)
    for bad in (dict(ld=dict(gp=19)), dict(ld=dict(gk=5)), dict(ld=dict(gv=4)), dict(ld=dict(gq=2)), dict(null="gp"), dict(null="gk"),
                dict(null="gv"), dict(null="gq")):                       # the backward's own operands
        rc_f, rc_b, _, raw = call(**bad)
        assert rc_f == 0 and rc_b == _lib.XV_ERR_INVALID and all(poisoned(raw[k]) for k in ("gvalue", "gkey", "gquery")), bad
    least = lib.xv_att_pool_workspace_min(1, 17, 2, 6, 5, 1, 0)
    for bad in (dict(ws_bytes=least - 1), dict(null="ws")):
        rc_f, rc_b, _, raw = call(**bad)
        assert rc_f == 0 and rc_b == _lib.XV_ERR_WORKSPACE and all(poisoned(raw[k]) for k in ("gvalue", "gkey", "gquery")), bad
    assert lib.xv_att_pool_workspace(0, 0, 2, 6, 5, 1, 0) == 0 and lib.xv_att_pool_workspace(1, 17, 17, 6, 5, 1, 0) == _lib.XV_ERR_UNSUPPORTED
    # the limits the header promises are legal sizes.  total_rows = 2^24 sizes grids and the workspace: rows past offsets[batch]
    # are never touched, so the buffers stay as small as the utterance, and the bits are those of the tight bound
    base, _ = ok_call(cfg, key, value, q, offs, gp)
    got, raw = ok_call(cfg, key, value, q, offs, gp, total_rows=1 << 24)
    assert all(got[k].tobytes() == base[k].tobytes() for k in OUTS) and poisoned(raw["gvalue"][:, 5:])
    # 16 heads on 4096 columns each side, one short utterance
    wide = ra.Cfg(16, 256, 4096, 1, 0, 1)
    r = np.random.RandomState(5)
    k3, v3 = r.standard_normal((3, 4096)).astype(np.float32), r.standard_normal((3, 4096)).astype(np.float32)
    q3 = (0.2 * r.standard_normal((16, 256))).astype(np.float32)
    gp3 = r.standard_normal((1, 2 * wide.P)).astype(np.float32)
    o3 = np.array([0, 3], dtype=np.int32)
    got, _ = ok_call(wide, k3, v3, q3, o3, gp3, pad="tight")
    worst = ra.check_batch(wide, k3, v3, q3, o3, gp3, got)
    print("16 heads, 4096 columns: error / bound " + " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst
