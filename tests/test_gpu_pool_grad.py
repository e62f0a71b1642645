"""GPU: xv_stat_pool_forward / xv_stat_pool_backward (csrc/pool_grad.hip) through the raw C ABI on the batch of
tests/helpers/pool_grad_cases.py: twelve utterances of 1 .. 1025 frames behind three rows that no utterance owns.

Forward: every mean, variance and std within the bars of tests/helpers/ref_pool.py (k = 16) of the float64 pooling of the same
rows.  Backward: every element within the bound derived in the header of csrc/pool_grad.hip of the float64 rule at the float32
m, std, v the forward wrote.  No element is left out.  Then the binding properties of include/xvec_hip.h: the floored channel
gives gx = a exactly; an utterance gets the same bits alone, in the batch and in the reversed batch; the same bits on repeat, for
a larger total_rows, for every pitch and for a base pointer that rules the 16-byte accesses out; rows nobody owns and padding
columns keep their poison, and NaN in the padding of x reaches nothing.  Every test prints the largest error / bound first."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import poison                                                       # noqa: E402
import pool_grad_cases as pc                                        # noqa: E402
import ref_pool_grad as rpg                                         # noqa: E402

pytestmark = pytest.mark.gpu

OUT_FILL = 0x5A
_CASES = {}


def case_of(C_):
    if C_ not in _CASES:
        _CASES[C_] = pc.make(C_)
    return _CASES[C_]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pitch(width, pad, extra):
    return width if pad == "tight" else (width + 3) // 4 * 4 + 4 * extra


def poisoned(arr, byte=OUT_FILL):
    return bool(np.all(np.ascontiguousarray(arr).view(np.uint8) == byte))


def pool_call(x, offsets, gp, pad="padded", shift=0, fill=OUT_FILL, extra_rows=0, channels=None, batch=None, total_rows=None,
              ld=None, null=None):
    """Both calls on x [rows, C] (rows the offsets do not own are handed over as they are), every operand on the pitch `pad`
    asks for, x's padding columns NaN, every output filled bytewise with `fill` first; `shift` moves the base pointers of x and
    gx by that many floats.  -> (rc forward, rc backward, dict of numpy outputs cut to their widths, the raw padded arrays)."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    rows, C_ = x.shape
    B = len(offsets) - 1
    total = rows + extra_rows
    lds = dict(x=_pitch(C_, pad, 1), gx=_pitch(C_, pad, 2), p=_pitch(2 * C_, pad, 1), v=_pitch(C_, pad, 3), gp=_pitch(2 * C_, pad, 2))
    use = dict(lds)                                                       # the pitches handed to the library (`ld`: a wrong one)
    use.update(ld or {})

    def buf(r, ld_, byte, off=0):
        flat = poison.fill(torch.empty(max(r, 1) * ld_ + off, dtype=torch.float32, device="cuda"), byte)
        return flat, flat[off:off + max(r, 1) * ld_].view(max(r, 1), ld_)

    _, xd = buf(total, lds["x"], 0xFF, shift)                             # NaN wherever the case writes nothing
    xd[:rows, :C_] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    _, gpd = buf(B, lds["gp"], 0xFF)
    if B:
        gpd[:B, :2 * C_] = torch.from_numpy(np.ascontiguousarray(gp)).cuda()
    gx_flat, gxd = buf(total, lds["gx"], fill, shift)
    _, pd = buf(B, lds["p"], fill)
    _, vd = buf(B, lds["v"], fill)
    od = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int32)).cuda()
    ch = C_ if channels is None else channels
    nb = B if batch is None else batch
    tr = total if total_rows is None else total_rows
    ptr = dict(x=xd, gp=gpd, gx=gxd, p=pd, v=vd, o=od)
    if null:
        ptr[null] = None
    rc_f = lib.xv_stat_pool_forward(0, _p(ptr["x"]), use["x"], ch, _p(ptr["o"]), nb, tr, _p(ptr["p"]), use["p"], _p(ptr["v"]), use["v"], None)
    rc_b = lib.xv_stat_pool_backward(0, _p(ptr["gp"]), use["gp"], _p(ptr["x"]), use["x"], ch, _p(ptr["o"]), nb, tr, _p(ptr["p"]), use["p"],
                                     _p(ptr["v"]), use["v"], _p(ptr["gx"]), use["gx"], None)
    torch.cuda.synchronize()
    raw = dict(pooled=pd.cpu().numpy(), var=vd.cpu().numpy(), gx=gxd.cpu().numpy(), gx_flat=gx_flat.cpu().numpy())
    got = dict(pooled=raw["pooled"][:B, :2 * C_], var=raw["var"][:B, :C_], gx=raw["gx"][:rows, :C_])
    return rc_f, rc_b, got, raw


def ok_call(*a, **k):
    from tf_kaldi_speaker_amd import _lib
    rc_f, rc_b, got, raw = pool_call(*a, **k)
    _lib.check(rc_f)
    _lib.check(rc_b)
    return got, raw


def batch_call(case, **k):
    return ok_call(case["x"], case["offsets"], case["gp"], **k)


@pytest.mark.parametrize("pad", ["tight", "padded"])
@pytest.mark.parametrize("C_", pc.CHANNELS)
def test_every_element_within_the_bars_and_the_bound(C_, pad):
    case = case_of(C_)
    off = case["offsets"]
    got, raw = batch_call(case, pad=pad, extra_rows=2)
    assert np.all(np.isfinite(got["pooled"])) and np.all(np.isfinite(got["var"])) and np.all(np.isfinite(got["gx"][pc.LEAD:]))
    worst = dict(mean=0.0, var=0.0, std=0.0, gx=0.0)
    for u, n in enumerate(pc.LENGTHS):
        x = pc.utterance(case, u)
        mean, std, var = got["pooled"][u, :C_], got["pooled"][u, C_:], got["var"][u]
        rm, rv, rsd = rpg.forward_ratios(x, mean, var, std)
        gx = got["gx"][off[u]:off[u + 1]]
        ref = rpg.backward(x, mean, std, var, case["gp"][u])
        rgx = np.abs(gx.astype(np.float64) - ref) / rpg.backward_bound(x, mean, std, var, case["gp"][u])
        for k, rat in (("mean", rm), ("var", rv), ("std", rsd), ("gx", rgx)):
            worst[k] = max(worst[k], float(np.max(rat)))
        if case["const"] is not None:                                     # the floored channel: gx = a bit for bit
            j = case["const"]
            assert var[j] == 0 and std[j] == np.sqrt(np.float32(1e-12)) and mean[j] == pc.CONST_VALUE
            assert np.all(gx[:, j] == np.float32(case["gp"][u, j]) / np.float32(n))
        if n == 1:
            assert np.all(var == 0) and np.array_equal(gx[0], case["gp"][u, :C_])
    print("C = %d %s: error / bar " % (C_, pad) + " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst
    # rows nobody owns and the padding columns keep what they held
    assert poisoned(raw["gx"][:pc.LEAD]) and poisoned(raw["gx"][off[-1]:])
    assert poisoned(raw["gx"][:, C_:]) and poisoned(raw["pooled"][:, 2 * C_:]) and poisoned(raw["var"][:, C_:])


@pytest.mark.parametrize("C_", [5, 64])
def test_an_utterance_does_not_depend_on_its_batch(C_):
    case = case_of(C_)
    off = case["offsets"]
    base, _ = batch_call(case)
    # the batch in reversed order, packed from row 0
    order = list(range(len(pc.LENGTHS)))[::-1]
    xr = np.concatenate([pc.utterance(case, u) for u in order])
    offr = np.concatenate([[0], np.cumsum([pc.LENGTHS[u] for u in order])]).astype(np.int32)
    rev, _ = ok_call(xr, offr, case["gp"][order])
    for k, u in enumerate(order):
        assert rev["pooled"][k].tobytes() == base["pooled"][u].tobytes() and rev["var"][k].tobytes() == base["var"][u].tobytes(), u
        assert rev["gx"][offr[k]:offr[k + 1]].tobytes() == base["gx"][off[u]:off[u + 1]].tobytes(), u
    for u, n in enumerate(pc.LENGTHS):                                   # alone, at row 0
        alone, _ = ok_call(pc.utterance(case, u), np.array([0, n], dtype=np.int32), case["gp"][u:u + 1])
        assert alone["pooled"][0].tobytes() == base["pooled"][u].tobytes() and alone["var"][0].tobytes() == base["var"][u].tobytes(), u
        assert alone["gx"].tobytes() == base["gx"][off[u]:off[u + 1]].tobytes(), u


@pytest.mark.parametrize("C_", [4, 65, 64])
def test_bits_do_not_depend_on_repeat_layout_total_rows_or_poison(C_):
    case = case_of(C_)
    off = case["offsets"]
    base, _ = batch_call(case)

    def same(got, what):
        assert got["pooled"].tobytes() == base["pooled"].tobytes() and got["var"].tobytes() == base["var"].tobytes(), what
        assert got["gx"][off[0]:off[-1]].tobytes() == base["gx"][off[0]:off[-1]].tobytes(), what

    same(batch_call(case)[0], "repeat")
    same(batch_call(case, pad="tight")[0], "pitch = width")
    same(batch_call(case, extra_rows=200)[0], "a larger total_rows")
    for pad in ("tight", "padded"):
        got, raw = batch_call(case, pad=pad, shift=1)                  # the 16-byte accesses must decline: 4-byte ones, same bits
        same(got, "base pointer off by one float, %s" % pad)
        assert poisoned(raw["gx_flat"][:1])                            # the float in front of the shifted buffer
    for fill in poison.FILLS:
        got, raw = batch_call(case, fill=fill, extra_rows=1)
        same(got, "fill %#x" % fill)
        assert poisoned(raw["gx"][:pc.LEAD], fill) and poisoned(raw["gx"][off[-1]:], fill) and poisoned(raw["gx"][:, C_:], fill)


def test_empty_utterances_and_batch_zero():
    case = case_of(5)
    x = pc.utterance(case, 4)                                             # 17 frames
    offs = np.array([0, 0, 17, 17], dtype=np.int32)
    gp = case["gp"][:3]
    got, _ = ok_call(x, offs, gp)
    alone, _ = ok_call(x, np.array([0, 17], dtype=np.int32), gp[1:2])
    assert got["pooled"][1].tobytes() == alone["pooled"][0].tobytes() and got["gx"].tobytes() == alone["gx"].tobytes()
    for u in (0, 2):                                                      # n = 0: m = 0, v = 0, std = sqrtf(1e-12f)
        assert np.all(got["pooled"][u, :5] == 0) and np.all(got["var"][u] == 0) and np.all(got["pooled"][u, 5:] == np.sqrt(np.float32(1e-12)))
    rc_f, rc_b, _, raw = pool_call(x, offs, gp, batch=0)
    assert rc_f == 0 and rc_b == 0 and all(poisoned(raw[k]) for k in ("pooled", "var", "gx"))
    rc_f, rc_b, _, raw = pool_call(x, offs, gp, batch=0, null="x")       # batch = 0 touches nothing, pointers included
    assert rc_f == 0 and rc_b == 0


def test_error_statuses_and_limits():
    from tf_kaldi_speaker_amd import _lib
    case = case_of(5)
    x = pc.utterance(case, 4)
    offs = np.array([0, 17], dtype=np.int32)
    gp = case["gp"][:1]

    def untouched(raw):
        return all(poisoned(raw[k]) for k in ("pooled", "var", "gx"))

    for bad in (dict(channels=0), dict(channels=4097), dict(total_rows=(1 << 24) + 1)):
        rc_f, rc_b, _, raw = pool_call(x, offs, gp, **bad)
        assert rc_f == _lib.XV_ERR_UNSUPPORTED and rc_b == _lib.XV_ERR_UNSUPPORTED and untouched(raw), bad
    for bad in (dict(batch=-1), dict(ld=dict(x=4)), dict(ld=dict(p=9)), dict(ld=dict(v=4)), dict(null="x"), dict(null="o"),
                dict(null="p"), dict(null="v")):
        rc_f, rc_b, _, raw = pool_call(x, offs, gp, **bad)
        assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and untouched(raw), bad
    for bad in (dict(ld=dict(gp=9)), dict(ld=dict(gx=4)), dict(null="gp"), dict(null="gx")):       # the backward's own operands
        rc_f, rc_b, _, raw = pool_call(x, offs, gp, **bad)
        assert rc_f == 0 and rc_b == _lib.XV_ERR_INVALID and poisoned(raw["gx"]), bad
    # the limits the header promises are legal sizes.  total_rows = 2^24 only sizes the backward's grid: rows past offsets[batch]
    # are never touched, so the buffers stay as small as the utterance, and the bits are those of the tight bound
    base, _ = ok_call(x, offs, gp)
    got, raw = ok_call(x, offs, gp, total_rows=1 << 24)
    assert all(got[k].tobytes() == base[k].tobytes() for k in ("pooled", "var", "gx")) and poisoned(raw["gx"][:, 5:])
    # 4096 channels, one short utterance
    r = np.random.RandomState(5)
    wide = r.standard_normal((3, 4096)).astype(np.float32)
    got, _ = ok_call(wide, np.array([0, 3], dtype=np.int32), r.standard_normal((1, 8192)).astype(np.float32), pad="tight")
    rm, rv, rsd = rpg.forward_ratios(wide, got["pooled"][0, :4096], got["var"][0], got["pooled"][0, 4096:])
    assert max(np.max(rm), np.max(rv), np.max(rsd)) <= 1.0
