"""GPU: xv_tconv_forward / xv_tconv_backward (csrc/tconv_grad.hip) through the raw C ABI against the float64 oracle
tests/helpers/ref_tconv.py, on the float32 inputs the kernels saw.

Every element of z, y, gx, gw, gbias, ggamma and gbeta must lie within ref_tconv.bounds (the bound derived in the header of
csrc/tconv_grad.hip); no element is left out (tests/helpers/tconv_cases.py keeps every h off the ReLU's discontinuity, checked
on the CPU in tests/test_tconv_host.py).  As a coarse cap that keeps the bound honest the relative L2 error of every output
stays within 1e-4, the project's parity requirement.  Every test prints the largest error / bound before it asserts.  The
binding properties of include/xvec_hip.h: bit-equal repeats, bit-equal for every legal ws_bytes, poison, an utterance alone.

The packed input lies between rows of NaN that no utterance owns (offsets[0] = 3): a read outside the owned rows shows in the
outputs.  Layout "odd" puts every operand on a pitch beyond its width and 4 bytes off a 16-byte boundary."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import poison                                                       # noqa: E402
import ref_tconv as rt                                              # noqa: E402
import tconv_cases as tc                                            # noqa: E402

pytestmark = pytest.mark.gpu

OUT_FILL = 0x5A
LEAD, TRAIL = 3, 2
OUTPUTS = ("z", "y", "gx", "gw", "gbias", "ggamma", "gbeta")
_CASES = {}


def case_of(name):
    """The inputs and the oracle of a case, computed once and never changed."""
    if name not in _CASES:
        c = tc.make(name)
        fwd = rt.forward(c["x"], c["offsets"], c["taps"], c["w"], c["b"], c["bn"], c["act"])
        bwd = rt.backward(fwd, c["gy"])
        _CASES[name] = (c, fwd, bwd, rt.bounds(fwd, bwd))
    return _CASES[name]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def tconv_call(c, ws_bytes=None, fill=OUT_FILL, want_gx=True, drop_bn=None, taps=None, channels=None, out_dim=None, extra_total=0,
               ldx_short=False, ws_offset=0):
    """xv_tconv_forward then xv_tconv_backward on the case's float32 arrays, every output and the workspace filled bytewise with
    `fill` first -> (rc forward, rc backward, dict of numpy outputs, raw padded arrays)."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    x, gy, w = c["x"], c["gy"], c["w"]
    W = c["taps"]
    rows, Cc = x.shape
    N, K = w.shape
    odd = c["layout"] == "odd"
    shift = 1 if odd else 0                                          # floats between the 16-byte aligned allocation and the base
    ldx = Cc + 3 if odd else Cc
    ldw = K + 5 if odd else (K + 3) // 4 * 4
    ldz, ldy, ldgy, ldgx = (N + 1, N + 2, N + 3, Cc + 1) if odd else (N, N + 4, N, Cc)
    offsets = np.asarray(c["offsets"], dtype=np.int64) + LEAD
    batch = offsets.size - 1
    total_in = int(offsets[-1] - offsets[0]) + extra_total
    total_out = int(rt.out_offsets(offsets, W)[-1]) + extra_total
    all_rows = rows + LEAD + TRAIL

    def padded(a, ld, n_rows, lead=0, background=0.0):
        buf = torch.full((n_rows * ld + shift + 4,), background, dtype=torch.float32, device="cuda")
        t = buf[shift:shift + n_rows * ld].view(n_rows, ld)
        if a.shape[0]:
            t[lead:lead + a.shape[0], :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        return t

    def vec(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def out(r, ld):
        buf = poison.fill(torch.empty((max(r, 1) * ld + shift + 4,), dtype=torch.float32, device="cuda"), fill)
        return buf, buf[shift:shift + max(r, 1) * ld].view(max(r, 1), ld)

    xd = padded(x, ldx, all_rows, LEAD, float("nan"))
    wd, gyd = padded(w, ldw, N), padded(gy, ldgy, max(total_out, 1))
    bd = vec(c["b"])
    bn = [None] * 4 if c["bn"] is None else [vec(v) for v in c["bn"]]
    if drop_bn is not None:
        bn[drop_bn] = None
    offd = torch.from_numpy(offsets.astype(np.int32)).cuda()
    (zb, z), (yb, y), (gwb, gw) = out(total_out, ldz), out(total_out, ldy), out(N, ldw)
    gxb, gx = out(all_rows, ldgx) if want_gx else (None, None)
    gb, gg, gbe = (poison.fill(torch.empty((N,), dtype=torch.float32, device="cuda"), fill) for _ in range(3))
    W_, C_, N_ = W if taps is None else taps, Cc if channels is None else channels, N if out_dim is None else out_dim
    need = int(lib.xv_tconv_workspace(batch, total_in, total_out, W, Cc, N))
    given = need if ws_bytes is None else ws_bytes
    wsb = poison.fill(torch.empty(max(given, 16) + 32, dtype=torch.uint8, device="cuda"), fill)
    ws = wsb[ws_offset:]
    rc_f = lib.xv_tconv_forward(0, _p(xd), ldx if not ldx_short else Cc - 1, C_, W_, _p(offd), batch, total_in, total_out, _p(wd), ldw,
                                N_, _p(bd), _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]), c["act"], _p(z), ldz, _p(y), ldy, _p(ws), given,
                                None)
    poison.fill(wsb, fill)                                           # the backward call builds its own maps
    rc_b = lib.xv_tconv_backward(0, _p(gyd), ldgy, _p(xd), ldx if not ldx_short else Cc - 1, C_, W_, _p(offd), batch, total_in,
                                 total_out, _p(z), ldz, _p(wd), ldw, N_, _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]), c["act"], _p(gx),
                                 ldgx, _p(gw), _p(gb), _p(gg), _p(gbe), _p(ws), given, None)
    torch.cuda.synchronize()
    raw = dict(z=zb.cpu().numpy(), y=yb.cpu().numpy(), gx=None if gxb is None else gxb.cpu().numpy(), gw=gwb.cpu().numpy(),
               gbias=gb.cpu().numpy(), ggamma=gg.cpu().numpy(), gbeta=gbe.cpu().numpy())
    view = dict(z=z.cpu().numpy(), y=y.cpu().numpy(), gx=None if gx is None else gx.cpu().numpy(), gw=gw.cpu().numpy())
    n_out = total_out - extra_total
    got = dict(z=view["z"][:n_out, :N], y=view["y"][:n_out, :N], gx=None if gx is None else view["gx"][LEAD:LEAD + rows, :Cc],
               gw=view["gw"][:, :K], gbias=raw["gbias"], ggamma=raw["ggamma"], gbeta=raw["gbeta"])
    # what the call must leave alone: beyond the widths, beyond the last output row, the rows of gx no utterance owns
    rest = [view["z"][:, N:], view["y"][:, N:], view["gw"][:, K:], view["z"][n_out:], view["y"][n_out:]]
    if gx is not None:
        rest += [view["gx"][:, Cc:], view["gx"][:LEAD], view["gx"][LEAD + rows:]]
    untouched = all(poisoned(v, fill) for v in rest)
    return rc_f, rc_b, got, raw, untouched


def ok_call(c, **k):
    from tf_kaldi_speaker_amd import _lib
    rc_f, rc_b, got, raw, untouched = tconv_call(c, **k)
    _lib.check(rc_f)
    _lib.check(rc_b)
    assert untouched, "something beyond the outputs was written"
    return got


def same_bits(a, b, what, names=OUTPUTS):
    for k in names:
        if a[k] is None or b[k] is None:
            continue
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def poisoned(arr, byte=OUT_FILL):
    return bool(np.all(np.ascontiguousarray(arr).view(np.uint8) == byte))


def names_of(c):
    # without batch norm ggamma and gbeta are no outputs of the call: they keep whatever they held
    return OUTPUTS if c["bn"] is not None else tuple(k for k in OUTPUTS if k not in ("ggamma", "gbeta"))


@pytest.mark.parametrize("name", [c[0] for c in tc.CASES])
def test_every_element_within_the_bound(name):
    c, fwd, bwd, bnd = case_of(name)
    tc.precondition(c, fwd)
    got = ok_call(c)
    ref = dict(z=fwd["z"], y=fwd["y"], gx=bwd["gx"], gw=bwd["gw"], gbias=bwd["gbias"], ggamma=bwd["ggamma"], gbeta=bwd["gbeta"])
    worst, l2 = {}, {}
    for k in OUTPUTS:
        if ref[k] is None:
            assert poisoned(got[k]), "%s is not an output without batch norm" % k
            continue
        assert np.all(np.isfinite(got[k])), k
        err = np.abs(got[k].astype(np.float64) - ref[k])
        assert np.all(err[bnd[k] == 0] == 0), k
        worst[k] = float(np.max(err / (bnd[k] + 1e-300))) if np.any(err > 0) else 0.0
        norm = np.linalg.norm(ref[k])
        l2[k] = float(np.linalg.norm(err) / norm) if norm > 0 else float(np.linalg.norm(err))
    print("%s: W=%d C=%d N=%d rows=%d bn=%s act=%d  error/bound %s  rel-L2 %s"
          % (name, c["taps"], c["x"].shape[1], c["w"].shape[0], fwd["z"].shape[0], c["bn"] is not None, c["act"],
             " ".join("%s %.3f" % kv for kv in sorted(worst.items())), " ".join("%s %.2e" % kv for kv in sorted(l2.items()))))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert all(v <= 1e-4 for v in l2.values()), l2


@pytest.mark.parametrize("name", ["w5_c30", "w7_c68", "w9_c8", "w5_long"])
def test_bits_do_not_depend_on_repeat_workspace_or_poison(name):
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    c = case_of(name)[0]
    names = names_of(c)
    base = ok_call(c)
    same_bits(base, ok_call(c), "repeat", names)
    batch = c["offsets"].size - 1
    total_in, total_out = int(c["offsets"][-1]), int(rt.out_offsets(c["offsets"], c["taps"])[-1])
    dims = (batch, total_in, total_out, c["taps"], c["x"].shape[1], c["w"].shape[0])
    least, full = int(lib.xv_tconv_workspace_min(*dims)), int(lib.xv_tconv_workspace(*dims))
    assert 0 < least <= full
    for ws in (least, full, full + 16, full + 4096 + 48):
        same_bits(base, ok_call(c, ws_bytes=ws), "ws_bytes %d" % ws, names)
    same_bits(base, ok_call(c, ws_offset=16), "workspace 16 bytes further", names)
    for fill in poison.FILLS:
        got = ok_call(c, ws_bytes=least, fill=fill)
        same_bits(base, got, "fill %#x" % fill, names)
        assert c["bn"] is not None or (poisoned(got["ggamma"], fill) and poisoned(got["gbeta"], fill))
    # host bounds beyond the true totals size grids only
    same_bits(base, ok_call(c, extra_total=70), "total_in and total_out 70 rows beyond", ("z", "y", "gx", "gbias", "ggamma", "gbeta")
              if c["bn"] is not None else ("z", "y", "gx", "gbias"))


@pytest.mark.parametrize("name", ["w5_c23", "w9_c68", "w9_c8"])
def test_an_utterance_does_not_depend_on_its_batch(name):
    c = case_of(name)[0]
    base = ok_call(c)
    off, oo = c["offsets"], rt.out_offsets(c["offsets"], c["taps"])
    for b in range(off.size - 1):
        if oo[b + 1] == oo[b]:                                         # an utterance without output rows: zero rows of gx
            assert not base["gx"][off[b]:off[b + 1]].any()             # (alone it is a call with total_out = 0: nothing touched)
            continue
        got = ok_call(tc.alone(c, b))
        for k in ("z", "y"):
            assert got[k].tobytes() == base[k][oo[b]:oo[b + 1]].tobytes(), (k, b)
        assert got["gx"].tobytes() == base["gx"][off[b]:off[b + 1]].tobytes(), ("gx", b)


def test_gx_may_be_null():
    c = case_of("w5_c68")[0]
    base = ok_call(c)
    got = ok_call(c, want_gx=False)
    same_bits(base, got, "gx = NULL", names_of(c))
    assert got["gx"] is None


def test_nothing_to_do_touches_nothing():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    c = dict(case_of("w5_c30")[0])
    empty = dict(c, x=c["x"][:0], offsets=np.zeros(1, dtype=np.int64), gy=c["gy"][:0])          # batch = 0
    rc_f, rc_b, _, raw, untouched = tconv_call(empty, ws_bytes=0)
    assert rc_f == 0 and rc_b == 0 and untouched and all(poisoned(v) for v in raw.values())
    short = dict(c, x=c["x"][:7], offsets=np.array([0, 3, 7], dtype=np.int64), gy=c["gy"][:0])   # total_out = 0
    rc_f, rc_b, _, raw, untouched = tconv_call(short, ws_bytes=0)
    assert rc_f == 0 and rc_b == 0 and untouched and all(poisoned(v) for v in raw.values())
    for f in (lib.xv_tconv_workspace, lib.xv_tconv_workspace_min):
        assert int(f(0, 0, 0, 5, 30, 8)) == 0 and int(f(2, 7, 0, 5, 30, 8)) == 0
    assert int(lib.xv_tconv_forward_workspace(0, 0)) == 0


def test_error_statuses():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    c = case_of("w5_c30")[0]
    batch = c["offsets"].size - 1
    total_in, total_out = int(c["offsets"][-1]), int(rt.out_offsets(c["offsets"], 5)[-1])
    least = int(lib.xv_tconv_workspace_min(batch, total_in, total_out, 5, 30, 8))
    rc_f, rc_b, _, raw, _ = tconv_call(c, ws_bytes=least - 16)
    assert rc_f == 0 and rc_b == _lib.XV_ERR_WORKSPACE              # the forward needs its row maps only
    assert all(poisoned(raw[k]) for k in ("gx", "gw", "gbias", "ggamma", "gbeta"))
    rc_f, rc_b, _, raw, _ = tconv_call(c, ws_bytes=int(lib.xv_tconv_forward_workspace(batch, total_out)) - 16)
    assert rc_f == _lib.XV_ERR_WORKSPACE and rc_b == _lib.XV_ERR_WORKSPACE and all(poisoned(v) for v in raw.values())
    rc_f, rc_b, _, raw, _ = tconv_call(c, ws_offset=4)
    assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and all(poisoned(v) for v in raw.values())
    for drop in range(4):                                          # some, but not all, of the four batch-norm pointers
        rc_f, rc_b, _, raw, _ = tconv_call(c, drop_bn=drop)
        assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID
        assert all(poisoned(v) for v in raw.values())
    for kw in (dict(taps=0), dict(taps=17), dict(taps=16, channels=1025), dict(out_dim=4097), dict(channels=0)):
        rc_f, rc_b, _, raw, _ = tconv_call(c, **kw)
        assert rc_f == _lib.XV_ERR_UNSUPPORTED and rc_b == _lib.XV_ERR_UNSUPPORTED and all(poisoned(v) for v in raw.values()), kw
    rc_f, rc_b, _, raw, _ = tconv_call(c, ldx_short=True)
    assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and all(poisoned(v) for v in raw.values())
    rc_f, rc_b, _, raw, _ = tconv_call(dict(c, act=3))
    assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and all(poisoned(v) for v in raw.values())
    # the limits the header promises are legal sizes
    assert int(lib.xv_tconv_workspace_min(64, 19200, 18304, 16, 1024, 4096)) > 0
    assert int(lib.xv_tconv_workspace(1 << 24, 1 << 24, 1 << 24, 1, 16384, 1)) > 0
