"""GPU: xv_gconv_forward / xv_gconv_backward and xv_add_act_* (csrc/gconv_grad.hip) through the raw C ABI against the float64
oracle tests/helpers/ref_gconv.py, on the float32 inputs the kernels saw.

Every element of z, y, gx, gw, gbias, ggamma and gbeta must lie within ref_gconv.bounds (the bound derived in the header of
csrc/gconv_grad.hip); no element is left out (tests/helpers/gconv_cases.py keeps every h off the ReLU's discontinuity, checked
on the CPU in tests/test_gconv_host.py).  As a coarse cap that keeps the bound honest the relative L2 error of every output
stays within 1e-4, the project's parity requirement.  Every test prints the largest error / bound before it asserts.  The
binding properties of include/xvec_hip.h: bit-equal repeats, bit-equal for every legal ws_bytes, poison, an utterance alone,
exact zeros in the rows of gx that no output reads, a refused call writes nothing.

The packed input lies between frames of NaN that no utterance owns (offsets[0] = 3): a read outside the owned rows shows in the
outputs.  Layout "odd" puts every operand on a pitch beyond its width and 4 bytes off a 16-byte boundary."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gconv_cases as gc                                            # noqa: E402
import poison                                                       # noqa: E402
import ref_gconv as rg                                              # noqa: E402

pytestmark = pytest.mark.gpu

OUT_FILL = 0x5A
LEAD, TRAIL = 3, 2                                                  # frames of NaN in front of and behind the owned ones
OUTPUTS = ("z", "y", "gx", "gw", "gbias", "ggamma", "gbeta")
_CASES = {}


def case_of(name):
    """The inputs and the oracle of a case, computed once and never changed."""
    if name not in _CASES:
        c = gc.make(name)
        fwd = rg.forward(c["x"], c["lens"], c["F_in"], c["window"], c["w"], c["b"], c["bn"], c["act"])
        bwd = rg.backward(fwd, c["gy"])
        _CASES[name] = (c, fwd, bwd, rg.bounds(fwd, bwd))
    return _CASES[name]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def poisoned(arr, byte=OUT_FILL):
    return bool(np.all(np.ascontiguousarray(arr).view(np.uint8) == byte))


def gconv_call(c, ws_bytes=None, fill=OUT_FILL, want_gx=True, drop_bn=None, window=None, channels=None, out_dim=None, extra_total=0,
               ldx_short=False, ws_offset=0):
    """xv_gconv_forward then xv_gconv_backward on the case's float32 arrays, every output and the workspace filled bytewise with
    `fill` first -> (rc forward, rc backward, dict of numpy outputs, raw padded arrays, nothing else written)."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    x, gy, w = c["x"], c["gy"], c["w"]
    kh, kw, st, sf = c["window"]
    F_in = c["F_in"]
    F_out = -(-F_in // sf)
    rows, Cc = x.shape
    N, K = w.shape
    odd = c["layout"] == "odd"
    shift = 1 if odd else 0                                          # floats between the 16-byte aligned allocation and the base
    ldx = Cc + 3 if odd else Cc
    ldw = K + 5 if odd else (K + 3) // 4 * 4
    ldz, ldy, ldgy, ldgx = (N + 1, N + 2, N + 3, Cc + 1) if odd else (N, N + 4, N, Cc)
    offsets = gc.offsets(c) + LEAD
    batch = offsets.size - 1
    total_in = int(offsets[-1] - offsets[0]) + extra_total
    n_out = int(sum(rg.out_lens(c["lens"], kh, st))) * F_out
    total_out = n_out // F_out + extra_total
    rows_out = total_out * F_out
    all_rows = rows + (LEAD + TRAIL) * F_in

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

    xd = padded(x, ldx, all_rows, LEAD * F_in, float("nan"))
    wd, gyd = padded(w, ldw, N), padded(gy, ldgy, max(rows_out, 1))
    bd = vec(c["b"])
    bn = [None] * 4 if c["bn"] is None else [vec(v) for v in c["bn"]]
    if drop_bn is not None:
        bn[drop_bn] = None
    offd = torch.from_numpy(offsets.astype(np.int32)).cuda()
    (zb, z), (yb, y), (gwb, gw) = out(rows_out, ldz), out(rows_out, ldy), out(N, ldw)
    gxb, gx = out(all_rows, ldgx) if want_gx else (None, None)
    gb, gg, gbe = (poison.fill(torch.empty((N,), dtype=torch.float32, device="cuda"), fill) for _ in range(3))
    win = c["window"] if window is None else window
    C_, N_ = Cc if channels is None else channels, N if out_dim is None else out_dim
    need = max(int(lib.xv_gconv_workspace(batch, total_in, total_out, F_in, kh, kw, st, sf, Cc, N)), 0)
    given = need if ws_bytes is None else ws_bytes
    wsb = poison.fill(torch.empty(max(given, 16) + 32, dtype=torch.uint8, device="cuda"), fill)
    ws = wsb[ws_offset:]
    ldx_ = ldx if not ldx_short else Cc - 1
    rc_f = lib.xv_gconv_forward(0, _p(xd), ldx_, C_, F_in, win[0], win[1], win[2], win[3], _p(offd), batch, total_in, total_out, _p(wd),
                                ldw, N_, _p(bd), _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]), c["act"], _p(z), ldz, _p(y), ldy, _p(ws),
                                given, None)
    poison.fill(wsb, fill)                                           # the backward call builds its own maps
    rc_b = lib.xv_gconv_backward(0, _p(gyd), ldgy, _p(xd), ldx_, C_, F_in, win[0], win[1], win[2], win[3], _p(offd), batch, total_in,
                                 total_out, _p(z), ldz, _p(wd), ldw, N_, _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]), c["act"], _p(gx),
                                 ldgx, _p(gw), _p(gb) if c["b"] is not None else None, _p(gg), _p(gbe), _p(ws), given, None)
    torch.cuda.synchronize()
    raw = dict(z=zb.cpu().numpy(), y=yb.cpu().numpy(), gx=None if gxb is None else gxb.cpu().numpy(), gw=gwb.cpu().numpy(),
               gbias=gb.cpu().numpy(), ggamma=gg.cpu().numpy(), gbeta=gbe.cpu().numpy())
    view = dict(z=z.cpu().numpy(), y=y.cpu().numpy(), gx=None if gx is None else gx.cpu().numpy(), gw=gw.cpu().numpy())
    lead = LEAD * F_in
    got = dict(z=view["z"][:n_out, :N], y=view["y"][:n_out, :N], gx=None if gx is None else view["gx"][lead:lead + rows, :Cc],
               gw=view["gw"][:, :K], gbias=raw["gbias"], ggamma=raw["ggamma"], gbeta=raw["gbeta"])
    # what the call must leave alone: beyond the widths, beyond the last output row, the rows of gx no utterance owns
    rest = [view["z"][:, N:], view["y"][:, N:], view["gw"][:, K:], view["z"][n_out:], view["y"][n_out:]]
    if gx is not None:
        rest += [view["gx"][:, Cc:], view["gx"][:lead], view["gx"][lead + rows:]]
    untouched = all(poisoned(v, fill) for v in rest)
    return rc_f, rc_b, got, raw, untouched


def ok_call(c, **k):
    from tf_kaldi_speaker_amd import _lib
    rc_f, rc_b, got, raw, untouched = gconv_call(c, **k)
    _lib.check(rc_f)
    _lib.check(rc_b)
    assert untouched, "something beyond the outputs was written"
    return got


def names_of(c):
    # without batch norm ggamma and gbeta are no outputs of the call, without a bias gbias is none: they keep what they held
    drop = (() if c["bn"] is not None else ("ggamma", "gbeta")) + (() if c["b"] is not None else ("gbias",))
    return tuple(k for k in OUTPUTS if k not in drop)


def same_bits(a, b, what, names):
    for k in names:
        if a[k] is None or b[k] is None:
            continue
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("name", [c[0] for c in gc.CASES])
def test_every_element_within_the_bound(name):
    c, fwd, bwd, bnd = case_of(name)
    gc.precondition(c, fwd)
    got = ok_call(c)
    ref = dict(z=fwd["z"], y=fwd["y"], gx=bwd["gx"], gw=bwd["gw"], gbias=bwd["gbias"] if c["b"] is not None else None,
               ggamma=bwd["ggamma"], gbeta=bwd["gbeta"])
    worst, l2 = {}, {}
    for k in OUTPUTS:
        if ref[k] is None:
            assert poisoned(got[k]), "%s is not an output of this call" % k
            continue
        assert np.all(np.isfinite(got[k])), k
        err = np.abs(got[k].astype(np.float64) - ref[k])
        assert np.all(err[bnd[k] == 0] == 0), k
        worst[k] = float(np.max(err / (bnd[k] + 1e-300))) if np.any(err > 0) else 0.0
        norm = np.linalg.norm(ref[k])
        l2[k] = float(np.linalg.norm(err) / norm) if norm > 0 else float(np.linalg.norm(err))
    unread = rg.unread_inputs(fwd)
    assert not got["gx"][unread].any(), "a row of gx that no output reads is not an exact zero"
    print("%s: window=%s C=%d N=%d F=%d rows=%d bias=%s bn=%s act=%d  error/bound %s  rel-L2 %s"
          % (name, c["window"], c["x"].shape[1], c["w"].shape[0], c["F_in"], fwd["z"].shape[0], c["b"] is not None, c["bn"] is not None,
             c["act"], " ".join("%s %.3f" % kv for kv in sorted(worst.items())), " ".join("%s %.2e" % kv for kv in sorted(l2.items()))))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert all(v <= 1e-4 for v in l2.values()), l2


def _dims(c):
    kh, kw, st, sf = c["window"]
    return (len(c["lens"]), int(sum(c["lens"])), int(sum(rg.out_lens(c["lens"], kh, st))), c["F_in"], kh, kw, st, sf, c["x"].shape[1],
            c["w"].shape[0])


@pytest.mark.parametrize("name", ["k33_s12_c3", "k33_s22_c33", "k11_s22_c4", "long"])
def test_bits_do_not_depend_on_repeat_workspace_or_poison(name):
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    c = case_of(name)[0]
    names = names_of(c)
    base = ok_call(c)
    same_bits(base, ok_call(c), "repeat", names)
    least, full = int(lib.xv_gconv_workspace_min(*_dims(c))), int(lib.xv_gconv_workspace(*_dims(c)))
    assert 0 < least <= full
    for ws in (least, full, full + 16, full + 4096 + 48):
        same_bits(base, ok_call(c, ws_bytes=ws), "ws_bytes %d" % ws, names)
    same_bits(base, ok_call(c, ws_offset=16), "workspace 16 bytes further", names)
    for fill in poison.FILLS:
        got = ok_call(c, ws_bytes=least, fill=fill)
        same_bits(base, got, "fill %#x" % fill, names)
        assert all(poisoned(got[k], fill) for k in OUTPUTS if k not in names)
    # host bounds beyond the true totals size grids only (the ranges of gw are a function of total_out)
    same_bits(base, ok_call(c, extra_total=3), "total_in and total_out 3 frames beyond", tuple(k for k in names if k != "gw"))


@pytest.mark.parametrize("name", ["k33_s11_c4", "k33_s22_c33", "k33_s22_c4", "k11_s12_c1"])
def test_an_utterance_does_not_depend_on_its_batch(name):
    c = case_of(name)[0]
    kh, kw, st, sf = c["window"]
    base = ok_call(c)
    F_out = -(-c["F_in"] // sf)
    off = gc.offsets(c) * c["F_in"]
    oo = np.concatenate([[0], np.cumsum(rg.out_lens(c["lens"], kh, st))]) * F_out
    for b in range(len(c["lens"])):
        if c["lens"][b] == 0:                                          # alone it is a call with total_out = 0: nothing touched
            continue
        got = ok_call(gc.alone(c, b))
        for k in ("z", "y"):
            assert got[k].tobytes() == base[k][oo[b]:oo[b + 1]].tobytes(), (k, b)
        assert got["gx"].tobytes() == base["gx"][off[b]:off[b + 1]].tobytes(), ("gx", b)


def test_gx_may_be_null():
    c = case_of("k33_s11_c1")[0]
    base = ok_call(c)
    got = ok_call(c, want_gx=False)
    same_bits(base, got, "gx = NULL", names_of(c))
    assert got["gx"] is None


def test_nothing_to_do_touches_nothing():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    c = dict(case_of("k33_s11_c4")[0])
    for lens in ([], [0, 0]):                                          # batch = 0; no output rows
        empty = dict(c, x=c["x"][:0], lens=lens, gy=c["gy"][:0])
        rc_f, rc_b, _, raw, untouched = gconv_call(empty, ws_bytes=0)
        assert rc_f == 0 and rc_b == 0 and untouched and all(poisoned(v) for v in raw.values())
    for f in (lib.xv_gconv_workspace, lib.xv_gconv_workspace_min):
        assert int(f(0, 0, 0, 7, 3, 3, 1, 1, 4, 33)) == 0 and int(f(2, 0, 0, 7, 3, 3, 1, 1, 4, 33)) == 0
    assert int(lib.xv_gconv_forward_workspace(0, 0, 7, 1)) == 0


def test_a_refused_call_writes_nothing():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    c = case_of("k33_s11_c4")[0]
    least = int(lib.xv_gconv_workspace_min(*_dims(c)))
    rc_f, rc_b, _, raw, _ = gconv_call(c, ws_bytes=least - 16)
    assert rc_f == 0 and rc_b == _lib.XV_ERR_WORKSPACE              # the forward needs its row map only
    assert all(poisoned(raw[k]) for k in ("gx", "gw", "gbias", "ggamma", "gbeta"))
    d = _dims(c)
    rc_f, rc_b, _, raw, _ = gconv_call(c, ws_bytes=int(lib.xv_gconv_forward_workspace(d[0], d[2], d[3], d[7])) - 16)
    assert rc_f == _lib.XV_ERR_WORKSPACE and rc_b == _lib.XV_ERR_WORKSPACE and all(poisoned(v) for v in raw.values())
    rc_f, rc_b, _, raw, _ = gconv_call(c, ws_offset=4)
    assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and all(poisoned(v) for v in raw.values())
    for drop in range(4):                                          # some, but not all, of the four batch-norm pointers
        rc_f, rc_b, _, raw, _ = gconv_call(c, drop_bn=drop)
        assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and all(poisoned(v) for v in raw.values())
    for kw in (dict(window=(2, 3, 1, 1)), dict(window=(3, 5, 1, 1)), dict(window=(3, 3, 3, 1)), dict(window=(3, 3, 1, 0)),
               dict(window=(0, 3, 1, 1)), dict(channels=0), dict(channels=1821), dict(out_dim=4097), dict(out_dim=0)):
        rc_f, rc_b, _, raw, _ = gconv_call(c, **kw)
        assert rc_f == _lib.XV_ERR_UNSUPPORTED and rc_b == _lib.XV_ERR_UNSUPPORTED and all(poisoned(v) for v in raw.values()), kw
    rc_f, rc_b, _, raw, _ = gconv_call(c, ldx_short=True)
    assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and all(poisoned(v) for v in raw.values())
    rc_f, rc_b, _, raw, _ = gconv_call(dict(c, act=3))
    assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID and all(poisoned(v) for v in raw.values())
    assert int(lib.xv_gconv_workspace(1, 5, 5, 7, 2, 3, 1, 1, 4, 33)) == _lib.XV_ERR_UNSUPPORTED
    # the limits the header promises are legal sizes
    assert int(lib.xv_gconv_workspace_min(64, 19200, 19200, 40, 3, 3, 1, 1, 64, 64)) > 0
    assert int(lib.xv_gconv_workspace(1 << 12, 1 << 12, 1 << 12, 4096, 3, 3, 1, 1, 1820, 4096)) > 0


# ---------------------------------------------------------------------------------------------- the residual join
def add_act_call(p, q, gy, act, odd, fill=OUT_FILL):
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    rows, N = p.shape
    lds = (N + 1, N + 2, N + 3, N + 5, N + 7) if odd else (N,) * 5
    shift = 1 if odd else 0

    def put(a, ld):
        buf = torch.full((rows * ld + shift + 4,), float("nan"), dtype=torch.float32, device="cuda")
        t = buf[shift:shift + rows * ld].view(rows, ld)
        t[:, :N] = torch.from_numpy(a).cuda()
        return t

    def out(ld):
        buf = poison.fill(torch.empty((rows * ld + shift + 4,), dtype=torch.float32, device="cuda"), fill)
        return buf[shift:shift + rows * ld].view(rows, ld)

    pd, qd, gyd, y, g = put(p, lds[0]), put(q, lds[1]), put(gy, lds[2]), out(lds[3]), out(lds[4])
    _lib.check(lib.xv_add_act_forward(0, _p(pd), lds[0], _p(qd), lds[1], rows, N, act, _p(y), lds[3], None))
    _lib.check(lib.xv_add_act_backward(0, _p(gyd), lds[2], _p(pd), lds[0], _p(qd), lds[1], rows, N, act, _p(g), lds[4], None))
    torch.cuda.synchronize()
    y, g = y.cpu().numpy(), g.cpu().numpy()
    assert poisoned(y[:, N:], fill) and poisoned(g[:, N:], fill)
    return y[:, :N], g[:, :N]


@pytest.mark.parametrize("shape", [(1, 1), (9, 7), (65537, 1)])        # 1, 63 and 64 k + 1 elements
@pytest.mark.parametrize("odd", [False, True])
def test_add_act_is_numpy_float32(shape, odd):
    r = np.random.RandomState(11)
    p, q, gy = (r.standard_normal(shape).astype(np.float32) for _ in range(3))
    flat_p, flat_q = p.reshape(-1), q.reshape(-1)
    flat_q[0] = -flat_p[0]                                            # p + q = +0
    if flat_p.size > 2:
        flat_p[1], flat_q[1] = np.float32(-0.0), np.float32(-0.0)     # p + q = -0
        flat_q[2] = -flat_p[2]
    assert shape[0] * shape[1] in (1, 63, 64 * 1024 + 1)
    for act in (rg.NONE, rg.RELU, rg.LRELU):
        y, g = add_act_call(p, q, gy, act, odd)
        assert y.tobytes() == rg.add_act(p, q, act).tobytes(), act
        assert g.tobytes() == rg.add_act_grad(gy, p, q, act).tobytes(), act


def test_add_act_refuses_before_it_writes():
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    t = poison.fill(torch.empty((4, 4), dtype=torch.float32, device="cuda"), OUT_FILL)
    assert lib.xv_add_act_forward(0, _p(t), 4, _p(t), 4, 4, 4, 3, _p(t), 4, None) == _lib.XV_ERR_INVALID
    assert lib.xv_add_act_forward(0, _p(t), 3, _p(t), 4, 4, 4, 1, _p(t), 4, None) == _lib.XV_ERR_INVALID
    assert lib.xv_add_act_backward(0, _p(t), 4, _p(t), 4, _p(t), 4, 4, 4, 1, _p(t), 3, None) == _lib.XV_ERR_INVALID
    assert lib.xv_add_act_forward(0, _p(t), 4, _p(t), 4, 0, 4, 1, _p(t), 4, None) == 0
    torch.cuda.synchronize()
    assert poisoned(t.cpu().numpy())
