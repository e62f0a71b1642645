"""GPU: xv_seg_forward / xv_seg_backward (csrc/seg_grad.hip) through the raw C ABI against the float64 oracle
tests/helpers/ref_seg_grad.py, on the float32 inputs the kernels saw.

Every element of z, y, gx, gw, gbias, ggamma and gbeta must lie within ref_seg_grad.bounds (the bound derived in the header of
csrc/seg_grad.hip); no element is left out (tests/helpers/seg_grad_cases.py keeps every h off the ReLU's discontinuity, checked
on the CPU in tests/test_seg_grad_host.py).  As a coarse cap that keeps the bound honest the relative L2 error of every output
stays within 1e-4, the project's parity requirement.  Every test prints the largest error / bound before it asserts.  The
binding properties of include/xvec_hip.h: bit-equal repeats, bit-equal for every legal ws_bytes, poison, row independence."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import poison                                                       # noqa: E402
import ref_seg_grad as rs                                           # noqa: E402
import seg_grad_cases as sc                                         # noqa: E402

pytestmark = pytest.mark.gpu

OUT_FILL = 0x5A
OUTPUTS = ("z", "y", "gx", "gw", "gbias", "ggamma", "gbeta")
_CASES = {}


def case_of(name):
    """The inputs and the oracle of a case, computed once and never changed."""
    if name not in _CASES:
        c = sc.make(name)
        fwd = rs.forward(c["x"], c["w"], c["b"], c["bn"], c["act"], rs.SLOPE)
        bwd = rs.backward(fwd, c["gy"], rs.SLOPE)
        _CASES[name] = (c, fwd, bwd, rs.bounds(fwd, bwd))
    return _CASES[name]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pitch(width, pad, extra):
    return (width + 3) // 4 * 4 + 4 * extra if pad == "vec" else width + 2 * extra + 1


def seg_call(c, ws_bytes=None, fill=OUT_FILL, want_gx=True, rows=None, in_dim=None, out_dim=None, drop_bn=None):
    """xv_seg_forward then xv_seg_backward on the case's float32 arrays (`rows`: those rows only), every operand on a pitch
    larger than its width, every output and the workspace filled bytewise with `fill` first -> (rc forward, rc backward, dict
    of numpy outputs, raw padded arrays)."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    x, gy = (c["x"], c["gy"]) if rows is None else (c["x"][rows], c["gy"][rows])
    n, K = x.shape
    N = c["w"].shape[0]
    pad = c["pad"]
    ldx, ldw, ldz, ldy, ldgy, ldgx = (_pitch(K, pad, 1), _pitch(K, pad, 2), _pitch(N, pad, 1), _pitch(N, pad, 2), _pitch(N, pad, 3),
                                      _pitch(K, pad, 3))

    def padded(a, ld, rows_min=1):
        t = torch.zeros((max(a.shape[0], rows_min), ld), dtype=torch.float32, device="cuda")
        t[:a.shape[0], :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        return t

    def vec(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def out(r, ld):
        return poison.fill(torch.empty((max(r, 1), ld), dtype=torch.float32, device="cuda"), fill)

    xd, wd, gyd = padded(x, ldx), padded(c["w"], ldw), padded(gy, ldgy)
    bd = vec(c["b"])
    bn = [None] * 4 if c["bn"] is None else [vec(v) for v in c["bn"]]
    if drop_bn is not None:
        bn[drop_bn] = None
    z, y = out(n, ldz), out(n, ldy)
    gx = out(n, ldgx) if want_gx else None
    gw = out(N, ldw)
    gb, gg, gbe = (poison.fill(torch.empty((N,), dtype=torch.float32, device="cuda"), fill) for _ in range(3))
    K_, N_ = K if in_dim is None else in_dim, N if out_dim is None else out_dim
    rc_f = lib.xv_seg_forward(0, _p(xd), ldx, n, K_, _p(wd), ldw, N_, _p(bd), _p(bn[0]), _p(bn[1]), _p(bn[2]), _p(bn[3]), c["act"],
                              _p(z), ldz, _p(y), ldy, None)
    need = int(lib.xv_seg_workspace(n, K, N))
    given = need if ws_bytes is None else ws_bytes
    ws = poison.fill(torch.empty(max(given, 16), dtype=torch.uint8, device="cuda"), fill)
    rc_b = lib.xv_seg_backward(0, _p(gyd), ldgy, _p(xd), ldx, _p(z), ldz, n, K_, _p(wd), ldw, N_, _p(bn[0]), _p(bn[1]), _p(bn[2]),
                               _p(bn[3]), c["act"], _p(gx), ldgx, _p(gw), _p(gb), _p(gg), _p(gbe), _p(ws), given, None)
    torch.cuda.synchronize()
    raw = dict(z=z.cpu().numpy(), y=y.cpu().numpy(), gx=None if gx is None else gx.cpu().numpy(), gw=gw.cpu().numpy(),
               gbias=gb.cpu().numpy(), ggamma=gg.cpu().numpy(), gbeta=gbe.cpu().numpy())
    got = dict(z=raw["z"][:n, :N], y=raw["y"][:n, :N], gx=None if gx is None else raw["gx"][:n, :K], gw=raw["gw"][:, :K],
               gbias=raw["gbias"], ggamma=raw["ggamma"], gbeta=raw["gbeta"])
    return rc_f, rc_b, got, raw


def ok_call(c, **k):
    from tf_kaldi_speaker_amd import _lib
    rc_f, rc_b, got, raw = seg_call(c, **k)
    _lib.check(rc_f)
    _lib.check(rc_b)
    return got, raw


def same_bits(a, b, what, names=OUTPUTS):
    for k in names:
        if a[k] is None or b[k] is None:
            continue
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def poisoned(arr, byte=OUT_FILL):
    return bool(np.all(np.ascontiguousarray(arr).view(np.uint8) == byte))


@pytest.mark.parametrize("name", [c[0] for c in sc.CASES])
def test_every_element_within_the_bound(name):
    c, fwd, bwd, bnd = case_of(name)
    sc.precondition(c, fwd)
    got, raw = ok_call(c)
    n, K = c["x"].shape
    N = c["w"].shape[0]
    ref = dict(z=fwd["z"], y=fwd["y"], gx=bwd["gx"], gw=bwd["gw"], gbias=bwd["gbias"], ggamma=bwd["ggamma"], gbeta=bwd["gbeta"])
    worst, l2 = {}, {}
    for k in OUTPUTS:
        if ref[k] is None:
            assert poisoned(got[k]), "%s is not an output without batch norm" % k
            continue
        err = np.abs(got[k].astype(np.float64) - ref[k])
        assert np.all(np.isfinite(got[k]))
        worst[k] = float(np.max(err / (bnd[k] + 1e-300))) if np.any(err > 0) else 0.0
        norm = np.linalg.norm(ref[k])
        l2[k] = float(np.linalg.norm(err) / norm) if norm > 0 else float(np.linalg.norm(err))
    print("%s: n=%d K=%d N=%d bn=%s act=%d  error/bound %s  rel-L2 %s"
          % (name, n, K, N, c["bn"] is not None, c["act"], " ".join("%s %.3f" % kv for kv in sorted(worst.items())),
             " ".join("%s %.2e" % kv for kv in sorted(l2.items()))))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert all(v <= 1e-4 for v in l2.values()), l2
    # what lies beyond the widths is left alone
    assert poisoned(raw["z"][:, N:]) and poisoned(raw["y"][:, N:]) and poisoned(raw["gx"][:, K:]) and poisoned(raw["gw"][:, K:])


@pytest.mark.parametrize("name", ["n70", "dyadic_bn", "dyadic_relu"])
def test_bits_do_not_depend_on_repeat_workspace_or_poison(name):
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    c = case_of(name)[0]
    n, K = c["x"].shape
    N = c["w"].shape[0]
    # without batch norm ggamma and gbeta are no outputs of the call: they keep whatever they held
    names = OUTPUTS if c["bn"] is not None else tuple(k for k in OUTPUTS if k not in ("ggamma", "gbeta"))
    base, _ = ok_call(c)
    again, _ = ok_call(c)
    same_bits(base, again, "repeat", names)
    least, full = int(lib.xv_seg_workspace_min(n, K, N)), int(lib.xv_seg_workspace(n, K, N))
    assert least < full                                            # n = 70: two panels at the minimum, one at the full size
    for ws in (least, least + 16, (least + full) // 2 // 16 * 16):
        got, _ = ok_call(c, ws_bytes=ws)
        same_bits(base, got, "ws_bytes %d" % ws, names)
    for fill in poison.FILLS:
        for ws in (least, full):
            got, _ = ok_call(c, ws_bytes=ws, fill=fill)
            same_bits(base, got, "fill %#x ws %d" % (fill, ws), names)
            assert c["bn"] is not None or (poisoned(got["ggamma"], fill) and poisoned(got["gbeta"], fill))


def test_a_row_does_not_depend_on_its_batch():
    c = case_of("n70")[0]
    base, _ = ok_call(c)
    alone, _ = ok_call(c, rows=[5])
    for k in ("z", "y", "gx"):
        assert alone[k][0].tobytes() == base[k][5].tobytes(), k


def test_gx_may_be_null():
    c = case_of("n33")[0]
    base, _ = ok_call(c)
    got, _ = ok_call(c, want_gx=False)
    same_bits(base, got, "gx = NULL")
    assert got["gx"] is None


def test_no_rows_touch_nothing():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    c = dict(case_of("n31")[0])
    rc_f, rc_b, _, raw = seg_call(c, rows=[], ws_bytes=0)
    assert rc_f == 0 and rc_b == 0
    assert all(poisoned(v) for v in raw.values())
    assert int(lib.xv_seg_workspace(0, 35, 33)) == 0 and int(lib.xv_seg_workspace_min(0, 35, 33)) == 0


def test_error_statuses():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    c = case_of("n31")[0]
    n, K = c["x"].shape
    N = c["w"].shape[0]
    least = int(lib.xv_seg_workspace_min(n, K, N))
    rc_f, rc_b, _, raw = seg_call(c, ws_bytes=least - 16)
    assert rc_f == 0 and rc_b == _lib.XV_ERR_WORKSPACE
    assert all(poisoned(raw[k]) for k in ("gx", "gw", "gbias", "ggamma", "gbeta"))
    for drop in range(4):                                          # some, but not all, of the four batch-norm pointers
        rc_f, rc_b, _, raw = seg_call(c, drop_bn=drop)
        assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID
        assert all(poisoned(v) for v in raw.values())
    rc_f, rc_b, _, raw = seg_call(c, in_dim=16385)
    assert rc_f == _lib.XV_ERR_UNSUPPORTED and rc_b == _lib.XV_ERR_UNSUPPORTED and all(poisoned(v) for v in raw.values())
    rc_f, rc_b, _, raw = seg_call(c, out_dim=4097)
    assert rc_f == _lib.XV_ERR_UNSUPPORTED and rc_b == _lib.XV_ERR_UNSUPPORTED and all(poisoned(v) for v in raw.values())
    rc_f, rc_b, _, _ = seg_call(dict(c, act=3))
    assert rc_f == _lib.XV_ERR_INVALID and rc_b == _lib.XV_ERR_INVALID
    # the limits the header promises are legal sizes
    assert int(lib.xv_seg_workspace_min(640, 8192, 2048)) > 0 and int(lib.xv_seg_workspace(640, 16384, 4096)) > 0
