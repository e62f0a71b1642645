"""GPU: xv_bn_batch_forward / xv_bn_batch_backward (csrc/bn_batch.hip) through the raw C ABI against the float64 oracle
tests/helpers/ref_bn_batch.py, on the float32 inputs the kernels saw.

Every element of y, batch_mean, batch_var, moving_mean, moving_variance, gz, ggamma and gbeta must lie within ref_bn_batch.bounds
(the bound derived in the header of csrc/bn_batch.hip, Bz = 0: the oracle starts from the device's own z); no element is left out
(tests/helpers/bn_batch_cases.py keeps every h off the mask's edge, checked on the CPU in tests/test_bn_batch_host.py).  Every
test prints the largest error / bound before it asserts.  The binding properties of include/xvec_hip.h: bit-equal repeats,
bit-equal for a larger workspace, for poisoned workspace and outputs, for padded and 4-byte-offset layouts; refused calls write
nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bn_batch_cases as bc                                         # noqa: E402
import poison                                                       # noqa: E402
import ref_bn_batch as rb                                           # noqa: E402

pytestmark = pytest.mark.gpu

OUT_FILL = 0x5A
OUTPUTS = ("y", "batch_mean", "batch_var", "moving_mean", "moving_variance", "gz", "ggamma", "gbeta")
XV_ERR_INVALID, XV_ERR_UNSUPPORTED, XV_ERR_WORKSPACE = -1, -2, -6
_CASES = {}


def case_of(name):
    """The inputs, the oracle and its bounds of a case, computed once and never changed."""
    if name not in _CASES:
        c = bc.make(name)
        fwd = rb.forward(c["z"], c["gamma"], c["beta"], c["act"])
        bwd = rb.backward(fwd, c["gy"])
        mm, mv, _ = rb.moving(c["mm"], c["mv"], fwd["mu"], fwd["v"], c["n"], c["momentum"], c["bessel"])
        want = dict(y=fwd["y"], batch_mean=fwd["mu"], batch_var=fwd["v"], moving_mean=mm, moving_variance=mv, gz=bwd["gz"],
                    ggamma=bwd["ggamma"], gbeta=bwd["gbeta"])
        b = rb.bounds(fwd, bwd, mm=c["mm"], mv=c["mv"], momentum=c["momentum"], bessel=c["bessel"])
        bars = dict(y=b["y"], batch_mean=b["mu"], batch_var=b["v"], moving_mean=b["moving_mean"], moving_variance=b["moving_variance"],
                    gz=b["gz"], ggamma=b["ggamma"], gbeta=b["gbeta"])
        _CASES[name] = (c, want, bars)
    return _CASES[name]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def poisoned(arr, byte=OUT_FILL):
    return bool(np.all(np.ascontiguousarray(arr).view(np.uint8) == byte))


def bn_call(c, layout="contiguous", ws_factor=1, ws_bytes=None, fill=OUT_FILL, ws_offset=0, **bad):
    """xv_bn_batch_forward then xv_bn_batch_backward on the case's float32 arrays in `layout`, every output and the workspace filled
    bytewise with `fill` first.  `bad` overrides single arguments (n, N, act, momentum, ldz, null=<name>, one_moving) ->
    (rc forward, rc backward, dict of numpy outputs, whether everything beyond the outputs kept the fill)."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    pad, shift = bc.LAYOUTS[layout]
    n, N = c["n"], c["N"]
    ldz, ldy, ldgy, ldgz = N + pad, N + 2 * pad, N + pad, N + 3 * pad

    def mat(a, ld):
        buf = torch.full((n * ld + shift + 4,), float("nan"), dtype=torch.float32, device="cuda")
        t = buf[shift:shift + n * ld].view(n, ld)
        t[:, :N] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        return t

    def vec(a):
        buf = torch.zeros((N + shift + 4,), dtype=torch.float32, device="cuda")
        buf[shift:shift + N] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        return buf[shift:shift + N]

    def out(rows, ld):
        buf = poison.fill(torch.empty((rows * ld + shift + 4,), dtype=torch.float32, device="cuda"), fill)
        return buf, buf[shift:shift + rows * ld].view(rows, ld)

    zd, gyd = mat(c["z"], ldz), mat(c["gy"], ldgy)
    gamma, beta, mm, mv = vec(c["gamma"]), vec(c["beta"]), vec(c["mm"]), vec(c["mv"])
    (yb, y), (gzb, gz) = out(n, ldy), out(n, ldgz)
    (mub, mu), (vb, v), (ggb, gg), (gbb, gb) = (out(1, N) for _ in range(4))
    need = int(lib.xv_bn_batch_workspace_min(n, N))
    assert need == int(lib.xv_bn_batch_workspace(n, N)) and need > 0
    given = ws_factor * need if ws_bytes is None else ws_bytes
    wsb = poison.fill(torch.empty(max(given, 16) + 64, dtype=torch.uint8, device="cuda"), fill)
    ws = wsb[ws_offset:]
    ptr = dict(z=zd, gamma=gamma, beta=beta, mm=mm, mv=mv, y=y, mean=mu, var=v, gy=gyd, gz=gz, ggamma=gg, gbeta=gb)
    if "null" in bad:
        ptr[bad["null"]] = None
    if bad.get("one_moving"):
        ptr["mv"] = None
    n_, N_, act, momentum = bad.get("n", n), bad.get("N", N), bad.get("act", c["act"]), bad.get("momentum", c["momentum"])
    ldz_ = bad.get("ldz", ldz)
    rc_f = lib.xv_bn_batch_forward(0, _p(ptr["z"]), ldz_, n_, N_, _p(ptr["gamma"]), _p(ptr["beta"]), act, momentum, int(c["bessel"]),
                                   _p(ptr["mm"]), _p(ptr["mv"]), _p(ptr["y"]), ldy, _p(ptr["mean"]), _p(ptr["var"]), _p(ws), given, None)
    if rc_f != 0:                            # the backward needs statistics: the oracle's, rounded, when the forward was refused
        ref = rb.forward(c["z"], c["gamma"], c["beta"], c["act"])
        stat_mu, stat_v = vec(ref["mu"]), vec(ref["v"])
    else:
        stat_mu, stat_v = mu.view(-1), v.view(-1)
    if ptr["mean"] is None:
        stat_mu = None
    poison.fill(wsb, fill)                                           # the backward call keeps nothing of the forward's workspace
    rc_b = lib.xv_bn_batch_backward(0, _p(ptr["gy"]), ldgy, _p(ptr["z"]), ldz_, n_, N_, _p(stat_mu), _p(stat_v), _p(ptr["gamma"]),
                                    _p(ptr["beta"]), act, _p(ptr["gz"]), ldgz, _p(ptr["ggamma"]), _p(ptr["gbeta"]), _p(ws), given, None)
    torch.cuda.synchronize()
    yv, gzv = y.cpu().numpy(), gz.cpu().numpy()
    got = dict(y=yv[:, :N], batch_mean=mu.cpu().numpy()[0], batch_var=v.cpu().numpy()[0], moving_mean=mm.cpu().numpy(),
               moving_variance=mv.cpu().numpy(), gz=gzv[:, :N], ggamma=gg.cpu().numpy()[0], gbeta=gb.cpu().numpy()[0])
    raw = [yb, gzb, mub, vb, ggb, gbb]
    edges = [t.cpu().numpy() for b in raw for t in (b[:shift], b[-4:])] + [yv[:, N:], gzv[:, N:]]
    untouched = all(poisoned(e, fill) for e in edges)
    wrote_nothing = untouched and all(poisoned(b.cpu().numpy(), fill) for b in raw) and \
        np.array_equal(got["moving_mean"], c["mm"]) and np.array_equal(got["moving_variance"], c["mv"])
    return rc_f, rc_b, got, untouched, wrote_nothing


def ok_call(c, **k):
    from tf_kaldi_speaker_amd import _lib
    rc_f, rc_b, got, untouched, _ = bn_call(c, **k)
    _lib.check(rc_f)
    _lib.check(rc_b)
    assert untouched, "something beyond the outputs was written"
    return got


def same_bits(a, b, what):
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("name", bc.NAMES)
def test_every_element_within_the_bound(name):
    c, want, bars = case_of(name)
    got = ok_call(c)
    worst = {}
    for k in OUTPUTS:
        err = np.abs(got[k].astype(np.float64) - want[k])
        assert np.all(np.isfinite(got[k])), k
        ratio = np.where(err == 0.0, 0.0, err / np.maximum(bars[k], 1e-300))
        worst[k] = float(ratio.max())
    print("%s: largest error / bound: %s" % (name, ", ".join("%s %.3f" % (k, worst[k]) for k in OUTPUTS)))
    for k in OUTPUTS:
        assert worst[k] <= 1.0, "%s: %s leaves its bound by a factor of %.3f" % (name, k, worst[k])
    # the moving vectors are the float32 replay of the three operations from the returned statistics
    mm, mv = rb.moving_f32(c["mm"], c["mv"], got["batch_mean"], got["batch_var"], c["n"], c["momentum"], c["bessel"])
    assert mm.tobytes() == got["moving_mean"].tobytes() and mv.tobytes() == got["moving_variance"].tobytes()
    if c["family"] == "dyadic":
        assert got["batch_mean"].tobytes() == want["batch_mean"].astype(np.float32).tobytes()
        assert np.array_equal(got["batch_mean"].astype(np.float64), want["batch_mean"])
    if c["zero_col"] is not None:
        assert np.all(got["y"][:, c["zero_col"]] == 0.0) and np.all(got["gz"][:, c["zero_col"]] == 0.0)
    if c["const_col"] is not None:
        assert got["batch_var"][c["const_col"]] == 0.0


@pytest.mark.parametrize("name", bc.NAMES)
def test_same_bits_whatever_the_call_finds(name):
    c, _, _ = case_of(name)
    base = ok_call(c)
    same_bits(base, ok_call(c), "a repeat")
    same_bits(base, ok_call(c, ws_factor=2, ws_offset=48), "a workspace of twice the least size")
    for byte in poison.FILLS:
        same_bits(base, ok_call(c, fill=byte), "workspace and outputs filled with 0x%02X" % byte)
    for layout in ("padded", "offset"):
        same_bits(base, ok_call(c, layout=layout), "layout %s" % layout)


BAD = [
    ("no rows", dict(n=0), XV_ERR_INVALID, XV_ERR_INVALID),
    ("negative rows", dict(n=-3), XV_ERR_INVALID, XV_ERR_INVALID),
    ("no columns", dict(N=0), XV_ERR_INVALID, XV_ERR_INVALID),
    ("too wide", dict(N=4097, ldz=4097), XV_ERR_UNSUPPORTED, XV_ERR_UNSUPPORTED),
    ("too many rows", dict(n=(1 << 24) + 1), XV_ERR_UNSUPPORTED, XV_ERR_UNSUPPORTED),
    ("momentum below 0", dict(momentum=-0.01), XV_ERR_INVALID, 0),
    ("momentum above 1", dict(momentum=1.5), XV_ERR_INVALID, 0),
    ("momentum nan", dict(momentum=float("nan")), XV_ERR_INVALID, 0),
    ("activation 3", dict(act=3), XV_ERR_INVALID, XV_ERR_INVALID),
    ("activation -1", dict(act=-1), XV_ERR_INVALID, XV_ERR_INVALID),
    ("ldz below N", dict(ldz=32), XV_ERR_INVALID, XV_ERR_INVALID),
    ("null z", dict(null="z"), XV_ERR_INVALID, XV_ERR_INVALID),
    ("null gamma", dict(null="gamma"), XV_ERR_INVALID, XV_ERR_INVALID),
    ("null batch_mean", dict(null="mean"), XV_ERR_INVALID, XV_ERR_INVALID),
    ("moving_mean alone", dict(one_moving=True), XV_ERR_INVALID, 0),
    ("workspace too small", dict(ws_bytes=16), XV_ERR_WORKSPACE, XV_ERR_WORKSPACE),
    ("workspace misaligned", dict(ws_offset=4), XV_ERR_INVALID, XV_ERR_INVALID),
]


@pytest.mark.parametrize("what,bad,rc_forward,rc_backward", BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_are_refused_and_write_nothing(what, bad, rc_forward, rc_backward):
    c, _, _ = case_of("n65_N33_lrelu")
    rc_f, rc_b, got, untouched, wrote_nothing = bn_call(c, **bad)
    assert (rc_f, rc_b) == (rc_forward, rc_backward), what
    assert untouched
    if rc_backward != 0:
        assert wrote_nothing, "%s: a refused call wrote something" % what
    else:                                    # the forward alone was refused: its outputs and the moving vectors are untouched
        assert poisoned(got["y"]) and poisoned(got["batch_mean"]) and poisoned(got["batch_var"])
        assert np.array_equal(got["moving_mean"], c["mm"]) and np.array_equal(got["moving_variance"], c["mv"])


def test_momentum_limits_and_no_moving_vectors():
    """momentum 1 leaves the moving vectors alone, momentum 0 moves them all the way to the batch statistics; without moving
    vectors the other outputs keep their bits."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    c, _, _ = case_of("n65_N33_relu")
    base = ok_call(c)
    one = ok_call(dict(c, momentum=1.0))
    assert np.array_equal(one["moving_mean"], c["mm"]) and np.array_equal(one["moving_variance"], c["mv"])
    zero = ok_call(dict(c, momentum=0.0, bessel=False))              # m - (m - mu) * 1: mu up to the rounding of m - mu
    mm, mv = rb.moving_f32(c["mm"], c["mv"], zero["batch_mean"], zero["batch_var"], c["n"], 0.0, False)
    assert zero["moving_mean"].tobytes() == mm.tobytes() and zero["moving_variance"].tobytes() == mv.tobytes()
    assert np.all(np.abs(zero["moving_mean"] - base["batch_mean"]) <= 2 * rb.U * (np.abs(c["mm"]) + np.abs(base["batch_mean"])))
    lib = _lib.load()
    n, N = c["n"], c["N"]
    z = torch.from_numpy(c["z"]).cuda()
    g, b = torch.from_numpy(c["gamma"]).cuda(), torch.from_numpy(c["beta"]).cuda()
    y = torch.empty((n, N), dtype=torch.float32, device="cuda")
    mu, v = torch.empty(N, dtype=torch.float32, device="cuda"), torch.empty(N, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.xv_bn_batch_workspace(n, N)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.xv_bn_batch_forward(0, _p(z), N, n, N, _p(g), _p(b), c["act"], 0.99, 0, None, None, _p(y), N, _p(mu), _p(v), _p(ws),
                                       ws.numel(), None))
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == base["y"].tobytes() and mu.cpu().numpy().tobytes() == base["batch_mean"].tobytes()
    assert v.cpu().numpy().tobytes() == base["batch_var"].tobytes()
