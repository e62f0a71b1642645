"""The gradient of the triplet heads on the GPU (csrc/metric_loss_grad.hip) through the C ABI (xv_metric_loss_grad): the four
forward outputs bit for bit those of xv_metric_loss; grad_x element by element against the float64 oracle
tests/helpers/ref_metric_grad.py on the float32 rows the GPU got, within its bounds() (derived in the header of the kernel file);
the rule's choices on ties and degenerate rows; purity (alone, in a batch, permuted, repeated, twice the workspace); poisoned
buffers; the limits.  Every parity case first asserts on the CPU that the oracle's decision margins exceed 1e-9: the forward's
double error is near 1e-13, so GPU and oracle take the same branches.

Every comparison prints the largest observed error as a fraction of its bound before it asserts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_metric_grad as rg                                        # noqa: E402
from test_metric_grad_host import AM, ARC, degenerate_cases, rows_and_labels      # noqa: E402

pytestmark = pytest.mark.gpu

KIND = {"semihard": 0, "all": 1, "hard": 2}
HEAD = {"asoftmax": 1, AM: 2, ARC: 3}
FILL = 0xFF
OPTIONS = [("semihard", dict(margin=0.2, squared=False, normalize=True)),
           ("semihard", dict(margin=30.0, squared=True, normalize=False)),
           ("all", dict(loss_type="asoftmax", margin=4)),
           ("all", dict(loss_type=ARC, margin=0.3)),
           ("hard", dict(loss_type="asoftmax", margin=2)),
           ("hard", dict(loss_type=AM, margin=0.2))]
EVERY_HEAD = OPTIONS + [("semihard", dict(margin=0.2, squared=True, normalize=True)),
                        ("semihard", dict(margin=2.0, squared=False, normalize=False)),
                        ("all", dict(loss_type="asoftmax", margin=1)), ("all", dict(loss_type="asoftmax", margin=2)),
                        ("all", dict(loss_type=AM, margin=0.2)), ("hard", dict(loss_type="asoftmax", margin=1)),
                        ("hard", dict(loss_type="asoftmax", margin=4)), ("hard", dict(loss_type=ARC, margin=0.3))]
# (d, B, ldx, ldg, classes, seed): 16 / 17 / 33 are the tile and half-wave edges, 257 the second pass over the panel's columns,
# 1024 the LDS limit (64 labels of 16 rows)
SHAPES = [(1, 2, 1, 1, 2, 1), (3, 3, 5, 4, 2, 2), (17, 15, 17, 19, 4, 3), (130, 16, 131, 130, 4, 4), (3, 17, 8, 3, 3, 5),
          (17, 33, 19, 17, 5, 6), (130, 257, 130, 132, 9, 7), (8, 1024, 8, 8, 64, 8)]


def make_rows(d, b, classes, seed):
    if b == 1024:
        rs = np.random.RandomState(seed)
        cls = rs.permutation(np.repeat(np.arange(64), 16))
        x = rs.standard_normal((64, d))[cls] * 0.8 + rs.standard_normal((b, d))
        return x.astype(np.float32), (cls * 7 - 3).astype(np.int32)
    return rows_and_labels(seed, b, d, classes)


_ORACLE = {}


def oracle(kind, o, x, labels, grad_scale=1.0):
    key = (kind, tuple(sorted(o.items())), x.tobytes(), labels.tobytes(), grad_scale)
    if key not in _ORACLE:
        _ORACLE[key] = rg.grad(kind, x, labels, grad_scale=grad_scale, **o)
    return _ORACLE[key]


def abi(x, labels, offsets, kind, o, ldx=None, ldg=None, grad_scale=1.0, ws_factor=1, x_shift=0):
    """One xv_metric_loss_grad call.  Rows are padded to `ldx` with NaN behind every row and after the last; the outputs and the
    workspace are prefilled with 0xFF bytes; `x_shift` floats move the base off its 16-byte alignment.
    -> dict(rc, need, loss, rows, counts, gcounts, grad [n, d], raw = the whole grad_x buffer as bytes, ldg)."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    ldx, ldg = ldx or d, ldg or d
    host = np.full(x_shift + n * ldx + 5, np.nan, dtype=np.float32)
    host[x_shift:x_shift + n * ldx].reshape(n, ldx)[:, :d] = x
    xd = torch.from_numpy(host).cuda()
    ld = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    groups = len(off) - 1
    ptr = off.ctypes.data_as(C.c_void_p)
    kid = KIND.get(kind, kind)
    need = int(lib.xv_metric_loss_grad_workspace(groups, ptr, d, kid))
    filled = lambda count, dtype: torch.full((count * np.dtype(dtype).itemsize,), FILL, dtype=torch.uint8, device="cuda")  # noqa: E731
    ws = filled(max(need, 0) * ws_factor + 64, np.uint8)
    rows, counts = filled(n, np.float64), filled(n, np.int64)
    gloss, gcount = filled(max(groups, 1), np.float64), filled(2 * max(groups, 1), np.int64)
    gx = filled(n * ldg + 7, np.float32)
    p = lambda t, shift=0: C.c_void_p(t.data_ptr() + shift)        # noqa: E731
    rc = lib.xv_metric_loss_grad(0, p(xd, 4 * x_shift), ldx, ptr, groups, d, p(ld), kid, HEAD.get(o.get("loss_type"), 0),
                                 float(o.get("margin", 0.0)), int(o.get("squared", False)), int(o.get("normalize", True)),
                                 float(grad_scale), p(rows), p(counts), p(gloss), p(gcount), p(gx), ldg, p(ws),
                                 max(need, 0) * ws_factor, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    raw = gx.cpu().numpy()
    view = raw[:4 * n * ldg].view(np.float32).reshape(n, ldg)
    return dict(rc=rc, need=need, loss=gloss.cpu().numpy().view(np.float64), rows=rows.cpu().numpy().view(np.float64),
                counts=counts.cpu().numpy().view(np.int64), gcounts=gcount.cpu().numpy().view(np.int64).reshape(-1, 2),
                grad=view[:, :d].copy(), raw=raw, ldg=ldg, n=n, d=d)


def forward(x, labels, offsets, kind, o, ldx=None):
    from test_gpu_metric_loss import abi as forward_abi
    return forward_abi(x, labels, offsets, kind, o, ldx=ldx)


def same_forward(g, f):
    assert f["rc"] == 0
    for k in ("loss", "rows", "counts", "gcounts"):
        assert g[k].tobytes() == f[k].tobytes(), k


def padding_untouched(g):
    raw, n, d, ldg = g["raw"], g["n"], g["d"], g["ldg"]
    body = raw[:4 * n * ldg].reshape(n, 4 * ldg)
    assert np.all(body[:, 4 * d:] == FILL) and np.all(raw[4 * n * ldg:] == FILL)


def check_grad(tag, got, out, d):
    want, tol = out["grad"], rg.bounds(out, d)
    assert np.all(np.isfinite(got))
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = float(np.max(np.where(err == 0.0, 0.0, err / tol)))
    print("%s: max |g| %.3g, error/bound %.3f" % (tag, np.abs(want).max(), frac))
    assert frac <= 1.0


# ------------------------------------------------------------------------------------------------ parity and forward bits
@pytest.mark.parametrize("shape", SHAPES, ids=["d%d-B%d-ldx%d-ldg%d" % s[:4] for s in SHAPES])
@pytest.mark.parametrize("kind,o", OPTIONS, ids=["%s-%s" % (k, "-".join(str(v) for v in o.values())) for k, o in OPTIONS])
def test_gradient_within_the_bound_and_forward_bits(kind, o, shape):
    d, b, ldx, ldg, classes, seed = shape
    x, labels = make_rows(d, b, classes, seed)
    out = oracle(kind, o, x, labels)
    m = rg.margins(out)
    assert min(m.values()) > 1e-9, "the inputs hold a near-tie: %s" % (m,)
    g = abi(x, labels, [0, b], kind, o, ldx=ldx, ldg=ldg)
    assert g["rc"] == 0
    same_forward(g, forward(x, labels, [0, b], kind, o, ldx=ldx))
    np.testing.assert_array_equal(g["counts"], out["res"]["counts"])
    check_grad("%s %s d=%d B=%d" % (kind, o, d, b), g["grad"], out, d)
    padding_untouched(g)


@pytest.mark.parametrize("kind,o", EVERY_HEAD, ids=["%s-%s" % (k, "-".join(str(v) for v in o.values())) for k, o in EVERY_HEAD])
def test_every_kind_and_head(kind, o):
    x, labels = make_rows(17, 33, 5, 6)
    out = oracle(kind, o, x, labels)
    assert min(rg.margins(out).values()) > 1e-9
    g = abi(x, labels, [0, 33], kind, o, ldx=19, ldg=18, x_shift=1)
    assert g["rc"] == 0
    same_forward(g, forward(x, labels, [0, 33], kind, o, ldx=19))
    check_grad("%s %s" % (kind, o), g["grad"], out, 17)
    padding_untouched(g)


# ------------------------------------------------------------------------------------------------ ties and degenerates
@pytest.mark.parametrize("case", degenerate_cases(), ids=lambda c: c[0])
def test_rule_cases_match_the_oracles_choices(case):
    name, kind, o, x, labels = case
    out = oracle(kind, o, x, labels)
    g = abi(x, labels, [0, len(labels)], kind, o)
    assert g["rc"] == 0
    np.testing.assert_array_equal(g["counts"], out["res"]["counts"])
    assert np.all(np.isfinite(g["grad"]))
    if name == "zero_row":
        # under the semi-hard loss the zero row is an anchor at distance sqrt(n_k) = 1 +- an ulp from every unit row: its mining is
        # a tie within rounding, not an exact one, so its choices are not pinned (the cosine kinds, where c = 0 exactly, are)
        return
    check_grad(name, g["grad"], out, x.shape[1])
    if name.startswith("no_negative"):
        assert not g["grad"].any()


# ------------------------------------------------------------------------------------------------ purity
@pytest.mark.parametrize("kind,o", OPTIONS, ids=["%s-%s" % (k, "-".join(str(v) for v in o.values())) for k, o in OPTIONS])
def test_a_group_is_a_pure_function_of_its_rows(kind, o):
    d = 17
    groups = [make_rows(d, b, c, s) for b, c, s in ((33, 5, 6), (15, 4, 3), (40, 6, 9))]
    alone = [abi(x, l, [0, len(l)], kind, o) for x, l in groups]
    assert all(a["rc"] == 0 for a in alone)
    for order in ((0, 1, 2), (2, 0, 1)):
        x = np.concatenate([groups[i][0] for i in order])
        l = np.concatenate([groups[i][1] for i in order])
        off = np.concatenate([[0], np.cumsum([len(groups[i][1]) for i in order])])
        for ws_factor, ldx, shift in ((1, d, 0), (2, d + 3, 3)):
            got = abi(x, l, off, kind, o, ldx=ldx, ws_factor=ws_factor, x_shift=shift)
            assert got["rc"] == 0
            for pos, i in enumerate(order):
                r0, r1 = off[pos], off[pos + 1]
                assert got["grad"][r0:r1].tobytes() == alone[i]["grad"].tobytes()
                assert got["rows"][r0:r1].tobytes() == alone[i]["rows"].tobytes()
                assert got["loss"][pos] == alone[i]["loss"][0]
    again = abi(groups[0][0], groups[0][1], [0, 33], kind, o, ws_factor=2)
    assert again["grad"].tobytes() == alone[0]["grad"].tobytes()
    # grad_scale: the oracle's float32(0.5 g), and exactly half of the unscaled result (a power of two)
    half = abi(groups[0][0], groups[0][1], [0, 33], kind, o, grad_scale=0.5)
    check_grad("grad_scale 0.5", half["grad"], oracle(kind, o, groups[0][0], groups[0][1], grad_scale=0.5), d)
    assert half["rows"].tobytes() == alone[0]["rows"].tobytes()


# ------------------------------------------------------------------------------------------------ limits
def test_limits_leave_the_outputs_alone():
    from tf_kaldi_speaker_amd import _lib
    x, labels = make_rows(4, 12, 3, 1)
    for kind in (3, 4):
        g = abi(x, labels, [0, 12], kind, {})
        assert g["rc"] == _lib.XV_ERR_UNSUPPORTED and g["need"] == _lib.XV_ERR_UNSUPPORTED
        assert np.all(g["raw"] == FILL) and np.all(g["rows"].view(np.uint8) == FILL) and np.all(g["loss"].view(np.uint8) == FILL)
    big = np.zeros((1025, 2), np.float32)
    g = abi(big, np.arange(1025) % 5, [0, 1025], "semihard", dict(margin=0.2))
    assert g["rc"] == _lib.XV_ERR_UNSUPPORTED and np.all(g["raw"] == FILL)
    assert abi(x, labels, [0], "semihard", dict(margin=0.2))["rc"] == 0            # no group: XV_OK, nothing touched


def test_metric_head_returns_the_abi_bits():
    import torch
    from tf_kaldi_speaker_amd import metric_losses as ml
    from tf_kaldi_speaker_amd.params import Params
    x, labels = make_rows(17, 33, 5, 6)
    for params, kind, o in ((Params(loss_func="semihard_triplet_loss", margin=0.2, triplet_loss_squared=False), *OPTIONS[0]),
                            (Params(loss_func="angular_triplet_loss", margin=0.2, triplet_type="hard", loss_type=AM), *OPTIONS[5])):
        head = ml.MetricHead(params, 0)
        g = abi(x, labels, [0, 33], kind, o)
        r = head.loss_and_grad(x, labels)
        assert r.grad_x.tobytes() == g["grad"].tobytes() and r.loss == g["loss"][0]
        np.testing.assert_array_equal(r.rows, g["rows"])
        np.testing.assert_array_equal(r.group_counts, g["gcounts"])
        f = head.loss(x, labels)
        assert f.loss == r.loss and f.rows.tobytes() == r.rows.tobytes()
        t = head.loss_and_grad(torch.from_numpy(x).cuda(), labels, grad_scale=0.5, as_tensor=True)
        assert t.grad_x.is_cuda and np.array_equal(t.grad_x.cpu().numpy(), 0.5 * g["grad"])
