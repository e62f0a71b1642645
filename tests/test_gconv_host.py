"""CPU: the float64 oracle of xv_gconv_forward / xv_gconv_backward (tests/helpers/ref_gconv.py) against torch.autograd of
F.pad + F.conv2d + eval-mode batch_norm + relu / leaky_relu(0.2) in float64, per utterance, for every case of
tests/helpers/gconv_cases.py; the condition those cases keep (no h within 64 bounds of zero); the placement of TensorFlow's
'same' padding; the numpy twin of xv_add_act_*; and that the new translation unit is built."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gconv_cases as gc                                            # noqa: E402
import ref_gconv as rg                                              # noqa: E402
import ref_grid as rgd                                              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES = {}


def case_of(name):
    if name not in _CASES:
        c = gc.make(name)
        fwd = rg.forward(c["x"], c["lens"], c["F_in"], c["window"], c["w"], c["b"], c["bn"], c["act"])
        _CASES[name] = (c, fwd, rg.backward(fwd, c["gy"]))
    return _CASES[name]


def torch_reference(c):
    """The same layer in torch float64, one utterance at a time -> dict(z, y, gx, gw, gbias, ggamma, gbeta) as numpy."""
    import torch
    import torch.nn.functional as Fn
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)         # noqa: E731
    kh, kw, st, sf = c["window"]
    C, N, F_in = c["x"].shape[1], c["w"].shape[0], c["F_in"]
    x, w = t(c["x"]), t(c["w"])
    b = None if c["b"] is None else t(c["b"])
    bn = None if c["bn"] is None else [t(v) for v in c["bn"]]
    w4 = w.reshape(N, kh, kw, C).permute(0, 3, 1, 2)
    zs, row = [], 0
    for L in c["lens"]:
        if L == 0:
            continue
        xu = x[row:row + L * F_in].reshape(1, L, F_in, C).permute(0, 3, 1, 2)
        row += L * F_in
        (Lo, pt), (Fo, pf) = rgd.same_pad(L, kh, st), rgd.same_pad(F_in, kw, sf)
        tt, tf = max((Lo - 1) * st + kh - L, 0), max((Fo - 1) * sf + kw - F_in, 0)
        assert pt == tt // 2 and pf == tf // 2
        z = Fn.conv2d(Fn.pad(xu, (pf, tf - pf, pt, tt - pt)), w4, b, stride=(st, sf))
        assert tuple(z.shape) == (1, N, Lo, Fo)
        zs.append(z.permute(0, 2, 3, 1).reshape(Lo * Fo, N))
    z = torch.cat(zs)
    h = z if bn is None else Fn.batch_norm(z, bn[2].detach(), bn[3].detach(), bn[0], bn[1], False, 0.0, 1e-3)
    y = h if c["act"] == rg.NONE else (Fn.relu(h) if c["act"] == rg.RELU else Fn.leaky_relu(h, rg.SLOPE))
    (y * torch.tensor(c["gy"].astype(np.float64))).sum().backward()
    g = lambda v: None if v is None else v.grad.numpy()                                     # noqa: E731
    return dict(z=z.detach().numpy(), y=y.detach().numpy(), gx=g(x), gw=g(w), gbias=g(b), ggamma=g(bn[0]) if bn else None,
                gbeta=g(bn[1]) if bn else None)


@pytest.mark.parametrize("name", [c[0] for c in gc.CASES])
def test_the_oracle_is_torch_autograd(name):
    c, fwd, bwd = case_of(name)
    ref = torch_reference(c)
    got = dict(z=fwd["z"], y=fwd["y"], gx=bwd["gx"], gw=bwd["gw"], gbias=bwd["gbias"] if c["b"] is not None else None,
               ggamma=bwd["ggamma"], gbeta=bwd["gbeta"])
    for k, v in ref.items():
        if v is None:
            continue
        scale = max(float(np.max(np.abs(v))), 1e-30)
        assert got[k].shape == v.shape, k
        assert float(np.max(np.abs(got[k] - v))) <= 1e-11 * scale * max(fwd["x"].shape), k


@pytest.mark.parametrize("name", [c[0] for c in gc.CASES])
def test_no_h_lies_near_the_discontinuity(name):
    c, fwd, _ = case_of(name)
    zero, exact, far = gc.precondition(c, fwd)
    assert zero + exact + far == fwd["h"].size or c["act"] == rg.NONE


def test_the_cases_cover_what_the_kernels_branch_on():
    windows = {c[1] for c in gc.CASES}
    assert windows == {(3, 3, 1, 1), (3, 3, 1, 2), (3, 3, 2, 2), (1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 2, 2)}
    assert {c[2] for c in gc.CASES} == {1, 3, 4, 33, 68} and {c[3] for c in gc.CASES} == {1, 31, 33, 68}
    assert {c[4] for c in gc.CASES} == {1, 2, 5, 6, 7, 40}
    rows = {name: case_of(name)[1]["z"].shape[0] for name in ("k33_s12_c3", "k33_s22_c33", "k11_s11_c68", "long")}
    assert rows == {"k33_s12_c3": 63, "k33_s22_c33": 64, "k11_s11_c68": 65, "long": 1120}
    assert rg.split_of(1120, 36, 31)[1] == 2 and rg.split_of(1024, 36, 31)[1] == 1
    assert rg.split_of(768000, 576, 64) == (6752, 114)                # the first stage of the ResNet at the recipe's batch
    assert {(c[6], c[7]) for c in gc.CASES} == {(False, True), (True, True), (False, False), (True, False)}
    assert {c[8] for c in gc.CASES} == {rg.NONE, rg.RELU, rg.LRELU}


def test_same_padding_parities():
    # (size, window, stride) -> (output size, zeros in front): stride 2 pads an even size 0 / 1 and an odd size 1 / 1
    assert rgd.same_pad(6, 3, 2) == (3, 0) and rgd.same_pad(7, 3, 2) == (4, 1) and rgd.same_pad(40, 3, 2) == (20, 0)
    assert rgd.same_pad(1, 3, 1) == (1, 1) and rgd.same_pad(1, 3, 2) == (1, 1) and rgd.same_pad(2, 3, 2) == (1, 0)
    assert rgd.same_pad(5, 1, 2) == (3, 0) and rgd.same_pad(6, 1, 2) == (3, 0) and rgd.same_pad(5, 3, 1) == (5, 1)
    # a strided 1 x 1 reads the even positions only: the odd ones have no reader and a zero gradient
    c, fwd, bwd = case_of("k11_s22_c4")
    unread = rg.unread_inputs(fwd)
    frames = np.concatenate([np.arange(n) for n in c["lens"]]).repeat(c["F_in"])
    bins = np.tile(np.arange(c["F_in"]), int(sum(c["lens"])))
    assert np.array_equal(unread, (frames % 2 == 1) | (bins % 2 == 1))
    assert not bwd["gx"][unread].any() and bwd["gx"][~unread].any()
    # time is padded per utterance: no window reads a neighbour's frames
    idx, _, _ = rgd.gather_windows([2, 3], 1, 3, 1, 1, 1)
    assert idx.tolist() == [[-1, 0, 1], [0, 1, -1], [-1, 2, 3], [2, 3, 4], [3, 4, -1]]


def test_add_act_twin():
    r = np.random.RandomState(5)
    p = r.standard_normal((7, 5)).astype(np.float32)
    q = r.standard_normal((7, 5)).astype(np.float32)
    q[0] = -p[0]                                                       # p + q = +0: the lower branch
    p[1, 0], q[1, 0] = np.float32(-0.0), np.float32(-0.0)              # p + q = -0
    gy = r.standard_normal((7, 5)).astype(np.float32)
    s = p.astype(np.float64) + q.astype(np.float64)
    for act, slope in ((rg.NONE, 1.0), (rg.RELU, 0.0), (rg.LRELU, rg.SLOPE)):
        y, g = rg.add_act(p, q, act), rg.add_act_grad(gy, p, q, act)
        assert y.dtype == np.float32 and g.dtype == np.float32
        want_y = np.where(s > 0, s, slope * s)
        want_g = gy * np.where(s > 0, 1.0, slope)
        assert np.max(np.abs(y - want_y)) <= 2.0 ** -23 * np.max(np.abs(want_y)) and np.max(np.abs(g - want_g)) <= 2.0 ** -23 * 4
        if act != rg.NONE:
            assert not y[0].any() and (np.array_equal(g[0], gy[0] * np.float32(0.2)) if act == rg.LRELU else not g[0].any())
        else:
            assert np.array_equal(g, gy)


def test_the_unit_is_built_and_bound():
    import __graft_entry__ as ge
    from tf_kaldi_speaker_amd import _lib
    assert "gconv_grad.hip" in ge.SOURCES and os.path.isfile(os.path.join(ge.CSRC, "gconv_grad.hip"))
    for name in ("xv_gconv_workspace", "xv_gconv_workspace_min", "xv_gconv_forward_workspace", "xv_gconv_forward", "xv_gconv_backward",
                 "xv_add_act_forward", "xv_add_act_backward"):
        assert name in _lib.EXPORTS
