"""Host: the rule of xv_att_pool_forward / xv_att_pool_backward (tests/helpers/ref_att_pool.py) against torch.autograd in float64
of the einsum formulation of model/pooling.py:150-218, for all four split combinations, with and without the scale: the floor
branch (a constant value channel passes nothing from std), the dropped d var / d m term (autograd carries it, the rule does not,
and they agree), the closed form of c[h] (= sum_t w gw), the head sums of a key or value that is not split.  The forward agrees
with oracle.ref_numpy.attention_core.  The case list covers what the issue of the operator asks for."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import att_pool_cases as ac                                         # noqa: E402
import ref_att_pool as ra                                           # noqa: E402

CFGS = [ra.Cfg(H, dq, dv, sk, sv, sc) for (H, dq, dv) in ((1, 5, 4), (3, 4, 5), (2, 1, 3)) for sk in (0, 1) for sv in (0, 1)
        for sc in (0, 1)]


def torch_att(cfg, key, value, query):
    """model/pooling.py:150-218 on one utterance (batch of 1); the mask enters as a constant."""
    import torch
    n, H = key.shape[0], cfg.H
    v = value[None].reshape(1, n, H, cfg.dv).permute(0, 2, 1, 3) if cfg.split_v else value[None, None]
    k = key[None].reshape(1, n, H, cfg.dq).permute(0, 2, 1, 3) if cfg.split_k else key[None, None]
    qk = torch.einsum("bhld,hd->blh" if cfg.split_k else "bmld,hd->blh", k, query) * cfg.scale
    w = torch.softmax(qk.transpose(1, 2), dim=-1)                        # [b, h, l]
    mean = torch.einsum("bhld,bhl->bhd" if cfg.split_v else "bmld,bhl->bhd", v, w)
    var = torch.einsum("bhld,bhl->bhd", (v - mean[:, :, None, :]) ** 2, w)
    mean, var = mean.reshape(1, -1), var.reshape(1, -1)
    mask = (var <= ra.FLOOR).to(torch.float64).detach()
    var = (1.0 - mask) * var + mask * ra.FLOOR
    return torch.cat([mean, torch.sqrt(var)], dim=1)[0], w[0].transpose(0, 1)


def inputs(cfg, n, seed):
    r = np.random.RandomState(seed)
    key = r.standard_normal((n, cfg.Dk))
    value = r.standard_normal((n, cfg.Dv))
    if cfg.Dv > 1:
        value[:, 1] = 0.75                                              # a constant channel: floored
    query = r.standard_normal((cfg.H, cfg.dq))
    gp = r.standard_normal(2 * cfg.P)
    return key, value, query, gp


@pytest.mark.parametrize("n", [1, 2, 9])
@pytest.mark.parametrize("cfg", CFGS, ids=repr)
def test_rule_is_torch_autograd(cfg, n):
    import torch
    key, value, query, gp = inputs(cfg, n, 7 * n + cfg.H)
    kt, vt, qt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (key, value, query))
    pooled, wt = torch_att(cfg, kt, vt, qt)
    pooled.backward(torch.tensor(gp))
    f = ra.forward(cfg, key, value, query)
    want = pooled.detach().numpy()
    assert np.max(np.abs(np.concatenate([f["m"], f["std"]]) - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.max(np.abs(f["w"] - wt.detach().numpy())) <= 1e-14
    b = ra.backward(cfg, key, value, query, f["w"], f["m"], f["std"], f["var"], gp)
    for name, ref in (("gvalue", vt.grad.numpy()), ("gkey", kt.grad.numpy()), ("gquery", qt.grad.numpy())):
        scale = max(np.max(np.abs(ref)), 1e-300)
        rel = np.max(np.abs(b[name] - ref)) / scale
        assert rel <= 1e-11, (name, rel)
    if n == 1:                                                          # one frame: w = 1, everything floored, no key gradient
        assert np.all(f["w"] == 1) and np.all(f["var"] == 0) and np.all(b["gkey"] == 0) and np.all(b["gquery"] == 0)
        if cfg.split_v:
            assert np.array_equal(b["gvalue"][0], gp[:cfg.P])
        else:
            assert np.allclose(b["gvalue"][0], gp[:cfg.P].reshape(cfg.H, cfg.dv).sum(axis=0), rtol=1e-14)


def test_floor_branch_passes_nothing_from_std():
    cfg = ra.Cfg(2, 3, 4, 0, 0, 1)
    key, value, query, gp = inputs(cfg, 9, 3)
    f = ra.forward(cfg, key, value, query)
    assert np.all(f["var"][[1, 5]] <= ra.FLOOR) and np.all(f["std"][[1, 5]] == np.sqrt(ra.FLOOR))
    b = ra.backward(cfg, key, value, query, f["w"], f["m"], f["std"], f["var"], gp)
    gp2 = gp.copy()
    gp2[cfg.P + 1] += 100.0                                             # gs of the floored columns: no effect at all
    gp2[cfg.P + 5] -= 100.0
    b2 = ra.backward(cfg, key, value, query, f["w"], f["m"], f["std"], f["var"], gp2)
    assert all(np.array_equal(b[k], b2[k]) for k in ("gvalue", "gkey", "gquery"))
    gp2[cfg.P] += 1.0                                                   # a live column: it matters
    b3 = ra.backward(cfg, key, value, query, f["w"], f["m"], f["std"], f["var"], gp2)
    assert not np.array_equal(b[k := "gvalue"], b3[k])


@pytest.mark.parametrize("cfg", CFGS[:8], ids=repr)
def test_dropped_term_and_closed_form_of_c(cfg):
    key, value, query, gp = inputs(cfg, 11, 21)
    f = ra.forward(cfg, key, value, query)
    w, m, var = f["w"], f["m"], f["var"]
    gvar = np.where(var > ra.FLOOR, gp[cfg.P:] / (2 * f["std"]), 0.0)
    for h in range(cfg.H):
        v = cfg.value_head(value, h)
        pc = cfg.pcols(h)
        d = v - m[pc][None, :]
        # d var / d m = -2 sum_t w (v - m): zero at the exact weighted mean
        assert np.max(np.abs(w[:, h] @ d)) <= 1e-13 * max(1.0, np.max(np.abs(v)))
        gw = (gp[:cfg.P][pc] * v + gvar[pc] * d * d).sum(axis=1)
        c = (gp[:cfg.P][pc] * m[pc] + gvar[pc] * var[pc]).sum()
        assert abs(w[:, h] @ gw - c) <= 1e-12 * max(1.0, np.max(np.abs(gw)))


@pytest.mark.parametrize("sk,sv", ac.SPLITS)
def test_heads_that_share_rows_add_up(sk, sv):
    """A key or value that is not split receives the sum over the heads; a split one the head's own slice."""
    cfg = ra.Cfg(3, 4, 5, sk, sv, 0)
    key, value, query, gp = inputs(cfg, 7, 5)
    f = ra.forward(cfg, key, value, query)
    b = ra.backward(cfg, key, value, query, f["w"], f["m"], f["std"], f["var"], gp)
    parts_v, parts_k = np.zeros((cfg.H, 7, cfg.dv)), np.zeros((cfg.H, 7, cfg.dq))
    gvar = np.where(f["var"] > ra.FLOOR, gp[cfg.P:] / (2 * f["std"]), 0.0)
    for h in range(cfg.H):
        pc = cfg.pcols(h)
        parts_v[h] = f["w"][:, h:h + 1] * (gp[:cfg.P][pc] + 2 * gvar[pc] * (cfg.value_head(value, h) - f["m"][pc]))
        parts_k[h] = cfg.scale * b["gscore"][:, h:h + 1] * query[h]
    want_v = np.concatenate(list(parts_v), axis=1) if sv else parts_v.sum(axis=0)
    want_k = np.concatenate(list(parts_k), axis=1) if sk else parts_k.sum(axis=0)
    assert np.allclose(b["gvalue"], want_v, rtol=1e-13, atol=1e-15) and np.allclose(b["gkey"], want_k, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("cfg", CFGS, ids=repr)
def test_forward_is_the_oracle(cfg):
    from oracle import ref_numpy
    r = np.random.RandomState(11)
    lens = 6
    key = r.standard_normal((2, lens, cfg.Dk))
    value = r.standard_normal((2, lens, cfg.Dv))
    query = r.standard_normal((cfg.H, cfg.dq))
    att, w = ref_numpy.attention_core(value, key, query, cfg.H, cfg.split_v, cfg.split_k, cfg.use_scale)
    for b in range(2):
        f = ra.forward(cfg, key[b], value[b], query)
        # the oracle divides by sqrt(dq) in float64; the rule multiplies by the float32 scale the caller passes
        assert np.max(np.abs(f["w"] - w[b].T)) <= 1e-6
        assert np.max(np.abs(np.concatenate([f["m"], f["std"]]) - att[b])) <= 1e-6 * max(1.0, np.max(np.abs(att[b])))


def test_no_frames_and_the_case_list():
    cfg = ra.Cfg(2, 3, 4, 1, 0, 1)
    f = ra.forward(cfg, np.zeros((0, cfg.Dk)), np.zeros((0, cfg.Dv)), np.ones((2, 3)))
    assert np.all(f["m"] == 0) and np.all(f["var"] == 0) and np.allclose(f["std"], 1e-6)
    assert len(ac.CASES) == 112
    for H in ac.HEADS:
        for sp in ac.SPLITS:
            cell = [c for c in ac.CASES if c.H == H and (int(c.split_k), int(c.split_v)) == sp]
            assert sorted(c.dq for c in cell) == sorted(ac.WIDTHS) and sorted(c.dv for c in cell) == sorted(ac.WIDTHS)
            assert {c.use_scale for c in cell} == {False, True}
    case = ac.make(ac.CASES[5])
    assert case["key"].shape[1] == ac.CASES[5].Dk and case["gp"].shape == (12, 2 * ac.CASES[5].P)
    again = ac.make(ac.CASES[5])
    assert all(np.array_equal(case[k], again[k], equal_nan=True) for k in ("key", "value", "query", "gp"))
