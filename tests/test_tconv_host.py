"""Host: the rule of xv_tconv_forward / xv_tconv_backward (tests/helpers/ref_tconv.py) against torch.autograd in float64 on
packed variable-length utterances, W = 1 against ref_seg_grad, the condition tests/helpers/tconv_cases.py puts on the GPU
tests' inputs, a float32 evaluation in the stated chain orders against the bounds, and the host helpers of
tf_kaldi_speaker_amd/conv_train.py: the kernel-layout round trip and out_offsets."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_seg_grad as rs                                           # noqa: E402
import ref_tconv as rt                                              # noqa: E402
import tconv_cases as tc                                            # noqa: E402


@pytest.mark.parametrize("taps", [1, 3, 5])
@pytest.mark.parametrize("has_bn", [False, True])
@pytest.mark.parametrize("act", [rt.NONE, rt.RELU, rt.LRELU])
def test_rule_is_torch_autograd(taps, has_bn, act):
    import torch
    import torch.nn.functional as fn
    r = np.random.RandomState(11 + act + 10 * has_bn + 100 * taps)
    C, N = 4, 3
    lengths = [taps + 2, max(taps - 1, 0), taps, taps + 5]             # one utterance too short for a single output row
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    oo = rt.out_offsets(offsets, taps)
    x, w, b = r.standard_normal((offsets[-1], C)), r.standard_normal((N, taps * C)), r.standard_normal(N)
    gy = r.standard_normal((oo[-1], N))
    bn = [r.uniform(0.5, 1.5, N), r.standard_normal(N), r.standard_normal(N), r.uniform(0.5, 1.5, N)] if has_bn else None
    fwd = rt.forward(x, offsets, taps, w, b, bn, act, 0.2)
    bwd = rt.backward(fwd, gy, 0.2)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)      # noqa: E731
    xt, wt, bt = t(x), t(w), t(b)
    # w [N, taps C] with k = tau C + c -> conv1d's [N, C, taps]
    wc = wt.view(N, taps, C).permute(0, 2, 1)
    gt, bet = (t(bn[0]), t(bn[1])) if has_bn else (None, None)
    zs, ys = [], []
    for i in range(len(lengths)):
        if oo[i + 1] == oo[i]:
            continue
        z = fn.conv1d(xt[offsets[i]:offsets[i + 1]].t()[None], wc, bt)          # [1, N, n_out]
        h = fn.batch_norm(z, torch.tensor(bn[2]), torch.tensor(bn[3]), gt, bet, training=False, eps=1e-3) if has_bn else z
        y = h if act == rt.NONE else (fn.relu(h) if act == rt.RELU else fn.leaky_relu(h, 0.2))
        zs.append(z[0].t())
        ys.append(y[0].t())
    z, y = torch.cat(zs), torch.cat(ys)
    y.backward(torch.tensor(gy))

    def close(got, want, what):
        want = want.detach().numpy()
        assert got.shape == want.shape, what
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), what

    close(fwd["z"], z, "z")
    close(fwd["y"], y, "y")
    close(bwd["gx"], xt.grad, "gx")
    close(bwd["gw"], wt.grad, "gw")
    close(bwd["gbias"], bt.grad, "gbias")
    if has_bn:
        close(bwd["ggamma"], gt.grad, "ggamma")
        close(bwd["gbeta"], bet.grad, "gbeta")
    if taps > 1:
        assert not bwd["gx"][offsets[1]:offsets[2]].any()             # the short utterance: zero rows


def test_one_tap_is_the_dense_layer():
    r = np.random.RandomState(5)
    x, w, b, gy = r.standard_normal((12, 6)), r.standard_normal((5, 6)), r.standard_normal(5), r.standard_normal((12, 5))
    bn = [r.uniform(0.5, 1.5, 5), r.standard_normal(5), r.standard_normal(5), r.uniform(0.5, 1.5, 5)]
    f1, f2 = rt.forward(x, [0, 5, 5, 12], 1, w, b, bn, rt.LRELU), rs.forward(x, w, b, bn, rs.LRELU, rs.SLOPE)
    b1, b2 = rt.backward(f1, gy), rs.backward(f2, gy, rs.SLOPE)
    for k in ("z", "h", "y"):
        assert np.array_equal(f1[k], f2[k]), k
    for k in ("gx", "gw", "gbias", "ggamma", "gbeta"):
        assert np.array_equal(b1[k], b2[k]), k
    e1, e2 = rt.bounds(f1, b1), rs.bounds(f2, b2)
    for k in ("z", "h", "y", "gbias", "ggamma", "gbeta"):
        assert np.array_equal(e1[k], e2[k]), k
    assert np.all(e1["gw"] >= e2["gw"]) and np.all(e1["gx"] >= e2["gx"])          # the split and the padded chain only add


def test_out_offsets():
    from tf_kaldi_speaker_amd import conv_train
    for f in (rt.out_offsets, conv_train.out_offsets):
        assert f([0, 5, 5, 7, 20], 5).tolist() == [0, 1, 1, 1, 10]
        assert f([3, 10], 1).tolist() == [0, 7]
        assert f([4], 7).tolist() == [0]
    assert rt.rows_of([3, 8, 9, 16], 5).tolist() == [3, 9, 10, 11]


@pytest.mark.parametrize("rank", [3, 4])
def test_kernel_layout_round_trip(rank):
    from tf_kaldi_speaker_amd import conv_train
    r = np.random.RandomState(rank)
    W, C, N = 5, 4, 3
    k = r.standard_normal((W, C, N)).astype(np.float32)
    kernel = k if rank == 3 else k[None]
    rows, taps, channels = conv_train.kernel_to_rows(kernel)
    assert rows.shape == (N, W * C) and (taps, channels) == (W, C)
    for tau in range(W):
        for c in range(C):
            assert np.array_equal(rows[:, tau * C + c], k[tau, c, :])
    back = conv_train.rows_to_kernel(rows, kernel.shape)
    assert back.shape == kernel.shape and back.dtype == np.float32 and np.array_equal(back, kernel)
    # and it is the layout of the rule: TensorFlow's VALID convolution of a sequence with this kernel
    x = r.standard_normal((9, C))
    z = rt.forward(x, [0, 9], W, rows, np.zeros(N))["z"]
    want = np.stack([sum(x[t + tau] @ k[tau].astype(np.float64) for tau in range(W)) for t in range(9 - W + 1)])
    assert np.allclose(z, want, rtol=0, atol=1e-12)
    dense = r.standard_normal((C, N)).astype(np.float32)
    rows, taps, channels = conv_train.kernel_to_rows(dense)
    assert (taps, channels) == (1, C) and np.array_equal(rows, dense.T)
    assert np.array_equal(conv_train.rows_to_kernel(rows, dense.shape), dense)
    with pytest.raises(ValueError):
        conv_train.kernel_to_rows(np.zeros((2, 5, 4, 3), dtype=np.float32))


@pytest.mark.parametrize("name", [c[0] for c in tc.CASES])
def test_no_element_of_a_case_sits_on_the_discontinuity(name):
    c = tc.make(name)
    again = tc.make(name)
    assert all(np.array_equal(c[k], again[k]) for k in ("x", "w", "b", "gy"))       # fixed seeds
    zero, exact, far = tc.precondition(c)
    n, N = c["gy"].shape
    print("%s: %d elements zero by construction, %d of exact sign, %d at least 64 bounds from zero" % (name, zero, exact, far))
    assert zero + exact + far == n * N or c["act"] == rs.NONE
    if c["zero_col"] is not None:
        assert zero == n
    if c["family"] == "dyadic" and c["bn"] is None:
        assert np.any(rt.forward(c["x"], c["offsets"], c["taps"], c["w"], c["b"], None, c["act"])["h"] == 0)


def test_the_cases_cover_the_shape_list():
    assert {k[1] for k in tc.CASES} == {1, 5, 7, 9}
    assert {(k[2], k[3]) for k in tc.CASES} == {(30, 8), (23, 72), (8, 130), (68, 64)}
    assert {k[7] for k in tc.CASES} == {"mixed", "short", "one", "long"} and {k[8] for k in tc.CASES} == {"vec", "odd"}
    for W in (1, 5, 9):
        assert [n - (W - 1) for n in tc._lengths(W, "mixed")] == [64, 1, 65, 2, 63]
        assert tc._lengths(W, "short")[2] == max(W - 1, 0) and len(tc._lengths(W, "one")) == 1


@pytest.mark.parametrize("name", ["w1_c30", "w5_c23", "w7_c68", "w9_c8", "w5_long"])
def test_a_float32_evaluation_in_the_stated_orders_lies_within_the_bounds(name):
    c = tc.make(name)
    fwd = rt.forward(c["x"], c["offsets"], c["taps"], c["w"], c["b"], c["bn"], c["act"])
    bwd = rt.backward(fwd, c["gy"])
    bnd = rt.bounds(fwd, bwd)
    got = rt.emulate(c["x"], c["offsets"], c["taps"], c["w"], c["b"], c["bn"], c["act"], c["gy"])
    worst = {}
    for k in ("z", "y", "gx", "gw", "gbias", "ggamma", "gbeta"):
        ref = fwd[k] if k in ("z", "y") else bwd[k]
        if ref is None:
            continue
        err = np.abs(got[k].astype(np.float64) - ref)
        worst[k] = float(np.max(err / (bnd[k] + 1e-300))) if np.any(err > 0) else 0.0
        top = np.max(np.abs(ref))
        # and the bound is no blanket: the worst-case chain bound (K + 2) u sum |x w| grows like K sqrt(K) u against values of
        # order 1, 6e-4 at K = 612; the GPU test caps the error itself at 1e-4 relative L2
        assert top == 0 or np.max(bnd[k]) < 1e-2 * top, (k, np.max(bnd[k]) / top)
    print(name, " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_split_of_is_a_function_of_the_shapes_and_total_out():
    assert rt.split_of(18304, 3584, 512) == (18304, 1)               # tdnn3: the tiles alone fill the device
    rows, s = rt.split_of(19072, 150, 512)                           # tdnn1: 24 tiles
    assert s == 21 and rows % 32 == 0 and rows * s >= 19072 > rows * (s - 1)
    assert rt.split_of(195, 150, 8) == (224, 1)                      # fewer than 256 rows are never cut
    assert rt.split_of(1100, 150, 8) == (224, 5)                     # the `long` case of tconv_cases.py
