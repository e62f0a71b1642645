"""GPU: every TDNN / extended-TDNN layer GEMM against a float64 model of the same product on the GPU's own input, per element.

Layer L's input x is an fp32 endpoint of the GPU path (the '_relu' endpoint of layer L - 1, the features, or 'pooling'), so the
reference (tests/helpers/ref_layer.py, numpy) carries no error of the layers in front: it splits x and the weights by the
library's own rules into the exactly representable operands the kernel multiplies, sums their products in float64, and what is
left between it and the '_conv' / '_dense', '_bn' and '_relu' endpoints of L is the rounding of one fp32 accumulation -- held per
element to lambda u sqrt(sum S_i^2) (Hoeffding; lambda from the number of elements this file checks, p = 1e-6; the host file
tests/test_layer_bars_host.py shows that fp32 emulations stay inside and which faults leave).  Not one relative L2 norm over a
tensor: that bar (1e-4) sits 10 to 1000 times above the measured error.

The fused run never stores x; the endpoint of L - 1 returns the same accumulators only if both plans schedule that GEMM alike,
so every trainer runs with "tail_split" 0 (see tests/test_gpu_pool_isolated.py).  The profiler reports a plan's steps by layer
('tdnn3_conv'); which kernel a step launches follows from the dispatch rules restated in layer_cases.expected_kernel and from
Trainer.runs_two_unit, and both are asserted per case.

Exact selection: weights with one non-zero entry per output channel make every accumulator a sum of at most three exactly
representable products, and the '_conv' / '_dense' endpoint must equal the host prediction bit for bit -- every (tap, 32-channel
block) pair and every position of a block, both pack orders, four precisions.  In f16f6 that compares the hardware fp6
converters (rounding, scale rule, code order) with what csrc/xv_f6.h says of them.

The worst error / bar per kernel, model, precision, regime and output channel class goes to
test_reports/layer_isolated_report.txt (XVEC_REPORT_DIR names another directory), the relative L2 against the exact float64
product of the same x beside it (documentation only)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_layer as rl                                                           # noqa: E402
import layer_cases as lc                                                         # noqa: E402
import pool_cases as pc                                                          # noqa: E402

pytestmark = pytest.mark.gpu
LAM = rl.hoeffding_lambda(lc.checked_elements())
_models, _weights, _trainers, _worst = {}, {}, {}, {}


def teardown_module(module):
    for tr in _trainers.values():
        tr.close()
    _trainers.clear()
    out = os.environ.get("XVEC_REPORT_DIR", "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "layer_isolated_report.txt"), "w") as f:
        f.write("# worst error / bar (<= 1 passes; lambda %.3f) and worst relative L2 against the exact product of the same input,\n"
                "# per kernel, model, precision, regime and output channel class; demoted = xv_finalize took the two-unit layer back\n" % LAM)
        for key in sorted(_worst):
            ratio, l2, demoted = _worst[key]
            f.write("%-28s %-6s %-7s %-8s %-20s ratio %.3e  rel_l2 %.3e%s\n" % (key + (ratio, l2, "  demoted" if demoted else "")))


def _trainer(params, weights, dim, precision):
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    tr = Trainer(Params(**dict(params)), None, dim, single_cpu=True, device=0, precision=precision)
    tr.build("predict")
    tr.load_weights(weights)
    tr.set_option("tail_split", 0)
    return tr


def _run(tr, feats, offs, node):
    return tr.predict_packed(feats, offs, node).cpu().numpy()


def _model(name):
    if name not in _models:
        _models[name] = lc.model(name)
    return _models[name]


def _regime_weights(name, regime):
    """The model's weights; "classes": the six channel classes in every normalisation with a reader, measured layer by layer on
    the fp32 path."""
    import torch
    if (name, regime) not in _weights:
        params, weights, dim, _ = _model(name)
        if regime == "classes":
            def measure(w, node, feats, offs):
                tr = _trainer(params, w, dim, "f32")
                z = _run(tr, torch.from_numpy(feats).cuda(), offs, node)
                tr.close()
                return z
            weights = lc.calibrated(name, weights, measure)
        _weights[name, regime] = weights
    return _weights[name, regime]


def _case_trainer(name, precision, regime):
    key = (name, precision, regime)
    if key not in _trainers:
        params, _, dim, _ = _model(name)
        _trainers[key] = _trainer(params, _regime_weights(name, regime), dim, precision)
    return _trainers[key]


def _input(tr, name, L, feats, feats_dev, offs):
    """(x [rows, cin] fp32 as the GPU has it, the offsets of its rows)."""
    node = lc.input_node(name, L)
    if node is None:
        return feats, np.asarray(offs, dtype=np.int64)
    x = _run(tr, feats_dev, offs, node)
    if node == "pooling":
        return x, np.array([0, x.shape[0]])
    p = lc.producer(name, L)
    return x, (lc.layer_offsets(offs, p.ctx) if L.frame_level else np.array([0, x.shape[0]]))


def _sum_sq_on_device(tms):
    """ref_layer.sum_sq_partials on float64 device tensors: the same expression, rows x N x K squares without the host's minutes."""
    import torch
    dev = [(torch.from_numpy(np.ascontiguousarray(A)).cuda(), torch.from_numpy(np.ascontiguousarray(W)).cuda()) for A, W in tms]
    return rl.sum_sq_partials(dev).cpu().numpy()


def _note(kernel, name, precision, regime, cout, ratio, l2, demoted):
    cls = pc.class_of(cout)
    for c in range(6):
        key = (kernel, name, precision, regime, pc.CLASS_NAMES[c])
        old = _worst.get(key, (0.0, 0.0, False))
        _worst[key] = (max(old[0], float(ratio[:, cls == c].max())), max(old[1], l2), old[2] or demoted)


CASES = [(name, L.index) for name in sorted(lc.MODELS) for L in lc.tested_layers(name)]


@pytest.mark.parametrize("regime", lc.REGIMES)
@pytest.mark.parametrize("precision", rl.PRECISIONS)
@pytest.mark.parametrize("name,index", CASES)
def test_layer_bars(name, index, precision, regime):
    import torch
    L = [x for x in lc.layers(name) if x.index == index][0]
    weights = _regime_weights(name, regime)
    tr = _case_trainer(name, precision, regime)
    two_unit = precision == "f16f6" and tr.runs_two_unit(L.affine)
    eligible = precision == "f16f6" and lc.two_unit_eligible(L)
    if regime == "plain":
        assert two_unit == eligible, (name, L.affine, "the plain model's 5/7/9-tap layers run on the two-unit kernel")
    assert not two_unit or eligible
    for order in lc.orders(L):
        feats, offs = lc.batch(name, L, order, 80 + order)
        feats_dev = torch.from_numpy(feats).cuda()
        x, x_offs = _input(tr, name, L, feats, feats_dev, offs)
        prod = lc.producer(name, L)
        if regime == "classes" and prod is not None:
            assert (x[:, pc.class_of(x.shape[1]) == 3] == 0).all(), "a dead input channel is not exactly zero"
        tr.profile_begin()
        got = {"bn": _run(tr, feats_dev, offs, L.endpoint("bn"))}
        recs, _ = tr.profile_end()
        assert L.affine in [r["name"] for r in recs], (L.affine, [r["name"] for r in recs])
        got["affine"] = _run(tr, feats_dev, offs, L.endpoint("affine"))
        got["relu"] = _run(tr, feats_dev, offs, L.endpoint("relu"))
        for st, g in got.items():
            assert np.array_equal(g, _run(tr, feats_dev, offs, L.endpoint(st)), equal_nan=True), (st, "not deterministic")
        kernel = lc.expected_kernel(L, precision, two_unit, got["bn"].shape[0])
        ref = lc.reference(weights, name, L, precision, two_unit, x, x_offs)
        assert got["bn"].shape == (ref["out_offsets"][-1], L.cout)
        acc = rl.model_acc(ref["terms"])
        bacc = rl.bar_acc(_sum_sq_on_device(ref["terms"]), LAM)
        exact = lc.reference(weights, name, L, "f32", False, x, x_offs)
        want = rl.model_acc(exact["terms"]) + exact["vectors"]["affine"][1].astype(np.float64)
        l2 = float(np.linalg.norm(got["affine"] - want) / max(np.linalg.norm(want), 1e-300))
        worst = np.zeros(acc.shape)
        for st, vec, act in (("affine", "affine", None), ("bn", "bn", None), ("relu", "bn", "relu")):
            sc, sh = ref["vectors"][vec]
            val, pre = rl.stage(acc, sc, sh, act)
            bar = rl.stage_bar(bacc, sc, pre, act)
            err = np.abs(got[st].astype(np.float64) - val)
            ratio = np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0)
            worst = np.maximum(worst, ratio)
            print("%s %s %s %s %s order %d %s: worst error / bar %.3f, rel L2 %.2e" % (name, L.affine, precision, regime, kernel, order, st,
                                                                                     ratio.max(), l2))
        _note(kernel, name, precision, regime, L.cout, worst, l2, eligible and not two_unit)
        bad = np.argwhere(worst > 1)
        assert bad.shape[0] == 0, (name, L.affine, precision, regime, kernel, order, "elements outside the bar", bad.shape[0],
                                   bad[:8].tolist(), worst[worst > 1][:8].tolist())


# ------------------------------------------------------------------------------------------------------ exact selection
SELECT = [("c128", i) for i in (1, 2, 3, 4, 5)] + [("c256", 2), ("c256", 3)] + [("e128", i) for i in range(1, 11)]


@pytest.mark.parametrize("value", [1.0, 1.0 + 2.0 ** -12])
@pytest.mark.parametrize("precision", rl.PRECISIONS)
@pytest.mark.parametrize("name,index", SELECT)
def test_exact_selection(name, index, precision, value):
    """w_lo = 0 for the value 1; 1 + 2^-12 makes w_lo one fp6-exact value, so that q6(a_hi) shows in the result."""
    import torch
    params, weights, dim, layers = _model(name)
    L = [x for x in layers if x.index == index][0]
    k, used = rl.selection_kernel(L.w, L.cin, L.cout, value)
    nb = (L.cin + 31) // 32
    assert {(t, b) for t, b, _ in used} == {(t, b) for t in range(L.w) for b in range(nb)}
    assert {p for _, _, p in used} == set(range(min(32, L.cin)))
    weights = dict(weights)
    weights[L.kernel_name] = k.reshape(weights[L.kernel_name].shape)
    weights[L.bias_name] = np.zeros(L.cout, dtype=np.float32)
    tr = _trainer(params, weights, dim, precision)
    try:
        two_unit = precision == "f16f6" and tr.runs_two_unit(L.affine)
        assert two_unit == (precision == "f16f6" and lc.two_unit_eligible(L))
        arith = rl.arithmetic(precision, True, two_unit)
        for order in (0, 1):
            feats, offs = lc.batch(name, L, order, 60 + order)
            feats_dev = torch.from_numpy(feats).cuda()
            x, x_offs = _input(tr, name, L, feats, feats_dev, offs)
            got = _run(tr, feats_dev, offs, L.affine)
            ref = lc.reference(weights, name, L, precision, two_unit, x, x_offs)
            # the three-unit kernels add a_lo w_hi, a_hi w_lo, a_hi w_hi in this order (csrc/gemm_bf16x3.hip); the two-unit kernel's
            # three instructions are interleaved over taps and blocks: any order of the three additions
            pred = rl.selection_predictions(ref["terms"], orders="any" if arith == "f16f6" else None, exact_products=arith != "f32")
            inv = ref["vectors"]["affine"][0].astype(np.float64)
            pred = (pred.astype(np.float64) * inv).astype(np.float32)          # fmaf(acc, 2^-k, 0): exact
            hit = (pred == got[None]).any(axis=0)
            miss = np.argwhere(~hit)
            assert miss.shape[0] == 0, (name, L.affine, precision, value, order, "elements that differ", miss.shape[0], miss[:6].tolist(),
                                        [(float(got[i, j]), pred[:, i, j].tolist(), used[j]) for i, j in miss[:6]])
            if arith == "f16f6" and value != 1.0:
                # the check decides the converters' rounding rule: round-half-up codes (e2m3_code) predict other bits somewhere
                up = lc.reference(weights, name, L, precision, True, x, x_offs, quantiser=rl.q6_half_up)
                pred_up = (rl.selection_predictions(up["terms"], orders="any").astype(np.float64) * inv).astype(np.float32)
                assert not (pred_up == got[None]).any(axis=0).all(), (name, L.affine, order, "no tie among the activations of this batch")
    finally:
        tr.close()
