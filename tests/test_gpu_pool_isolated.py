"""GPU: every pooling path against a float64 pooling of the GPU's own frames, per element.

The pooling's input is an fp32 endpoint of the GPU path (tdnn5_relu, dense2_relu; for attention also the last key layer and
attention_weights), so the reference (tests/helpers/ref_pool.py, numpy) carries no GEMM error and its bars are derived from
fp32 summation, per element and per utterance -- not one relative L2 norm over a vector that the means dominate.  The models
(tests/helpers/pool_cases.py) carry the channel classes a trained checkpoint has and synth.py does not: near-constant, dead,
exactly constant and sparse channels, and attention so peaked that whole 64-row slots carry no weight.

Fused paths never store their input; what the endpoint returns is the same GEMM's accumulators only if both plans schedule
that GEMM alike.  csrc/api_plan.hip (gemm_scratch): the K-split tail is planned for the endpoint's plan but never for a fused
layer of the three-unit kernels, so every trainer here runs with "tail_split" 0; the fp32 kernel takes its one-launch segment
form for a stored output of at most 512 rows but not for pooling partials, so an fp32 batch read through the fused
statistics path always has more than 512 rows.  No bar is widened for either.

The worst error / bar ratio per path and class goes to test_reports/pool_isolated_report.txt (XVEC_REPORT_DIR names
another directory)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_pool as rp                                                            # noqa: E402
import pool_cases as pc                                                          # noqa: E402

pytestmark = pytest.mark.gpu
STD_FLOOR = np.sqrt(np.float32(1e-12))
_report = []
_calibrated = {}


def teardown_module(module):
    out = os.environ.get("XVEC_REPORT_DIR", "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "pool_isolated_report.txt"), "w") as f:
        f.write("# worst error / bar per path and channel class (mean, std); <= 1 passes\n" + "\n".join(_report) + "\n")


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


def _batch(params, out_lens, dim, seed):
    import torch
    make = pc.resnet_batch if params["network_type"] == "resnet_18" else pc.tdnn_batch
    feats, offs, out_offs = make(out_lens, dim, seed)
    return torch.from_numpy(feats).cuda(), offs, out_offs


def _model(key, params, weights, dim):
    """The model with the six channel classes in front of its pooling; the pre-activation statistics are measured once, on
    the GPU (fp32 path, one batch), through a probe batch normalisation."""
    if key not in _calibrated:
        scope = pc.pool_bn_scope(params)
        tr = _trainer(params, pc.probe_weights(weights, scope), dim, "f32")
        feats, offs, _ = _batch(params, pc.PACK_ORDERS[0], dim, 90)
        probe = _run(tr, feats, offs, pc.pool_input_node(params))
        tr.close()
        _calibrated[key] = pc.calibrated(weights, scope, probe)
    return _calibrated[key]


class Worst:
    """Worst mean / std ratio per channel class of one path."""

    def __init__(self, tag):
        self.tag, self.m, self.s = tag, np.zeros(6), np.zeros(6)

    def add(self, rm, rs, cls):
        for c in range(6):
            if (cls == c).any():
                self.m[c] = max(self.m[c], rm[cls == c].max())
                self.s[c] = max(self.s[c], rs[cls == c].max())

    def close(self):
        for c in range(6):
            _report.append("%-58s %-20s mean %.3e  std %.3e" % (self.tag, pc.CLASS_NAMES[c], self.m[c], self.s[c]))


def _assert_bars(rm, rs, what):
    bad = np.flatnonzero((rm > 1) | (rs > 1))
    assert bad.size == 0, (what, "elements", bad[:8].tolist(), "mean ratio", rm[bad[:8]].tolist(), "std ratio", rs[bad[:8]].tolist())


# ------------------------------------------------------------------------------------------------------- statistics
def _statistics(key, params, weights, dim, precision, with_long, relu=True, ws_strict=True):
    weights = _model(key, params, weights, dim)
    node = pc.pool_input_node(params)
    tr = _trainer(params, weights, dim, precision)
    batches = [_batch(params, order, dim, 91 + i) for i, order in enumerate(pc.PACK_ORDERS)]
    if with_long:
        batches.append(_batch(params, pc.LONG, dim, 95))
    pooled, ws, identical = {}, {}, {1: 0, 0: 0}
    for fusion in (1, 0):
        tr.set_option("pool_fusion", fusion)
        worst = Worst("%s %s %s" % (key, precision, "fused" if fusion else "stat_pool_kernel"))
        for bi, (feats, offs, out_offs) in enumerate(batches):
            ws[fusion, bi] = tr.plan_info(offs, "pooling")["workspace_bytes"]
            x = _run(tr, feats, offs, node)
            got = _run(tr, feats, offs, "pooling")
            assert np.array_equal(got, _run(tr, feats, offs, "pooling"), equal_nan=True), "not deterministic"
            assert x.shape[0] == out_offs[-1] and got.shape == (len(offs) - 1, 2 * x.shape[1])
            pooled[fusion, bi] = got
            C = x.shape[1]
            cls = pc.class_of(C)
            for b in range(len(offs) - 1):
                r0, r1 = int(out_offs[b]), int(out_offs[b + 1])
                rm, rs = rp.stat_check(x[r0:r1], r0, got[b, :C], got[b, C:])
                worst.add(rm, rs, cls)
                _assert_bars(rm, rs, (key, precision, fusion, bi, b, r1 - r0))
                if relu:                          # a dead channel: mean exactly 0, std exactly sqrtf(1e-12f)
                    assert (x[r0:r1][:, cls == 3] == 0).all()
                    assert (got[b, :C][cls == 3] == 0).all() and (got[b, C:][cls == 3] == STD_FLOOR).all()
                assert (got[b, C:][cls == 4] == STD_FLOOR).all()
                # alone in the batch: the same bits whenever the frames are the same bits and the 64-row slots fall alike
                n = r1 - r0
                if n not in (1, 65, 300, 12000) or (fusion and precision == "f32" and n <= 512):
                    continue
                f1, o1 = feats[int(offs[b]):int(offs[b + 1])].contiguous(), np.array([0, offs[b + 1] - offs[b]], dtype=np.int32)
                xa, ga = _run(tr, f1, o1, node), _run(tr, f1, o1, "pooling")
                rm, rs = rp.stat_check(xa, 0, ga[0, :C], ga[0, C:])
                _assert_bars(rm, rs, (key, precision, fusion, bi, b, "alone"))
                if np.array_equal(xa, x[r0:r1]) and (not fusion or r0 % 64 == 0):
                    assert np.array_equal(ga[0], got[b]), (key, precision, fusion, bi, b, "alone")
                    identical[fusion] += 1
        worst.close()
    tr.close()
    for bi in range(len(batches)):                # which path ran: the unfused plan stores the frames, and sums in another order
        assert ws[0, bi] > ws[1, bi] or (not ws_strict and ws[0, bi] == ws[1, bi]), (ws, bi)
        assert not np.array_equal(pooled[1, bi], pooled[0, bi])
    if with_long:
        assert identical[1] > 0 and identical[0] > 0, identical


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x3", "f16f6"])
def test_statistics_pooling_narrow(precision):
    """Fused epilogue (each precision's kernel family has its own) and stat_pool_kernel<true>, ragged batches in both pack
    orders and the 12 000-frame utterance beside the shortest legal one."""
    params, weights, dim = pc.stat_model("narrow")
    _statistics("narrow", params, weights, dim, precision, with_long=True)


def test_statistics_pooling_narrow_prelu():
    params, weights, dim = pc.stat_model("narrow_prelu")
    _statistics("narrow_prelu", params, weights, dim, "bf16x3", with_long=False, relu=False)


@pytest.mark.parametrize("precision", ["bf16x3", "f16f6"])
def test_statistics_pooling_full_width(precision):
    """1500 channels: the epilogue's lane map over many 32-channel blocks, 1500 = 46 x 32 + 28."""
    params, weights, dim = pc.stat_model("full")
    _statistics("full", params, weights, dim, precision, with_long=False)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_statistics_pooling_resnet(precision):
    """dense2_relu -> OP_STAT_POOL under resnet_time_stride: the same fusion rule on the ResNet's time level.  The grid
    layers set the size of the ResNet's workspace, so storing the [rows, 96] frames does not show there: the unfused plan
    must not be smaller, and the bits differ."""
    params, weights, dim = pc.resnet_model()
    _statistics("resnet18_w32", params, weights, dim, precision, with_long=False, ws_strict=False)


# -------------------------------------------------------------------------------------------------------- attention
def _zero_slots(w32, r0):
    z, i = 0, 0
    for _, ni in rp._segments(r0, w32.shape[0]):
        z += int((w32[i:i + ni].sum(axis=0, dtype=np.float32) == 0).any())
        i += ni
    return z


def _attention(name, precision, regime):
    import torch
    params, weights, dim = pc.att_model(name, regime)
    weights = dict(_model("att_" + name, params, weights, dim))    # the query does not reach tdnn5: one calibration per layout
    weights["tdnn/attention/query"] = pc.att_model(name, regime)[1]["tdnn/attention/query"]
    H, split_v, split_k = int(params["att_num_heads"]), bool(params["att_split_value"]), bool(params["att_split_key"])
    query = weights["tdnn/attention/query"]
    knode, out = pc.key_node(params), "att_output_before_nonlinear"
    tr = _trainer(params, weights, dim, precision)
    utts = {n: pc.features([n + 14], dim, seed=300 + i)[0] for i, n in enumerate(pc.LENGTHS + pc.LONG[:1])}
    pooled, ws, zero_slots = {}, {}, 0
    for fusion in (1, 0):
        tr.set_option("att_fusion", fusion)
        path = "fused" if fusion and precision != "f32" else "att_pool_kernel"
        worst = Worst("att_%s %s %s att_fusion=%d %s" % (name, precision, regime, fusion, path))
        worst_w, alone = 0.0, {}
        # uniform batches (one utterance, and three of 65 frames): attention_weights against the stored key
        # (fp32: the utterance is repeated until the batch has more than 512 rows, so that its key layer runs on the kernel
        # that the ragged batches below get, not on the one-launch segment form -- the key must be the same bits)
        reps = {n: 512 // n + 1 if precision == "f32" else 1 for n in utts}
        cases = [(n, [utts[n]] * reps[n]) for n in utts] + [(65, [utts[65], utts[127], utts[128]] * reps[65])]
        for n, group in cases:
            group = [g[:n + 14] for g in group]
            feats = torch.from_numpy(np.concatenate(group)).cuda()
            offs = (np.arange(len(group) + 1) * (n + 14)).astype(np.int32)
            key = _run(tr, feats, offs, knode)
            value = _run(tr, feats, offs, "tdnn5_relu")
            w = _run(tr, feats, offs, "attention_weights").reshape(len(group), H, n)
            got = _run(tr, feats, offs, out)
            assert np.array_equal(got, _run(tr, feats, offs, out), equal_nan=True), "not deterministic"    # (a NaN is for the bars)
            scale = pc.att_scale(params, key.shape[1])
            for b in range(len(group)):
                kb, vb, wb = key[b * n:(b + 1) * n], value[b * n:(b + 1) * n], w[b].T.copy()
                ref = rp.softmax_weights(kb, query, scale, H, split_k)
                rw = rp.weight_ratio(wb, ref, rp.weight_bar(n, rp.score_bar(kb, query, scale, H, split_k)))
                worst_w = max(worst_w, rw.max())
                assert (rw <= 1).all(), (name, precision, regime, fusion, n, b, rw.max())
                if n >= 300 and regime == "peaked":      # a whole slot without weight: the w > 0 branch of att_pool_finalize_kernel
                    assert _zero_slots(ref.astype(np.float32), 0) > 0, (name, n, "no 64-row slot with weight sum 0")
                    zero_slots += 1
                odim = got.shape[1] // 2
                rm, rs = rp.att_check(vb, wb, split_v, 0, got[b, :odim], got[b, odim:])
                cls = pc.class_of(vb.shape[1]) if split_v else np.tile(pc.class_of(vb.shape[1]), H)
                worst.add(rm, rs, cls)
                _assert_bars(rm, rs, (name, precision, regime, fusion, n, b, "uniform"))
                assert (got[b, :odim][cls == 3] == 0).all() and (got[b, odim:][cls == 3] == STD_FLOOR).all()
                if n == 1:                        # one frame: weight exactly 1, mean = the frame, std at the floor
                    assert (wb == 1).all() and (got[b, odim:] == STD_FLOOR).all()
                    assert np.array_equal(got[b, :odim], vb[0] if split_v else np.tile(vb[0], H))
                if b == 0 and n not in alone:
                    alone[n] = (vb, wb, got[0], kb)
        # ragged batches for the pooled output, with the weights each utterance showed on its own
        for bi, order in enumerate(pc.PACK_ORDERS + (pc.LONG,)):
            feats = torch.from_numpy(np.concatenate([utts[n] for n in order])).cuda()
            offs = np.concatenate([[0], np.cumsum([n + 14 for n in order])]).astype(np.int32)
            ws[fusion, bi] = tr.plan_info(offs, out)["workspace_bytes"]
            value, got, key = _run(tr, feats, offs, "tdnn5_relu"), _run(tr, feats, offs, out), _run(tr, feats, offs, knode)
            pooled[fusion, bi] = got
            odim, r0 = got.shape[1] // 2, 0
            for b, n in enumerate(order):
                vb, (va, wb, ga, ka) = value[r0:r0 + n], alone[n]
                # the weights are this batch's only if the key is: peaked scores turn a last-bit difference into percents
                assert np.array_equal(ka, key[r0:r0 + n]), (name, precision, fusion, bi, b, "the key differs from the uniform batch's")
                rm, rs = rp.att_check(vb, wb, split_v, r0, got[b, :odim], got[b, odim:])
                cls = pc.class_of(vb.shape[1]) if split_v else np.tile(pc.class_of(vb.shape[1]), H)
                worst.add(rm, rs, cls)
                _assert_bars(rm, rs, (name, precision, regime, fusion, bi, b, n))
                if np.array_equal(va, vb) and (path != "fused" or r0 % 64 == 0):
                    assert np.array_equal(ga, got[b]), (name, precision, regime, fusion, bi, b, "alone")
                r0 += n
        worst.close()
        _report.append("%-58s %-20s weights %.3e" % (worst.tag, "attention_weights", worst_w))
    tr.close()
    assert zero_slots > 0 or regime != "peaked"
    for bi in range(3):
        if precision == "f32":                   # fp32 layers have no attention epilogue: the option changes nothing
            assert np.array_equal(pooled[1, bi], pooled[0, bi])
        else:
            assert ws[0, bi] > ws[1, bi], (ws, bi)
            if regime == "moderate":             # (a one-hot weight vector leaves nothing to sum in another order)
                assert not np.array_equal(pooled[1, bi], pooled[0, bi])


@pytest.mark.parametrize("regime", ["moderate", "peaked"])
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", sorted(pc.ATT_MODELS))
def test_attentive_pooling(name, precision, regime):
    """att_scores / att_softmax / att_pool kernels and the fused form (score partials in the key layer's epilogue, weighted
    moments in the value layer's, att_pool_finalize_kernel), one head, three heads unsplit, two heads split: the weights
    against the stored key, the pooled output against the GPU's own weights and value."""
    _attention(name, precision, regime)
