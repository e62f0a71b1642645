"""Models, layers and batches of the isolated ResNet convolution tests (tests/test_grid_bars_host.py,
tests/test_gpu_grid_isolated.py).

    r32    width 32: 32 / 64 / 128 / 256 channels, the four precisions.  The smallest width at which stages 3 and 4 are two-unit
           eligible (stride-1 3 x 3, channel counts multiples of 128): one quad of channel blocks reaches only the peeled body of
           gemm_f6v2_kernel<3>, two quads the looped one; stage 2 stays on the three-unit kernel
    r8     width 8, fp32 only: the fp32 kernels with 24-wide taps

both with resnet_blocks [2, 1, 2, 2] (an identity block in both two-unit stages, one stage without), 40-dim features and a
96-wide dense2, in two settings:

    plain     no time stride, no max-pool, PReLU
    ts_max    resnet_time_stride and resnet_maxpooling, leaky ReLU

Batches: the lengths {1, 2, 3, 9, 14, 16, 33, 40} (118 frames) in two pack orders -- the one-frame utterance first; the one-frame
utterance between the two long ones and the two-frame utterance last.  Under time stride they are even and odd at every level
(16 -> 8 -> 4 -> 2, 9 -> 5 -> 3 -> 2, 33 -> 17 -> 9 -> 5, 3 -> 2 -> 1 -> 1, 1 -> 1 -> 1 -> 1); stage 4 then still has 19 frames x 5
bins = 95 GEMM rows, one full 64-row tile and a partial one, and stage 1 without stride 4720.

The per-layer facts restated here from csrc/api_graph.hip build_resnet, csrc/api_weights.hip choose_kernels and csrc/api_plan.hip
chain_two_unit -- which arithmetic, which input exponent, which kernel, which fp6 quantiser -- are asserted against the library by
the GPU test (Trainer.runs_two_unit, the profiler's step names, and the bars themselves)."""
import numpy as np

import ref_grid as rg
import ref_layer as rl

SCOPE = "resnet_18"
BLOCKS = (2, 1, 2, 2)
FEAT_DIM = 40
POOL_NODES = 96
MODELS = {"r32": dict(width=32, precisions=rl.PRECISIONS, seed=31), "r8": dict(width=8, precisions=("f32",), seed=32)}
SETTINGS = {"plain": dict(network_relu_type="prelu"),
            "ts_max": dict(network_relu_type="lrelu", resnet_time_stride=True, resnet_maxpooling=True)}
LENGTHS = (1, 2, 3, 9, 14, 16, 33, 40)
PACK_ORDERS = ((1, 16, 9, 40, 3, 33, 14, 2), (33, 1, 40, 9, 16, 3, 14, 2))
MIN_ROWS = 64 + 1                        # one full 64-row tile plus a partial one


class Conv(object):
    """One GEMM of the graph in front of the pooling: step name (what the profiler reports), variables, geometry, and the nodes
    its input, residual and output are fetched from."""

    def __init__(self, name, kind, kh, kw, cin, cout, st, sw, F_in, level_in, in_node, out_node, bn, act, alpha=None, res_node=None,
                 bias=False, prod_bn=None, prod=None):
        self.name, self.kind, self.kh, self.kw, self.cin, self.cout, self.st, self.sw = name, kind, kh, kw, cin, cout, st, sw
        self.F_in, self.level_in, self.in_node, self.out_node, self.res_node = F_in, level_in, in_node, out_node, res_node
        self.kernel_name = "%s/%s/kernel" % (SCOPE, name)
        self.bias_name = "%s/%s/bias" % (SCOPE, name) if bias else None
        self.bn_scope = "%s/%s" % (SCOPE, bn)
        self.act = act
        self.alpha_name = "%s/%s/alpha" % (SCOPE, alpha) if (alpha and act == "prelu") else None
        self.prod_bn = None if prod_bn is None else "%s/%s" % (SCOPE, prod_bn)      # the normalisation whose exponent the input carries
        self.prod = prod                                                            # the GEMM that wrote the input (None: features)
        self.padding = "valid" if kind == "conv5" else "same"
        self.F_out = 1 if kind in ("conv5", "dense") else -(-F_in // sw)
        self.level_out = level_in + (1 if st == 2 else 0)
        self.ntaps = kh * kw


def params(model, setting, **kw):
    from tf_kaldi_speaker_amd import synth
    return dict(synth.RESNET_PARAMS, num_nodes_pooling_layer=POOL_NODES, resnet_blocks=list(BLOCKS), **dict(SETTINGS[setting], **kw))


def weights(model, setting, **kw):
    from tf_kaldi_speaker_amd import synth
    m = MODELS[model]
    return dict(synth.synth_resnet_weights(params(model, setting, **kw), seed=m["seed"] + (10 if setting == "ts_max" else 0), width=m["width"]))


def layers(model, setting, act=None):
    """Every GEMM up to the pooling, in graph order (csrc/api_graph.hip build_resnet)."""
    width = MODELS[model]["width"]
    s = SETTINGS[setting]
    act = act or s["network_relu_type"]
    ts = 2 if s.get("resnet_time_stride") else 1
    out = [Conv("conv0_1", "conv0", 3, 3, 1, width, 1, 1, FEAT_DIM, 0, None, "conv0_relu", "conv0_bn", act, "conv0_relu")]
    node, bn, prod, F, lvl, cin = "conv0_relu", "conv0_bn", out[0], FEAT_DIM, 0, width
    if s.get("resnet_maxpooling"):
        node = "conv0_max"
    for stage in (1, 2, 3, 4):
        nf, sw = width << (stage - 1), (1 if stage == 1 else 2)
        for bi in range(BLOCKS[stage - 1]):
            b = "conv%da" % stage if bi == 0 else "conv%db_%d" % (stage, bi - 1)
            s_w, s_t = (sw, ts if stage > 1 else 1) if bi == 0 else (1, 1)
            c0 = Conv(b + "_conv0", "conv3x3", 3, 3, cin, nf, s_t, s_w, F, lvl, node, b + "_relu0", b + "_bn0", act, b + "_relu0",
                      prod_bn=bn, prod=prod)
            out.append(c0)
            res = node
            if bi == 0:
                out.append(Conv(b + "_conv_short", "short", 1, 1, cin, nf, s_t, s_w, F, lvl, node, b + "_short", b + "_bn_short", None,
                                prod_bn=bn, prod=prod))
                res = b + "_short"
            F, lvl = c0.F_out, c0.level_out
            c1 = Conv(b + "_conv1", "conv3x3", 3, 3, nf, nf, 1, 1, F, lvl, b + "_relu0", b, b + "_bn1", act, b + "_relu_final", res_node=res,
                      prod_bn=b + "_bn0", prod=c0)
            out.append(c1)
            node, bn, prod, cin = b, b + "_bn1", c1, nf
    c5 = Conv("conv5", "conv5", 1, F, cin, cin, 1, 1, F, lvl, node, "conv5_relu", "conv5_bn", act, "conv5_relu", bias=True, prod_bn=bn, prod=prod)
    d1 = Conv("dense1", "dense", 1, 1, cin, cin, 1, 1, 1, lvl, "conv5_relu", "dense1_relu", "dense1_bn", act, "dense1_relu", bias=True,
              prod_bn="conv5_bn", prod=c5)
    d2 = Conv("dense2", "dense", 1, 1, cin, POOL_NODES, 1, 1, 1, lvl, "dense1_relu", "dense2_relu", "dense2_bn", act, "dense2_relu", bias=True,
              prod_bn="dense1_bn", prod=d1)
    return out + [c5, d1, d2]


def layer(model, setting, name, act=None):
    return [L for L in layers(model, setting, act) if L.name == name][0]


# -------------------------------------------------------------------------------------------------------------- batches
def level_lens(lens, level):
    """Utterance lengths at time level `level`: ceil(L / 2) per stride-2 stage ('same')."""
    lens = [int(n) for n in lens]
    for _ in range(level):
        lens = [-(-n // 2) for n in lens]
    return lens


def batch(order, seed):
    """(features [118, 40], offsets int32, lengths)."""
    from tf_kaldi_speaker_amd import synth
    lens = list(PACK_ORDERS[order])
    assert sorted(lens) == sorted(LENGTHS) and sum(lens) == 118
    feats = np.concatenate(synth.synth_features(len(lens), lens, FEAT_DIM, seed=seed))
    return feats, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), lens


def gemm_rows(L, setting, order):
    """Output bins of layer L = the rows of its compact GEMM; never below one full tile plus a partial one."""
    rows = sum(level_lens(PACK_ORDERS[order], L.level_out)) * L.F_out
    if L.kind != "dense" and L.kind != "conv5":          # (conv5 and the dense layers have one row per frame: 19 under time stride)
        assert rows >= MIN_ROWS, (L.name, setting, rows, "the batch no longer fills a 64-row tile and a partial one")
    return rows


def check_batches():
    """What the batch is for: the two orders as described, even and odd lengths at every level under time stride, utterance
    borders inside 64-row tiles at every stage."""
    a, b = PACK_ORDERS
    assert a[0] == 1 and b[1] == 1 and {b[0], b[2]} == {33, 40} and b[-1] == 2
    for order in PACK_ORDERS:
        for lvl in range(4):
            ls = level_lens(order, lvl)
            assert any(n % 2 == 0 for n in ls) and any(n % 2 == 1 for n in ls), (lvl, ls)
        assert level_lens([16, 9, 33, 3, 1], 3) == [2, 2, 5, 1, 1]
        for lvl, F in ((0, 40), (1, 20), (2, 10), (3, 5)):
            for setting in SETTINGS:
                ls = level_lens(order, lvl if setting == "ts_max" else 0)
                starts = np.cumsum([0] + [n * F for n in ls])[1:-1]
                assert (starts % 64 != 0).any(), (order, setting, lvl, "no utterance border inside a tile")
    assert sum(level_lens(a, 3)) * 5 == 95 and sum(a) * 40 == 4720


# ----------------------------------------------------------------------------------------------- the library's own rules
def use_split(L, precision):
    """choose_kernels: the grid convolutions need whole 32-channel blocks per tap (conv0 goes through its own im2col), the dense
    layers are one-tap frame layers."""
    return precision != "f32" and (L.kind in ("conv0", "dense") or L.cin % 32 == 0)


def two_unit_eligible(L):
    """choose_kernels: the stride-1 3 x 3 convolutions over whole 128-channel tiles."""
    return L.kind == "conv3x3" and L.st == 1 and L.sw == 1 and L.cin % 128 == 0 and L.cout % 128 == 0


def arithmetic(L, precision, two_unit):
    if not use_split(L, precision):
        return "f32"
    if precision == "f16f6":
        return "f16f6" if two_unit else "f16x3"
    return precision


def input_exponent(weights, L, arith):
    """api_weights.hip choose_kernels: a split layer reads its input at the producer's act_exponent -- a block output carries its
    bn1's, the max-pool passes its input's through; conv0 and the fp32 / bf16 paths use 0."""
    if arith not in ("f16x3", "f16f6") or L.kind == "conv0" or L.prod_bn is None:
        return 0
    return rl.act_exponent(weights, L.prod_bn)


def input_quantiser(L, producer_two_unit):
    """api_plan.hip chain_two_unit on the grid: a two-unit convolution reads the block format its producer's epilogue wrote with the
    hardware converters (nearest even) when that producer is another two-unit convolution or a stride-2 3 x 3 of the gathered f16
    kernel; behind a demoted stride-1 convolution f6_from_sb_kernel converts (e2m3_code: half up)."""
    p = L.prod
    if p is not None and p.kind == "conv3x3" and (producer_two_unit or p.st == 2 or p.sw == 2):
        return rl.q6_rne
    return rl.q6_half_up


def expected_kernel(L, precision, two_unit, rows):
    """run_gemm's dispatch (csrc/api_forward.hip; launch_gemm_f32, launch_gemm_bf16x3, launch_gemm_f16f6)."""
    arith = arithmetic(L, precision, two_unit)
    if arith == "f32":
        return "gemm_f32_seg_kernel" if (L.kind == "dense" and rows <= 512) else "gemm_f32_kernel"
    if arith == "f16f6":
        return "gemm_f6v2_kernel<3>"
    return "gemm_bf16x3_w1p3_kernel<gather>" if L.kind in ("conv3x3", "short") else "gemm_bf16x3_w1p3_kernel"


# ------------------------------------------------------------------------------------------------------------ reference
def reference(weights, L, arith, x, in_lens, in_exp=0, kernel=None, quantiser=rl.q6_rne, **gather_kw):
    """Everything a test compares of layer L on its own input x [sum(L_in) F_in, cin] (fp32, packed): the term pairs, the float
    vectors of its epilogue, the output lengths."""
    if L.kind == "conv0":
        x = np.asarray(x, np.float32).reshape(-1, 1)
    idx, out_lens, F_out = rg.gather_windows(in_lens, L.F_in, L.kh, L.kw, L.st, L.sw, L.padding, **gather_kw)
    split = arith != "f32"
    cin_pad = (L.cin + 31) // 32 * 32 if (split and L.kind != "conv0") else None
    k3 = rg.kernel_taps(weights[L.kernel_name] if kernel is None else kernel, cin_pad)
    wts = rl.split_weights(k3, arith)
    xin = rl.pad32(x) if cin_pad else np.asarray(x)
    acts = rl.split_acts(xin, arith, in_exp, quantiser)
    tms = rg.terms(acts, wts, arith, idx, kpad=32 if L.kind == "conv0" else None)
    vec = rg.vectors(weights, L.bn_scope, L.cout, weights[L.bias_name] if L.bias_name else None, wts["ws"], in_exp)
    alpha = weights[L.alpha_name] if L.alpha_name else None
    return dict(arith=arith, terms=tms, vectors=vec, out_lens=out_lens, F_out=F_out, idx=idx, acts=acts, wts=wts, ws=wts["ws"],
                in_exp=in_exp, alpha=alpha)


def checked_elements():
    """The number of elements the GPU bar test compares: N of the Hoeffding bound."""
    n = 0
    for model, m in MODELS.items():
        for setting in SETTINGS:
            for L in layers(model, setting):
                for order in range(len(PACK_ORDERS)):
                    n += sum(level_lens(PACK_ORDERS[order], L.level_out)) * L.F_out * L.cout * len(m["precisions"])
    return n
