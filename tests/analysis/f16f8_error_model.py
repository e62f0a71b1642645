#!/usr/bin/env python
"""Would a cheaper split meet the 1e-4 bar?  numpy emulation (CPU only) of
     a*b ~ f16(a)*f16(b)  +  q8(f16(a))*q8(b - f16(b))  +  q8(a - f16(a))*q8(f16(b))
with q8 = OCP fp8 e4m3 under a power-of-two scale per 32-element K block (what v_mfma_scale_f32_16x16x128_f8f6f4 consumes at twice the
bf16 rate): 1 + 2 x 1/2 = 2 MFMA units per product instead of the 3 of bf16x3 / f16x3.  Run as a script: TDNN x-vector (statistics
pooling), 4 utterances of 300 frames, sums in float64, against the exact float64 forward, every layer in one mode; also prints f16x3
and a one-sided variant for reference.

Importable (tests/test_f6_error_model.py): `q6_blocks` is the e2m3 block quantiser of csrc/xv_f6.h (E8M0 scale = 2^ceil(log2(amax /
7.5)), saturation at 7.5, subnormal steps of 1/8; rounded half up like e2m3_code for the weights, to nearest even like the hardware
converters for the activations), `network` runs the float64 oracle with the layers that the library
puts on the two-unit kernel (`two_unit_eligible`: 5-, 7- and 9-tap convolutions over whole quads of 32-channel blocks) emulated in
a given mode and every other layer in f16x3."""
import contextlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import ref_numpy  # noqa: E402

FORMATS = {'e4m3': dict(mant=3, emin=-6, vmax=448.0), 'e5m2': dict(mant=2, emin=-14, vmax=57344.0),
           'e2m3': dict(mant=3, emin=0, vmax=7.5), 'e3m2': dict(mant=2, emin=-2, vmax=28.0), 'e2m1': dict(mant=1, emin=0, vmax=6.0)}


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def q8_blocks(v, axis, mant=3, emin=-6, vmax=448.0, rne=False):
    """e4m3 (mant=3, emin=-6, max 448) or e5m2 (mant=2, emin=-14, max 57344) with one power-of-two scale per 32 elements along `axis`
    (the smallest that brings the block's largest magnitude to <= vmax).  Magnitudes rounded half up (rne=False: e2m3_code / host_e2m3,
    which quantise the weights) or to nearest even (rne=True: the hardware converters that quantise the activations,
    v_cvt_scalef32_*_fp6_* in csrc/xv_f6.h)."""
    v = np.moveaxis(np.asarray(v, np.float64), axis, -1)
    shp = v.shape
    k = shp[-1]
    pad = (-k) % 32
    if pad:
        v = np.concatenate([v, np.zeros(shp[:-1] + (pad,))], -1)
    b = v.reshape(shp[:-1] + (-1, 32))
    amax = np.abs(b).max(-1, keepdims=True)
    e = np.where(amax > 0, np.ceil(np.log2(np.maximum(amax, 1e-300) / vmax)), 0.0)
    s = 2.0 ** e
    x = b / s
    ax = np.abs(x)
    ex = np.floor(np.log2(np.maximum(ax, 2.0 ** (emin - mant - 2))))
    ex = np.maximum(ex, emin)                       # subnormals share the minimum exponent
    step = 2.0 ** (ex - mant)
    q = np.sign(x) * np.minimum((np.round(ax / step) if rne else np.floor(ax / step + 0.5)) * step, vmax)
    out = (q * s).reshape(shp[:-1] + (-1,))[..., :k]
    return np.moveaxis(out, -1, axis)


def q6_blocks(v, axis, rne=False):
    """fp6 e2m3 under one E8M0 scale per 32 elements along `axis` (the cross-term operands of csrc/gemm_f6v2.hip)."""
    return q8_blocks(v, axis, rne=rne, **FORMATS['e2m3'])


def mm(a, w, mode):
    """a @ w (a [..., K], w [K, N]) in `mode`: 'exact', 'f16x3', 'hi_only' or '<format> ...' (two-unit cross terms in that format)."""
    a = np.asarray(a, np.float32).astype(np.float64)      # activations are fp32 on the GPU
    w = np.asarray(w, np.float32).astype(np.float64)
    if mode == 'exact':
        return a @ w
    ah, wh = f16(a), f16(w)
    al, wl = a - ah, w - wh
    if mode == 'f16x3':
        return ah @ wh + ah @ f16(wl) + f16(al) @ wh
    if mode == 'hi_only':
        return ah @ wh
    fmt = FORMATS[mode.split()[0]]
    A = a.reshape(-1, a.shape[-1])
    ah2, al2 = ah.reshape(A.shape), al.reshape(A.shape)
    # activations through the hardware converters (round to nearest even), weights through the host packer (half up)
    y = (ah2 @ wh + q8_blocks(ah2, 1, rne=True, **fmt) @ q8_blocks(wl, 0, **fmt)
         + q8_blocks(al2, 1, rne=True, **fmt) @ q8_blocks(wh, 0, **fmt))
    return y.reshape(a.shape[:-1] + (w.shape[1],))


def two_unit_eligible(kernel):
    """The layers XV_PREC_F16F6 may run on the two-unit kernel: 5-, 7- and 9-tap convolutions with cin a multiple of 128."""
    k = np.asarray(kernel)
    if k.ndim == 4 and k.shape[0] == 1:
        k = k[0]
    return k.ndim == 3 and k.shape[0] in (5, 7, 9) and k.shape[1] % 128 == 0


@contextlib.contextmanager
def emulated(mode, select=None, other='f16x3'):
    """ref_numpy's convolutions and dense layers computed with mm(): in `mode` for the kernels `select` accepts (all by default),
    in `other` for the rest.  Restores the exact functions on exit."""
    conv0, dense0 = ref_numpy.conv_valid, ref_numpy.dense_layer

    def pick(kernel):
        return mode if select is None or select(kernel) else other

    def conv_emu(x, kernel, bias):
        md = pick(kernel)                                   # (before the float64 copy: `select` may compare buffers)
        kernel = np.asarray(kernel, np.float64)
        k = kernel.shape[1]
        lo = x.shape[1] - k + 1
        y = np.zeros((x.shape[0], lo, kernel.shape[3]))
        for j in range(k):
            y += mm(x[:, j:j + lo, :], kernel[0, j], md)
        return y + np.asarray(bias, np.float64)

    def dense_emu(x, kernel, bias):
        return mm(x, kernel, pick(kernel)) + np.asarray(bias, np.float64)

    ref_numpy.conv_valid, ref_numpy.dense_layer = conv_emu, dense_emu
    try:
        yield
    finally:
        ref_numpy.conv_valid, ref_numpy.dense_layer = conv0, dense0


def network(feats, weights, params, mode='e2m3', demote=()):
    """Endpoints of ref_numpy.entire_network with the two-unit eligible layers in `mode` (except the kernels named in `demote`,
    which run f16x3 like every other layer)."""
    demoted = [weights[n] for n in demote]

    def select(kernel):
        return two_unit_eligible(kernel) and not any(np.shares_memory(kernel, d) for d in demoted)
    with emulated(mode, select):
        return ref_numpy.entire_network(feats, weights, params)[1]


def main():
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.TDNN_STAT_PARAMS)
    weights = synth.synth_weights(params, 30, seed=0)
    feats = np.stack(synth.synth_features(4, 300, 30, seed=1234))
    _, ep = ref_numpy.entire_network(feats, weights, params)
    ref = ep["tdnn6_dense"]
    for mode in ('exact', 'f16x3', 'hi_only', 'e4m3 cross terms', 'e5m2 cross terms', 'e2m3 cross terms (fp6)', 'e3m2 cross terms (fp6)',
                 'e2m1 cross terms (fp4)'):
        with emulated(mode):
            _, e = ref_numpy.entire_network(feats, weights, params)
        err = np.linalg.norm(e["tdnn6_dense"] - ref, axis=1) / np.linalg.norm(ref, axis=1)
        print("%-24s tdnn6_dense rel-L2 max %.3e  mean %.3e" % (mode, err.max(), err.mean()))


if __name__ == "__main__":
    main()
