#!/usr/bin/env python
"""Generate tests/golden/loss_*.npz by running the REFERENCE's own numpy twins of its loss heads in the build container
(never on the GPU box, never at test time):

  /root/reference/model/test_utils.py   compute_asoftmax (:157-226), compute_amsoftmax (:229-270), compute_arcsoftmax (:273-318)

Only inputs, parameters and the returned loss (data) are stored; no reference source travels.

The twins compute -log(p + 1e-16) and add 1e-16 under the norms, TensorFlow (and tests/helpers/ref_loss.py, and the kernel) a
log-sum-exp with max(norm, 1e-12); the two agree to better than 1e-9 while every target probability exceeds 1e-6 and every
target |cos| stays below 0.999.  That is a condition on the inputs and is asserted here for every stored case.
usage: python tests/golden/make_loss_golden.py   (needs /root/reference)
"""
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
from model import test_utils as ref_tu            # noqa: E402

E, C = 16, 11


class P(object):
    pass


def rows_with_cosines(rs, w, labels, cosines, norms):
    """Rows whose cosine to their target column of w is the given one: c w^ + sqrt(1 - c^2) (a unit vector orthogonal to w^)."""
    x = np.zeros((len(labels), w.shape[0]))
    for i, (lab, c, r) in enumerate(zip(labels, cosines, norms)):
        wh = w[:, lab] / np.linalg.norm(w[:, lab])
        v = rs.standard_normal(w.shape[0])
        v -= np.dot(v, wh) * wh
        v /= np.linalg.norm(v)
        x[i] = r * (c * wh + np.sqrt(1.0 - c * c) * v)
    return x


def case(name, twin, prefix, seed, m, cosines, step, feature_norm=False, s=1.0, lam=(0.0, 10.0, 0.5, 1.0), norms=(2.0, 4.0)):
    rs = np.random.RandomState(seed)
    w = rs.standard_normal((E, C))
    n = len(cosines)
    labels = np.array([0, C - 1] + list(rs.randint(0, C, n - 2)), dtype=np.int32)
    x = rows_with_cosines(rs, w, labels, cosines, rs.uniform(norms[0], norms[1], n))
    p = P()
    p.feature_norm = feature_norm
    p.feature_scaling_factor = s
    p.global_step = step
    setattr(p, prefix + "_m", m)
    for k, v in zip(("lambda_min", "lambda_base", "lambda_gamma", "lambda_power"), lam):
        setattr(p, "%s_%s" % (prefix, k), v)
    loss = float(twin(x.copy(), labels.copy(), p, w.copy()))
    # the conditions under which -log(p + 1e-16) with 1e-16 under the norms equals the log-sum-exp form to 1e-9
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
    import ref_loss
    head = {"asoftmax": "asoftmax", "amsoftmax": "additive_margin_softmax", "arcsoftmax": "additive_angular_margin_softmax"}[prefix]
    fa = ref_loss.annealing_fa(lam[0], lam[1], lam[2], lam[3], step)
    xin = ref_loss.l2_scaling(x, s) if feature_norm else x
    r = ref_loss.classifier_loss(xin, labels, w, None, head, m, fa)
    wh = w / np.linalg.norm(w, axis=0, keepdims=True)
    cos_t = np.sum(x * wh[:, labels].T, axis=1) / np.linalg.norm(x, axis=1)
    assert np.all(np.exp(-r["loss"]) > 1e-6), (name, np.exp(-r["loss"]).min())
    assert np.all(np.abs(cos_t) < 0.999), (name, np.abs(cos_t).max())
    assert 0.0 < fa < 1.0 or (prefix == "asoftmax" and m == 1), (name, fa)
    assert abs(r["loss"].mean() - loss) < 1e-9, (name, r["loss"].mean(), loss)
    np.savez(os.path.join(HERE, "loss_%s.npz" % name), x=x, labels=labels, kernel=w, head=np.array(head), margin=np.float64(m),
             lambda_min=lam[0], lambda_base=lam[1], lambda_gamma=lam[2], lambda_power=lam[3], global_step=np.int64(step),
             feature_norm=np.int64(feature_norm), feature_scaling_factor=np.float64(s), loss=np.float64(loss))
    return cos_t


def main():
    spread = [0.9, 0.4, -0.3, -0.85, 0.75, 0.2, -0.5, -0.9]          # two target cosines in each quadrant k of test_utils.py:207-216
    mild = [0.8, 0.5, 0.1, -0.2, 0.95, 0.6, -0.6]
    case("asoftmax_m1", ref_tu.compute_asoftmax, "asoftmax", 11, 1, mild, 0)
    case("asoftmax_m2", ref_tu.compute_asoftmax, "asoftmax", 12, 2, spread, 30, norms=(1.0, 2.0))
    cos4 = case("asoftmax_m4", ref_tu.compute_asoftmax, "asoftmax", 13, 4, spread, 200, norms=(0.5, 1.0))
    quad = set()
    for c in cos4:
        l2 = 2.0 * c * c - 1.0
        quad.add(0 if c > 0 and l2 > 0 else 1 if c > 0 and l2 < 0 else 2 if c < 0 and l2 < 0 else 3)
    assert quad == {0, 1, 2, 3}, quad
    case("amsoftmax_m0", ref_tu.compute_amsoftmax, "amsoftmax", 14, 0.0, mild, 30)
    case("amsoftmax_m02", ref_tu.compute_amsoftmax, "amsoftmax", 15, 0.2, mild, 200)
    case("arcsoftmax_m0", ref_tu.compute_arcsoftmax, "arcsoftmax", 16, 0.0, mild, 30)
    cos_a = case("arcsoftmax_m03", ref_tu.compute_arcsoftmax, "arcsoftmax", 17, 0.3, [0.8, -0.97, 0.3, -0.99, 0.0, -0.9, 0.97], 200)
    over = np.arccos(cos_a) + 0.3 > np.pi
    assert over.any() and (~over).any(), cos_a                        # both sides of the theta + m > pi branch
    case("amsoftmax_norm", ref_tu.compute_amsoftmax, "amsoftmax", 18, 0.2, [0.9, 0.8, 0.7, 0.85, 0.95, 0.65, 0.75], 30, feature_norm=True, s=20.0)
    print("loss fixtures written to", HERE)


if __name__ == "__main__":
    main()
