#!/usr/bin/env python
"""Generate tests/golden/metric_*.npz by running the REFERENCE's own float64 numpy twins of its metric-learning losses in the
build container (never on the GPU box, never at test time):

  /root/reference/model/test_utils.py   compute_triplet_loss (:118-154), asoftmax_ / amsoftmax_ / arcsoftmax_angular_triplet_loss
                                        (:694-857), compute_ge2e_loss (:21-86)

Only inputs, options and the returned loss (data) are stored; no reference source travels.  The rows are stored as float32, the
type the kernels read, and the twins get exactly those values in float64.

The twins add 1e-16 under their norms and inside their logarithms and compare with `>` in their own order of operations; they
and the rules of include/xvec_hip.h (tests/helpers/ref_metric_loss.py) coincide to 1e-12 while no comparison is close to a tie.
That is a condition on the inputs and is asserted here for every stored case:
  every |d(i, k) - d(i, j)| and every |t| of a valid triplet exceeds 1e-6, every ge2e target probability exceeds 1e-6,
  every off-diagonal |cos| stays below 0.999, and the float64 oracle agrees with the twin to 1e-12.
usage: python tests/golden/make_metric_loss_golden.py   (needs /root/reference)
"""
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
from model import test_utils as ref_tu            # noqa: E402
import ref_metric_loss as ref                     # noqa: E402

TWINS = {"asoftmax": ref_tu.asoftmax_angular_triplet_loss, "additive_margin_softmax": ref_tu.amsoftmax_angular_triplet_loss,
         "additive_angular_margin_softmax": ref_tu.arcsoftmax_angular_triplet_loss}
SHORT = {"asoftmax": "asoftmax", "additive_margin_softmax": "amsoftmax", "additive_angular_margin_softmax": "arcsoftmax"}


def inputs():
    rs = np.random.RandomState(5)
    labels = np.repeat(np.arange(6) * 7 + 3, 4)
    perm = rs.permutation(24)
    spk = rs.standard_normal((6, 16))
    x = spk[np.repeat(np.arange(6), 4)] * 0.8 + rs.standard_normal((24, 16))
    return x.astype(np.float32), labels.astype(np.int32), perm


def main():
    x, labels, perm = inputs()
    cases = [("semihard_sq%d" % sq, "semihard", dict(margin=0.2, squared=bool(sq), normalize=True)) for sq in (0, 1)]
    for head, m in (("asoftmax", 1), ("asoftmax", 2), ("asoftmax", 4), ("additive_margin_softmax", 0.2),
                    ("additive_angular_margin_softmax", 0.3)):
        for tt in ("all", "hard"):
            cases.append(("%s_%s_m%s" % (tt, SHORT[head], str(m).replace(".", "")), tt, dict(loss_type=head, margin=m)))
    for gt in ("softmax", "contrastive"):
        for w, b in ((20.0, 0.0), (10.0, -5.0)):
            cases.append(("ge2e_%s_w%d" % (gt, int(w)), gt, dict(w=w, b=b)))
    worst, stats = 0.0, dict(gap=np.inf, t=np.inf, prob=np.inf, cos=0.0)
    for order, idx in (("major", np.arange(24)), ("perm", perm)):
        xo, lo = x[idx], labels[idx]
        x64 = xo.astype(np.float64)
        for name, kind, o in cases:
            if kind == "semihard":
                twin = ref_tu.compute_triplet_loss(x64.copy(), lo.copy(), o["margin"], o["squared"])
            elif kind in ("all", "hard"):
                twin = TWINS[o["loss_type"]](x64.copy(), lo.copy(), o["margin"], kind)
            else:
                twin = ref_tu.compute_ge2e_loss(x64.copy(), lo.copy(), o["w"], o["b"], kind)
            twin = float(twin)
            r = ref.evaluate(kind, xo, lo, **o)
            if kind == "semihard":
                stats["gap"] = min(stats["gap"], r["min_gap"])
                assert r["min_gap"] > 1e-6, (name, r["min_gap"])
            elif kind in ("all", "hard"):
                c = r["cos"] - np.diag(np.diag(r["cos"]))
                stats["cos"] = max(stats["cos"], np.abs(c).max())
                assert np.abs(c).max() < 0.999, (name, np.abs(c).max())
                if kind == "all":
                    stats["t"] = min(stats["t"], r["min_abs_t"])
                    assert r["min_abs_t"] > 1e-6, (name, r["min_abs_t"])
            else:
                stats["prob"] = min(stats["prob"], r["min_target_prob"])
                assert r["min_target_prob"] > 1e-6, (name, r["min_target_prob"])
            worst = max(worst, abs(r["loss"] - twin))
            assert abs(r["loss"] - twin) < 1e-12, (name, order, r["loss"], twin)
            np.savez(os.path.join(HERE, "metric_%s_%s.npz" % (name, order)), x=xo, labels=lo, kind=np.array(kind),
                     loss_type=np.array(o.get("loss_type", "")), margin=np.float64(o.get("margin", 0.0)),
                     squared=np.int64(o.get("squared", False)), normalize=np.int64(o.get("normalize", True)),
                     w=np.float64(o.get("w", 0.0)), b=np.float64(o.get("b", 0.0)), loss=np.float64(twin))
    print("%d metric-loss fixtures written to %s" % (2 * len(cases), HERE))
    print("largest |oracle - twin| %.3g; least distance gap %.3g, least |t| %.3g, least target probability %.3g, largest |cos| %.3g"
          % (worst, stats["gap"], stats["t"], stats["prob"], stats["cos"]))


if __name__ == "__main__":
    main()
