"""The inputs of tests/test_gpu_att_pool.py and tests/test_att_pool_host.py (self-attentive pooling of packed rows and its
gradient, csrc/att_pool_grad.hip).

One batch per case, the layout of pool_grad_cases.py: twelve utterances of LENGTHS frames behind LEAD rows that no utterance
owns (NaN).  The value rows are pool_grad_cases.make(Dv): ordinary, offset and scaled channels, ONE constant channel and a near
constant one.  The key rows are N(0, 1), the query N(0, 1) 2 / sqrt(dq) (scores of the order of 2, or of 2 / sqrt(dq) with the
scale: peaked and flat softmaxes both occur).

CASES is a covering design over the dimensions (H in 1, 2, 3, 5; per-head widths 1, 3, 4, 5, 63, 64, 65 on both sides; the four
split combinations; scale on and off): every H meets every split combination, and inside each of those sixteen cells the seven
widths run through the key side and, rotated by three, through the value side, the scale alternating.  So every width occurs on
both sides with every H and every split combination, both with and without the scale somewhere in its H: 112 cases.  The full
product (1568) checks nothing these do not: the kernels have no path that depends on a PAIR of widths."""
import zlib

import numpy as np

import pool_grad_cases as pc
import ref_att_pool as ra

F = np.float32
HEADS = (1, 2, 3, 5)
WIDTHS = (1, 3, 4, 5, 63, 64, 65)
SPLITS = ((0, 0), (0, 1), (1, 0), (1, 1))
LENGTHS, LEAD = pc.LENGTHS, pc.LEAD

CASES = [ra.Cfg(H, WIDTHS[i], WIDTHS[(i + 3) % 7], sk, sv, (i + sk + sv + H) % 2)
         for H in HEADS for (sk, sv) in SPLITS for i in range(7)]


def make(cfg, seed=None):
    """-> dict(key [rows, Dk], value [rows, Dv], query [H, dq], gp [12, 2 P] float32, offsets int32 [13], const: the constant
    value COLUMN or None); the LEAD unowned rows of key and value are NaN."""
    r = np.random.RandomState(zlib.crc32(repr(cfg).encode()) if seed is None else seed)
    val = pc.make(cfg.Dv, seed=r.randint(1 << 30))
    rows = val["x"].shape[0]
    key = r.standard_normal((rows, cfg.Dk)).astype(F)
    key[:LEAD] = np.nan
    query = (r.standard_normal((cfg.H, cfg.dq)) * 2.0 / np.sqrt(cfg.dq)).astype(F)
    gp = r.standard_normal((len(LENGTHS), 2 * cfg.P)).astype(F)
    return dict(cfg=cfg, key=key, value=val["x"], query=query, gp=gp, offsets=val["offsets"], const=val["const"])


def rows_of(case, u):
    o = case["offsets"]
    return slice(int(o[u]), int(o[u + 1]))
