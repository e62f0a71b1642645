"""Pooling on its own: float64 references, per-element error bars, and fp32 emulations of the pooling kernels (numpy only).

The pooling kernels (csrc/pool.hip, the pooling epilogues of csrc/xv_epilogue.h and csrc/xv_epilogue_n32.h) are checked against a float64 pooling of the
frames the GPU itself produced, so the GEMM's error is not in the budget and every bar below follows from fp32 summation
alone.  u = 2^-24 (unit round-off), n = frames of the utterance, k = 64-row slots it touches in the packed batch.

References (the formulas of oracle/ref_numpy.statistics_pooling / attention_core; weights are taken as given, never
renormalised):
    stat_pool(x), weighted_pool(x, w) -> (mean, variance before the floor, floored std);  softmax_weights(...).

Bars.  a = mean |x| (statistics) or sum w |x| (attention), v = the float64 variance.

  mean      |m^ - m| <= E_m = C1 (n + k) (u a + eta),  C1 = 2,  eta = 2^-149.
      A sum of n terms carries at most n - 1 roundings per term when it is accumulated sequentially (the strided / pairwise
      orders of the kernels carry fewer), the attention product w x one more, and the division (or the multiplication by a
      rounded 1 / n) two: at most n + 2 roundings on any term.  The slot forms sum <= 64 frames pairwise and then k slots
      sequentially: fewer again.  n + 2 <= 2 (n + k) for every n, k >= 1, and the factor left over covers the second-order
      part of gamma_n = n u / (1 - n u) at n = 12 000.  eta is the underflow term of the standard model
      fl(x op y) = (x op y)(1 + delta) + eta': a product w x with a subnormal result is rounded to a multiple of 2^-149, an
      absolute error, not a relative one.  It matters only where a = sum w |x| is itself subnormal-sized: a channel that is
      zero on the few frames that carry a peaked attention's weight (found on the emulations, with the peaked weights of the
      host test; in the variance it disappears in the 4 u about the 1e-12 floor).

  variance  |v^ - v| <= E_v = E_m^2 + C2 (n + k) u (v + E_m^2),  C2 = 3.
      Every kernel forms d = fl(x - m^) with the COMPUTED mean, and sum (x - m^)^2 / n = v + (m^ - m)^2 exactly: the mean's
      error enters squared, not multiplied by m as in E[x^2] - m^2 (error ~ n u m^2).  Then d carries one rounding (two on
      d^2), the square one, the weight product one, the accumulation at most n - 1, the division two: n + 4 <= 3 (n + k)
      whenever 2 n + 3 k >= 4.  Chan merges: the slot partials carry <= 11 roundings, the between term n_i d_i^2 four and
      the merge k: min(n, 11) + k + 6 <= 3 (n + k) for n >= 2 (n = 1: every term is an exact zero).
      Two second-order terms are NOT in this form and are named here so that a miss can be traced to them: (i) a Chan merge
      sees each slot mean with its own error e_i <= 12 u a, which leaves 2 / n sum n_i e_i (mu_i - m) <= 2 max|e_i| sqrt(v)
      (Cauchy-Schwarz; zero for k = 1, and the M2 of a slot is taken about the very same rounded slot mean the merge
      recomputes); (ii) attention weights that sum to W != 1 leave 2 (m - m^) m (1 - W).  Both stay far inside E_m^2 for the
      sequential-sum E_m used here unless every rounding lines up; the host tests hold the emulations to the bars as stated.

  std       accepted when std^2 lies in [floor(v - E_v), floor(v + E_v)], widened by 4 u (sqrtf: one rounding = 2 u on the
            square; the fp32 floor constant: one), floor(y) = 1e-12 if y <= 1e-12 else y.

  weights   |w^_t / w_t - 1| <= 2 E_s + C3 (n + 8) u,  E_s = (d_k + 2) u |scale| max_t sum_d |k_td q_d|,  C3 = 2.
      A score is d_k fused multiply-adds (sequential worst case) and the scale: (d_k + 1) u S; fl(s_t - max) adds u |s_t - max|
      <= 2 u S; numerator and denominator each move by that: 2 E_s.  expf <= 2 u, the sum n + 8 (256 strided accumulators,
      six shuffles, the cross-wave adds), 1 / sum and the product one each: n + 14 <= 2 (n + 8).  Reference weights below
      1e-30 are compared absolutely, against the bar times 1e-30.

Emulations: the arithmetic of each kernel as its source writes it, in numpy fp32, vectorised over channels.  A fused
multiply-add is emulated through float64 (the product of two fp32 numbers is exact there).  Mutants are switches of the
emulations; tests/test_pool_bars_host.py requires each of them to leave a bar.
"""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -149                             # underflow unit: the spacing of the subnormal fp32 numbers
FLOOR = 1e-12
C1, C2, C3 = 2, 3, 2
F32 = np.float32
TINY_W = 1e-30


# --------------------------------------------------------------------------------------------------------- references
def n_slots(r0, n):
    """64-row slots that rows r0 .. r0 + n - 1 of the packed batch touch."""
    return ((r0 + n - 1) >> 6) - (r0 >> 6) + 1


def floor_var(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(v <= FLOOR, FLOOR, v)


def stat_pool(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.mean(axis=0)
    v = ((x - m) ** 2).mean(axis=0)
    return m, v, np.sqrt(floor_var(v))


def weighted_pool(x, w):
    """x [n, C], w [n]: mean = sum w x, variance = sum w (x - mean)^2 (model/pooling.py:203-206)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    m = w @ x
    v = w @ (x - m) ** 2
    return m, v, np.sqrt(floor_var(v))


def head_columns(dv, H, split):
    """(head, value columns, output columns) of the pooled vector's mean half (odim = dv if split else dv * H)."""
    if split:
        dvh = dv // H
        return [(h, np.arange(h * dvh, (h + 1) * dvh), np.arange(h * dvh, (h + 1) * dvh)) for h in range(H)]
    return [(h, np.arange(dv), h * dv + np.arange(dv)) for h in range(H)]


def weighted_pool_heads(x, w, split):
    """x [n, dv], w [n, H] -> (mean, var, std), each [odim]."""
    dv, H = x.shape[1], w.shape[1]
    odim = dv if split else dv * H
    m, v, s = np.zeros(odim), np.zeros(odim), np.zeros(odim)
    for h, vc, oc in head_columns(dv, H, split):
        m[oc], v[oc], s[oc] = weighted_pool(x[:, vc], w[:, h])
    return m, v, s


def scores64(key, query, scale, heads, split_key):
    key = np.asarray(key, dtype=np.float64)
    query = np.asarray(query, dtype=np.float64)
    dk = key.shape[1]
    dkh = dk // heads if split_key else dk
    s = np.empty((key.shape[0], heads))
    mag = np.empty((key.shape[0], heads))
    for h in range(heads):
        kh = key[:, h * dkh:(h + 1) * dkh] if split_key else key
        s[:, h] = scale * (kh @ query[h])
        mag[:, h] = abs(scale) * (np.abs(kh) @ np.abs(query[h]))
    return s, mag, dkh


def softmax_weights(key, query, scale, heads, split_key):
    """key [n, dk] of ONE utterance, query [H, dk or dk / H] -> weights [n, H] (softmax over the frames)."""
    s, _, _ = scores64(key, query, scale, heads, split_key)
    e = np.exp(s - s.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def score_bar(key, query, scale, heads, split_key):
    """E_s per head."""
    _, mag, dkh = scores64(key, query, scale, heads, split_key)
    return (dkh + 2) * U * mag.max(axis=0)


# --------------------------------------------------------------------------------------------------------------- bars
def mean_bar(n, k, a):
    return C1 * (n + k) * (U * np.asarray(a, dtype=np.float64) + ETA)


def var_bar(n, k, a, v):
    em2 = mean_bar(n, k, a) ** 2
    return em2 + C2 * (n + k) * U * (np.asarray(v, dtype=np.float64) + em2)


def weight_bar(n, e_s):
    return 2.0 * np.asarray(e_s, dtype=np.float64) + C3 * (n + 8) * U


def mean_ratio(got, m, e_m):
    """|got - m| / E_m per element; a zero bar (all-zero channel) admits only the exact value."""
    err = np.abs(np.asarray(got, dtype=np.float64) - m)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e_m > 0, err / e_m, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(np.asarray(got, dtype=np.float64)), r, np.inf)


def std_ratio(got_std, v, e_v):
    """Distance of std^2 from floor(v) in units of the accepted interval's half on that side (<= 1: accepted)."""
    g = np.asarray(got_std, dtype=np.float64)
    g2 = g * g
    fv = floor_var(v)
    hi = floor_var(v + e_v) * (1 + 4 * U)
    lo = floor_var(v - e_v) * (1 - 4 * U)
    r = np.where(g2 >= fv, (g2 - fv) / (hi - fv), (fv - g2) / (fv - lo))
    return np.where(np.isfinite(g) & (g >= 0), r, np.inf)


def weight_ratio(got, w, bar):
    """got, w [n, H]; bar [H]."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - w)
    r = err / (np.maximum(w, TINY_W) * bar)
    return np.where(np.isfinite(got), r, np.inf)


def stat_check(x, r0, got_mean, got_std):
    """Per-element ratios (mean, std) of a pooled utterance against the float64 pooling of its own frames x [n, C]."""
    n = x.shape[0]
    k = n_slots(r0, n)
    m, v, _ = stat_pool(x)
    a = np.abs(np.asarray(x, dtype=np.float64)).mean(axis=0)
    return mean_ratio(got_mean, m, mean_bar(n, k, a)), std_ratio(got_std, v, var_bar(n, k, a, v))


def att_check(x, w, split, r0, got_mean, got_std):
    """The same for attentive pooling: x [n, dv], w [n, H] as given."""
    n, dv = x.shape
    H = w.shape[1]
    k = n_slots(r0, n)
    m, v, _ = weighted_pool_heads(x, w, split)
    a = np.zeros_like(m)
    ax = np.abs(np.asarray(x, dtype=np.float64))
    for h, vc, oc in head_columns(dv, H, split):
        a[oc] = np.asarray(w[:, h], dtype=np.float64) @ ax[:, vc]
    return mean_ratio(got_mean, m, mean_bar(n, k, a)), std_ratio(got_std, v, var_bar(n, k, a, v))


# -------------------------------------------------------------------------------------------------------- emulations
def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def _tree(parts):
    """xor-shuffle reduction of a power-of-two list: neighbours first, as lane group 0 sees it."""
    parts = list(parts)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0]


def _finish(mean, var, no_floor):
    var = np.asarray(var, dtype=F32)
    if not no_floor:
        var = np.where(var <= F32(FLOOR), F32(FLOOR), var)
    with np.errstate(invalid="ignore"):
        return np.asarray(mean, dtype=F32), np.sqrt(var).astype(F32)


def emu_stat_pool(x, one_pass=False, no_floor=False):
    """stat_pool_kernel: 16 row slots (frames r = rs mod 16, ascending), lanes 16 and 32 apart inside a wave, then the four
    waves in order; mean = sum * fl(1 / L); the second sweep about that mean."""
    x = np.asarray(x, dtype=F32)
    n, C = x.shape
    inv = F32(1.0) / F32(n)

    def block_sum(rows):                       # rows [n, C] -> [C]
        acc = np.zeros((16, C), dtype=F32)
        for i in range(0, n, 16):
            c = rows[i:i + 16]
            acc[:c.shape[0]] += c
        waves = [(acc[4 * w] + acc[4 * w + 1]) + (acc[4 * w + 2] + acc[4 * w + 3]) for w in range(4)]
        return ((waves[0] + waves[1]) + waves[2]) + waves[3]

    mean = block_sum(x) * inv
    if one_pass:
        var = block_sum(x * x) * inv - mean * mean
    else:
        d = x - mean
        var = block_sum(d * d) * inv
    return _finish(mean, var, no_floor)


def _segments(r0, n):
    """(tile row of the first frame, frames) of each 64-row slot of an utterance that starts at packed row r0."""
    out, r, r1 = [], r0, r0 + n
    while r < r1:
        e = min(r1, ((r >> 6) + 1) << 6)
        out.append((r & 63, e - r))
        r = e
    return out


def _group_sum(rows, t_first, G):
    """Sum of the rows of one slot segment: frame at tile row t goes to group t mod G (accumulated in ascending t), the G
    groups are combined by an xor tree.  Absent frames add nothing (the kernels skip them)."""
    C = rows.shape[1]
    acc = np.zeros((G, C), dtype=F32)
    t = t_first
    i = 0
    while i < rows.shape[0]:                   # frames up to the next multiple of G form one in-lane step
        g0 = t % G
        cnt = min(G - g0, rows.shape[0] - i)
        acc[g0:g0 + cnt] += rows[i:i + cnt]
        i += cnt
        t += cnt
    return _tree([acc[g] for g in range(G)])


def emu_tile_stats(x, r0, G=8):
    """The fused statistics epilogue: per 64-row slot (sum, M2 about the slot mean).  G = 8: the LDS-staged form of the
    128 x 32 wave tile, G = 4: of the 64 x 64 tile, G = 16: the accumulator form (16 frames of a DPP row, four in-lane)."""
    x = np.asarray(x, dtype=F32)
    parts, i = [], 0
    for t_first, ni in _segments(r0, x.shape[0]):
        seg = x[i:i + ni]
        s1 = _group_sum(seg, t_first, G)
        mu = s1 / F32(ni)
        d = seg - mu
        parts.append((s1, _group_sum(d * d, t_first, G), ni))
        i += ni
    return parts


def emu_pool_finalize(parts, no_between=False, no_floor=False):
    """pool_finalize_kernel: slots in order; mean = sum s_i / L; M2 = sum [M2_i + n_i (s_i / n_i - mean)^2]."""
    n = sum(p[2] for p in parts)
    s = np.zeros_like(parts[0][0])
    for s1, _, _ in parts:
        s = s + s1
    mean = s / F32(n)
    m2 = np.zeros_like(s)
    for s1, q, ni in parts:
        d = s1 / F32(ni) - mean
        m2 = m2 + (q if no_between else q + F32(ni) * d * d)
    return _finish(mean, m2 / F32(n), no_floor)


def emu_stat_fused(x, r0, G=8, **mutant):
    return emu_pool_finalize(emu_tile_stats(x, r0, G), **mutant)


def emu_att_pool(x, w, one_pass=False, no_floor=False):
    """att_pool_kernel for one head: four waves take the frames r mod 4, fused multiply-adds, the waves added in order."""
    x = np.asarray(x, dtype=F32)
    w = np.asarray(w, dtype=F32)
    n, C = x.shape

    def block_sum(rows, ws):
        acc = np.zeros((4, C), dtype=F32)
        for i in range(0, n, 4):
            c = rows[i:i + 4]
            acc[:c.shape[0]] = _fma(c, ws[i:i + 4, None], acc[:c.shape[0]])
        return ((acc[0] + acc[1]) + acc[2]) + acc[3]

    mean = block_sum(x, w)
    if one_pass:
        var = block_sum(x * x, w) - mean * mean
    else:
        d = x - mean
        var = block_sum(d * d, w)
    return _finish(mean, var, no_floor)


def _weighted_group_sum(rows, ws, t_first, G=8):
    C = rows.shape[1]
    acc = np.zeros((G, C), dtype=F32)
    t, i = t_first, 0
    while i < rows.shape[0]:
        g0 = t % G
        cnt = min(G - g0, rows.shape[0] - i)
        acc[g0:g0 + cnt] += rows[i:i + cnt] * ws[i:i + cnt, None]
        i += cnt
        t += cnt
    return _tree([acc[g] for g in range(G)])


def emu_att_tile_moments(x, w, r0, safe_inverse=True):
    """The weighted-moment epilogue of the value layer for one head: per slot s1 = sum w x and m2 = sum w (x - s1 / s0)^2,
    s0 by a 64-lane butterfly (far lanes first).  safe_inverse: the slot mean is s1 * (1 / s0) only while s0 is a normal
    number (a subnormal s0 would overflow the reciprocal); False reproduces `s0 > 0.f ? 1.0f / s0 : 0.f`."""
    x = np.asarray(x, dtype=F32)
    w = np.asarray(w, dtype=F32)
    parts, i = [], 0
    for t_first, ni in _segments(r0, x.shape[0]):
        seg, ws = x[i:i + ni], w[i:i + ni]
        lanes = np.zeros(64, dtype=F32)
        lanes[t_first:t_first + ni] = ws
        s0 = lanes
        while s0.shape[0] > 1:                 # xor 32, 16, ..., 1
            h = s0.shape[0] // 2
            s0 = s0[:h] + s0[h:]
        s0 = s0[0]
        s1 = _weighted_group_sum(seg, ws, t_first)
        ok = s0 >= F32(1.1754944e-38) if safe_inverse else s0 > 0
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            mu = s1 * (F32(1.0) / s0 if ok else F32(0.0))
            d = seg - mu
            m2 = _weighted_group_sum(d * d, ws, t_first)
        s0_seq = F32(0.0)                      # att_slot_sums_kernel: the frames in order
        for v in ws:
            s0_seq = s0_seq + v
        parts.append((s1, m2, s0_seq))
        i += ni
    return parts


def emu_att_pool_finalize(parts, no_between=False, no_floor=False, no_zero_branch=False):
    """att_pool_finalize_kernel: mean = sum s1_s; var = sum [m2_s + s0_s (s1_s / s0_s - mean)^2], d = 0 where s0_s == 0."""
    mean = np.zeros_like(parts[0][0])
    for s1, _, _ in parts:
        mean = mean + s1
    var = np.zeros_like(mean)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for s1, m2, s0 in parts:
            if s0 > 0 or no_zero_branch:
                d = s1 / s0 - mean
            else:
                d = np.zeros_like(mean)
            var = var + (m2 if no_between else m2 + s0 * d * d)
    return _finish(mean, var, no_floor)


def emu_att_fused(x, w, r0, safe_inverse=True, **mutant):
    return emu_att_pool_finalize(emu_att_tile_moments(x, w, r0, safe_inverse), **mutant)


def emu_att_heads(fn, x, w, split, head_shift=0, **kw):
    """Run a one-head emulation `fn(x_cols, w_head, **kw)` over the head layout; head_shift = 1 is the mutant that pools
    the columns of head h + 1 with the weights of head h."""
    dv, H = x.shape[1], w.shape[1]
    odim = dv if split else dv * H
    mean, std = np.zeros(odim, dtype=F32), np.zeros(odim, dtype=F32)
    for h, vc, oc in head_columns(dv, H, split):
        mean[oc], std[oc] = fn(x[:, vc], w[:, (h - head_shift) % H], **kw)
    return mean, std
