"""Float64 numpy statement of the wav-reverberate rule (include/xvec_hip.h, csrc/reverb.hip), and the error bound the
float32 kernel is held to.  No Kaldi pins it: **parity unpinned**."""
import numpy as np

U = 2.0 ** -24


class Ref(object):
    """out: float64 [n_out] before the int16 conversion; out_i16 / clipped: rule 7; p, scale; bound: the per-sample bound of
    csrc/reverb.hip on the float32 output."""
    pass


def _conv(h, x):
    return np.convolve(x, h) if h.size and x.size else np.zeros(0)


def reverberate(x, fs, h=None, noises=(), shift_output=True, normalize_output=True, duration=0.0, volume=0.0):
    """x: int16 samples; h: int16 impulse response or None; noises: (v int16, snr_db, start_time, ext_len or None) in order.
    ValueError where the rule says error."""
    xi = np.asarray(x)
    assert xi.dtype == np.int16 and xi.ndim == 1 and xi.size >= 1
    x = xi.astype(np.float64)
    N = x.size
    p_before = float(np.sum(x * x)) / N
    if h is not None:
        hi = np.asarray(h)
        assert hi.dtype == np.int16 and 1 <= hi.size <= 65536
        hf = hi.astype(np.float64) / 32768.0
        p = int(np.argmax(hi))                       # lowest index of the largest signed value
    else:
        hf = np.ones(1)
        p = 0
    L = hf.size
    y = _conv(hf, x)
    A = _conv(np.abs(hf), np.abs(x))
    b, a = int(0.001 * fs), int(0.05 * fs)
    s, e = max(0, p - b), min(L, p + a)
    early = _conv(hf[s:e], x)
    assert early.size == N + (e - s) - 1
    E = float(np.sum(early * early)) / early.size
    A_e = _conv(np.abs(hf[s:e]), np.abs(x))
    norm_e = np.sqrt(np.sum(early * early))
    eta_E = (e - s) * U * np.sqrt(np.sum(A_e * A_e)) / norm_e if norm_e > 0 else 0.0
    Y = y.size
    added = np.zeros(Y)
    for v, snr, start, ext in noises:
        v = np.asarray(v)
        assert v.dtype == np.int16 and v.size >= 1
        v = v.astype(np.float64)
        M = v.size
        ext = M if ext is None else int(ext)
        assert ext >= 1
        idx = np.arange(ext) % M
        P = float(np.sum(v[idx] ** 2)) / ext
        if P == 0.0:
            raise ValueError("an additive signal has zero power")
        g = np.sqrt(10.0 ** (-snr / 10.0) * E / P)
        o = int(start * fs)
        n = min(ext, Y - o)
        if n > 0:
            y[o:o + n] += g * v[idx[:n]]
            added[o:o + n] += np.abs(g * v[idx[:n]])
    A = A + added
    p_after = float(np.sum(y * y)) / Y
    if volume > 0:
        scale = float(volume)
    elif normalize_output:
        if p_after == 0.0:
            raise ValueError("the output has zero power")
        scale = np.sqrt(p_before / p_after)
    else:
        scale = 1.0
    shift = p if (h is not None and shift_output) else 0
    n_out = int(duration * fs) if duration > 0 else (N if shift_output else Y)
    src = (np.arange(n_out) + shift) % Y
    r = Ref()
    r.out = scale * y[src]
    t = np.trunc(r.out)
    r.clip_mask = (t > 32767) | (t < -32768)
    r.clipped = int(r.clip_mask.sum())
    r.out_i16 = np.clip(t, -32768, 32767).astype(np.int16)
    r.p, r.scale, r.n_out, r.Y, r.E, r.p_before, r.p_after = p, scale, n_out, Y, E, p_before, p_after
    # csrc/reverb.hip: eps[n] = (L + J + 12) u A[n] + eta_E sum_j |g_j v_j[n]|, delta = ||eps||_2 / ||y||_2 + 8u,
    # |out - ref| <= scale eps[n] + |ref| delta  (with J = 0: (L + 12) u A[n] alone)
    eps = (L + len(noises) + 12) * U * A + eta_E * added
    norm_y = np.sqrt(np.sum(y * y))
    delta = (np.sqrt(np.sum(eps * eps)) / norm_y if norm_y > 0 else 0.0) + 8 * U
    r.bound = scale * eps[src] + np.abs(r.out) * delta
    return r
