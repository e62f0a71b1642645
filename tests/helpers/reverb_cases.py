"""The utterances of tests/test_gpu_reverb.py, sized from the kernel's tile T and chunk C, with their float64 references
(tests/helpers/ref_reverb.py) computed once and shared.  A case is a dict: x, fs, h (or None), noises [(v, snr, start, ext)],
and the options of ref_reverb.reverberate."""
import numpy as np

import ref_reverb as R

CLOSE_CAP = 0.01          # share of samples that may lie within the bound of a saturation threshold


def sig(n, seed, amp=3000.0):
    return np.clip(np.random.RandomState(seed).standard_normal(n) * amp, -32768, 32767).astype(np.int16)


def rir(L, seed, peak=None, peak_value=30000, tail=6000.0):
    """A decaying random response with its largest signed sample at `peak` (default: about L / 8)."""
    rs = np.random.RandomState(seed)
    peak = min(L - 1, L // 8) if peak is None else peak
    h = rs.standard_normal(L) * tail * np.exp(-np.arange(L) / (L / 4.0 + 1.0))
    h = np.clip(h, -20000, 20000)
    h[peak] = peak_value
    return h.astype(np.int16)


def case(x, fs=16000, h=None, noises=(), **opts):
    return dict(x=x, fs=fs, h=h, noises=list(noises), opts=opts)


def conv_lengths(T, C):
    return [1, T - 1, T, T + 1, 3 * T + 5], [1, 2, C - 1, C, C + 1, 2 * C + 3]


def conv_cases(T, C):
    """Every N x L around the tile and chunk edges, fs alternating between 8000 and 16000."""
    out = {}
    Ns, Ls = conv_lengths(T, C)
    for i, n in enumerate(Ns):
        for j, l in enumerate(Ls):
            fs = (8000, 16000)[(i + j) % 2]
            out["conv_N%d_L%d_fs%d" % (n, l, fs)] = case(sig(n, 100 + 7 * i + j), fs, rir(l, 200 + 7 * i + j))
    out["conv_L_above_N"] = case(sig(C // 2 + 3, 150), 8000, rir(2 * C + 3, 250))
    return out


def peak_cases(T, C):
    L = 2 * C + 40                                  # fs = 8000: b = 8, a = 400
    out = {}
    for name, p in (("first", 0), ("last", L - 1), ("near_start", 3), ("near_end", L - 4), ("middle", L // 2)):
        out["peak_" + name] = case(sig(T + 9, 300 + p % 13), 8000, rir(L, 310 + p % 17, peak=p),
                                   noises=[(sig(500, 320), 12.0, 0.0, None)])
    h = rir(L, 330, peak=40, peak_value=9000, tail=2000.0)
    h[90] = -32768                                   # the largest magnitude is negative: the signed maximum stays at 40
    out["peak_signed"] = case(sig(T + 9, 331), 8000, h, noises=[(sig(500, 332), 12.0, 0.0, None)])
    h = np.full(50, 1234, dtype=np.int16)            # equal values: the lowest index
    out["peak_tie"] = case(sig(300, 333), 16000, h)
    return out


def mix_cases(T, C):
    fs = 8000
    N, L = T + 300, C + 17
    Y = N + L - 1
    x, h = sig(N, 400), rir(L, 401)
    v1, v2 = sig(700, 402, 1500.0), sig(2 * T + 50, 403, 800.0)
    sec = lambda n: (n + 0.5) / fs                  # noqa: E731  (trunc(t fs) = n)
    out = {
        "mix_start_at_Y": case(x, fs, h, [(v1, 10.0, sec(Y), None)]),
        "mix_start_past_Y": case(x, fs, h, [(v1, 10.0, sec(Y + 1000), None)]),
        "mix_runs_past_end": case(x, fs, h, [(v2, 5.0, sec(Y - 333), None)]),
        "mix_modulo": case(x, fs, h, [(v1, 8.0, sec(100), 3 * 700 + 11)]),
        "mix_two_overlapping": case(x, fs, h, [(v1, 15.0, sec(50), None), (v2, 3.0, sec(400), None)]),
        "mix_none": case(x, fs, h),
        "mix_no_rir": case(x, fs, None, [(v1, 6.0, sec(20), 2000), (v2, 12.0, 0.0, None)]),
        "plain": case(x, fs, None, normalize_output=False, shift_output=False),
        "emit_duration_below_N": case(x, fs, h, [(v1, 10.0, 0.0, None)], duration=sec(N - 700)),
        "emit_duration_equal_N": case(x, fs, h, duration=sec(N)),
        "emit_duration_above_Y_shift": case(x, fs, h, [(v1, 10.0, 0.0, None)], duration=sec(2 * Y + 77)),
        "emit_duration_above_Y_no_shift": case(x, fs, h, duration=sec(2 * Y + 77), shift_output=False),
        "emit_no_shift": case(x, fs, h, [(v2, 9.0, sec(5), None)], shift_output=False),
        "emit_no_normalize": case(x, fs, h, [(v1, 10.0, 0.0, None)], normalize_output=False),
        "emit_volume_saturates": case(x, fs, h, [(v1, 10.0, 0.0, None)], volume=6.0),
        "emit_volume_small": case(x, fs, h, volume=0.125, shift_output=False),
    }
    return out


_cache = {}


def all_cases(T, C):
    key = (T, C)
    if key not in _cache:
        cases = {}
        for part in (conv_cases, peak_cases, mix_cases):
            cases.update(part(T, C))
        for name, c in cases.items():
            c["name"] = name
        _cache[key] = cases
    return _cache[key]


def ref(c):
    """The float64 reference of a case, computed once."""
    if "ref" not in c:
        c["ref"] = R.reverberate(c["x"], c["fs"], c["h"], c["noises"], **c["opts"])
    return c["ref"]


def close_mask(r):
    """Samples whose reference lies within the bound of a saturation threshold (trunc(v) leaves int16 at v >= 32768 and at
    v <= -32769): too close to call."""
    return (np.abs(r.out - 32768.0) <= r.bound) | (np.abs(r.out + 32769.0) <= r.bound)
