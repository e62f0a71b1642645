"""ORACLE (test infrastructure only): numpy restatement of Kaldi's compute-mfcc-feats and compute-vad-decision, the
first step of the reference recipe (egs/voxceleb/v1/run.sh:57-65).  Written from the definition in the header of
csrc/mfcc.hip (Kaldi's published algorithm), not from the kernel: a direct real FFT, dense mel and DCT matrices.
float64 throughout; `dtype=np.float32` runs the same statements with float32 tables and a float32 FFT, which is what the
GPU test uses to measure how far a float32 pipeline may sit from this one.
**parity unpinned**: no Kaldi binary or fixture is available to pin it."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)

DEFAULTS = dict(sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, preemphasis_coefficient=0.97,
                remove_dc_offset=True, window_type="povey", snip_edges=True, num_mel_bins=23, low_freq=20.0, high_freq=0.0,
                num_ceps=13, cepstral_lifter=22.0, use_energy=True, energy_floor=0.0, raw_energy=True)
VOXCELEB = dict(DEFAULTS, num_mel_bins=30, num_ceps=30, low_freq=20.0, high_freq=7600.0, snip_edges=False)
SRE = dict(DEFAULTS, sample_frequency=8000.0, num_mel_bins=23, num_ceps=23, low_freq=20.0, high_freq=3700.0, snip_edges=False)
VAD_DEFAULTS = dict(vad_energy_threshold=5.0, vad_energy_mean_scale=0.5, vad_frames_context=0, vad_proportion_threshold=0.6)
VAD_VOXCELEB = dict(vad_energy_threshold=5.5, vad_energy_mean_scale=0.5, vad_frames_context=2, vad_proportion_threshold=0.12)


def frame_sizes(o):
    n = int(o["sample_frequency"] * 0.001 * o["frame_length"])
    s = int(o["sample_frequency"] * 0.001 * o["frame_shift"])
    p = 1
    while p < n:
        p *= 2
    return n, s, p


def num_frames(num_samples, o):
    n, s, _ = frame_sizes(o)
    if o["snip_edges"]:
        return 0 if num_samples < n else 1 + (num_samples - n) // s
    return (num_samples + s // 2) // s


def frame_indices(num_samples, o):
    """[T, N] sample index of every element of every frame, reflected into [0, L)."""
    n, s, _ = frame_sizes(o)
    t = num_frames(num_samples, o)
    start = np.arange(t, dtype=np.int64) * s + (0 if o["snip_edges"] else s // 2 - n // 2)
    idx = start[:, None] + np.arange(n, dtype=np.int64)[None, :]
    while t and ((idx < 0) | (idx >= num_samples)).any():
        idx = np.where(idx < 0, -idx - 1, idx)
        idx = np.where(idx >= num_samples, 2 * num_samples - 1 - idx, idx)
    return idx


def window(o):
    n = frame_sizes(o)[0]
    a = 2.0 * np.pi * np.arange(n) / (n - 1)
    kind = o["window_type"]
    if kind == "povey":
        return (0.5 - 0.5 * np.cos(a)) ** 0.85
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    if kind == "hanning":
        return 0.5 - 0.5 * np.cos(a)
    if kind == "rectangular":
        return np.ones(n)
    raise ValueError("unknown window type %r" % kind)


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_bank(o):
    """[M, P/2] weights."""
    fs = o["sample_frequency"]
    p = frame_sizes(o)[2]
    m = o["num_mel_bins"]
    nyquist = 0.5 * fs
    high = o["high_freq"] if o["high_freq"] > 0 else nyquist + o["high_freq"]
    low = o["low_freq"]
    assert 0 <= low < nyquist and 0 < high <= nyquist and low < high
    points = mel(low) + (mel(high) - mel(low)) / (m + 1) * np.arange(m + 2)
    left, centre, right = points[:-2, None], points[1:-1, None], points[2:, None]
    u = mel(fs / p * np.arange(p // 2))[None, :]
    w = np.where(u <= centre, (u - left) / (centre - left), (right - u) / (right - centre))
    return np.where((u > left) & (u < right), w, 0.0)


def dct_matrix(m, rows):
    n = np.arange(m)[None, :]
    k = np.arange(rows)[:, None]
    d = np.sqrt(2.0 / m) * np.cos(np.pi / m * (n + 0.5) * k)
    d[0, :] = np.sqrt(1.0 / m)
    return d


def lifter(o):
    q = o["cepstral_lifter"]
    k = np.arange(o["num_ceps"])
    return 1.0 + 0.5 * q * np.sin(np.pi * k / q) if q > 0 else np.ones(len(k))


def mfcc(samples, opts=None, dtype=np.float64, return_mel=False):
    """samples: int16 (or integer-valued) vector.  Returns [T, num_ceps] in `dtype`."""
    o = dict(DEFAULTS, **(opts or {}))
    n, s, p = frame_sizes(o)
    x = np.asarray(samples).astype(dtype)
    t = num_frames(x.shape[0], o)
    if t == 0:
        return np.zeros((0, o["num_ceps"]), dtype=dtype)
    eps = dtype(FLT_EPSILON)
    fr = x[frame_indices(x.shape[0], o)]
    if o["remove_dc_offset"]:
        fr = fr - fr.mean(axis=1, keepdims=True, dtype=dtype)
    if o["raw_energy"]:
        log_e = np.log(np.maximum((fr * fr).sum(axis=1, dtype=dtype), eps))
    c = dtype(o["preemphasis_coefficient"])
    fr = fr - c * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = fr * window(o).astype(dtype)[None, :]
    if not o["raw_energy"]:
        log_e = np.log(np.maximum((fr * fr).sum(axis=1, dtype=dtype), eps))
    if o["energy_floor"] > 0:
        log_e = np.maximum(log_e, dtype(np.log(o["energy_floor"])))
    padded = np.zeros((t, p), dtype=dtype)
    padded[:, :n] = fr
    if dtype == np.float32:
        import scipy.fft
        spec = scipy.fft.rfft(padded, axis=1)
        assert spec.dtype == np.complex64
    else:
        spec = np.fft.rfft(padded, axis=1)
    power = (spec.real * spec.real + spec.imag * spec.imag)[:, :p // 2].astype(dtype)
    mel_e = power @ mel_bank(o).astype(dtype).T
    log_mel = np.log(np.maximum(mel_e, eps)).astype(dtype)
    if return_mel:
        return log_mel
    mat = (dct_matrix(o["num_mel_bins"], o["num_ceps"]) * lifter(o)[:, None]).astype(dtype)
    out = log_mel @ mat.T
    if o["use_energy"]:
        out[:, 0] = log_e
    return out.astype(dtype)


def vad(feats, opts=None):
    """feats [T, >= 1] -> [T] float32 of 0 / 1.
    The mean and the threshold are float64.  The decision count >= window * proportion is Kaldi's float comparison
    (compute-vad-decision: `num_count >= den_count * vad_proportion_threshold` on BaseFloat): the product is rounded to float32
    before it is compared.  Over every proportion 0.01 .. 0.99 and window 1 .. 41 this differs from a float64 comparison in
    three places, all at window 25: 0.6 (the default) with 15 above is unvoiced (25 * 0.6f rounds to 15.000001), 0.28 with 7
    and 0.56 with 14 are voiced (the products round to 7 and 14)."""
    o = dict(VAD_DEFAULTS, **(opts or {}))
    e = np.asarray(feats, dtype=np.float64)[:, 0]
    t = e.shape[0]
    if t == 0:
        return np.zeros(0, dtype=np.float32)
    thr = o["vad_energy_threshold"] + o["vad_energy_mean_scale"] * e.mean()
    above = np.concatenate([[0], np.cumsum(e > thr)])
    c = o["vad_frames_context"]
    lo = np.maximum(np.arange(t) - c, 0)
    hi = np.minimum(np.arange(t) + c, t - 1) + 1
    need = (hi - lo).astype(np.float32) * np.float32(o["vad_proportion_threshold"])
    assert need.dtype == np.float32
    return ((above[hi] - above[lo]).astype(np.float32) >= need).astype(np.float32)


def vad_threshold(feats, opts=None):
    o = dict(VAD_DEFAULTS, **(opts or {}))
    e = np.asarray(feats, dtype=np.float64)[:, 0]
    return o["vad_energy_threshold"] + o["vad_energy_mean_scale"] * e.mean()
