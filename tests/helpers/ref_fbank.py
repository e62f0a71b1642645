"""ORACLE (test infrastructure only): numpy restatement of Kaldi's compute-fbank-feats, the first step of the ResNet recipe
(egs/voxceleb/v3/run.sh:54).  Written from the definition in the header of csrc/mfcc.hip, not from the kernel: the framing,
window and mel bank of ref_mfcc.py, a direct real FFT, a dense mel matrix.  float64 throughout; `dtype=np.float32` runs the same
statements with float32 tables and a float32 FFT (scipy.fft.rfft), as ref_mfcc.mfcc does.
**parity unpinned**: no Kaldi binary or fixture is available to pin it."""
import numpy as np

import ref_mfcc

FLT_EPSILON = ref_mfcc.FLT_EPSILON

DEFAULTS = dict(sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, preemphasis_coefficient=0.97,
                remove_dc_offset=True, window_type="povey", snip_edges=True, num_mel_bins=23, low_freq=20.0, high_freq=0.0,
                use_energy=False, energy_floor=0.0, raw_energy=True, use_log_fbank=True, use_power=True)
V3 = dict(DEFAULTS, window_type="hamming", num_mel_bins=40, low_freq=20.0, high_freq=7600.0, snip_edges=False)     # v3/fbank.conf
ENERGY8K = dict(DEFAULTS, sample_frequency=8000.0, num_mel_bins=64, use_energy=True, raw_energy=False, energy_floor=1.0,
                use_power=False)
LINEAR = dict(V3, use_log_fbank=False)
CONFIGS = {"v3": V3, "kaldi_defaults": DEFAULTS, "energy8k": ENERGY8K, "linear": LINEAR}


def num_feats(o):
    return o["num_mel_bins"] + int(bool(o["use_energy"]))


def fbank(samples, opts=None, dtype=np.float64):
    """samples: int16 (or integer-valued) vector.  Returns ([T, num_feats], [T] log energy), both in `dtype`."""
    o = dict(DEFAULTS, **(opts or {}))
    n, s, p = ref_mfcc.frame_sizes(o)
    x = np.asarray(samples).astype(dtype)
    t = ref_mfcc.num_frames(x.shape[0], o)
    if t == 0:
        return np.zeros((0, num_feats(o)), dtype=dtype), np.zeros(0, dtype=dtype)
    eps = dtype(FLT_EPSILON)
    fr = x[ref_mfcc.frame_indices(x.shape[0], o)]
    if o["remove_dc_offset"]:
        fr = fr - fr.mean(axis=1, keepdims=True, dtype=dtype)
    if o["raw_energy"]:
        log_e = np.log(np.maximum((fr * fr).sum(axis=1, dtype=dtype), eps))
    c = dtype(o["preemphasis_coefficient"])
    fr = fr - c * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = fr * ref_mfcc.window(o).astype(dtype)[None, :]
    if not o["raw_energy"]:
        log_e = np.log(np.maximum((fr * fr).sum(axis=1, dtype=dtype), eps))
    if o["energy_floor"] > 0:
        log_e = np.maximum(log_e, dtype(np.log(o["energy_floor"])))
    log_e = log_e.astype(dtype)
    padded = np.zeros((t, p), dtype=dtype)
    padded[:, :n] = fr
    if dtype == np.float32:
        import scipy.fft
        spec = scipy.fft.rfft(padded, axis=1)
        assert spec.dtype == np.complex64
    else:
        spec = np.fft.rfft(padded, axis=1)
    power = (spec.real * spec.real + spec.imag * spec.imag)[:, :p // 2].astype(dtype)
    if not o["use_power"]:
        power = np.sqrt(power)
    mel_e = (power @ ref_mfcc.mel_bank(o).astype(dtype).T).astype(dtype)
    if o["use_log_fbank"]:
        mel_e = np.log(np.maximum(mel_e, eps)).astype(dtype)
    if o["use_energy"]:
        mel_e = np.concatenate([log_e[:, None], mel_e], axis=1)
    return mel_e, log_e
