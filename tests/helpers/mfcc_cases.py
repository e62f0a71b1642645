"""Shared inputs of the MFCC / VAD tests: deterministic int16 signals and the three option sets of the issue, as dictionaries for
the oracle (tests/helpers/ref_mfcc.py) and as `--name=value` config text for the product."""
import numpy as np

import ref_mfcc

CONFIGS = {"kaldi_defaults": ref_mfcc.DEFAULTS, "voxceleb": ref_mfcc.VOXCELEB, "sre": ref_mfcc.SRE}
VAD_CONFIGS = {"kaldi_defaults": ref_mfcc.VAD_DEFAULTS, "voxceleb": ref_mfcc.VAD_VOXCELEB}
LENGTHS = [100, 399, 400, 401, 560, 1360, 4000, 16123]


def config_text(opts):
    lines = ["# written by the test"]
    for k, v in sorted(opts.items()):
        lines.append("--%s=%s" % (k.replace("_", "-"), str(v).lower() if isinstance(v, bool) else v))
    return "\n".join(lines) + "\n\n"


def signal(n, fs, seed, dc=120.0, gain=1.0):
    """A few harmonics of amplitude about 3000 plus white noise of amplitude about 30 plus a DC offset."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / fs
    f0 = 110.0 + 40.0 * (seed % 5)
    x = np.zeros(n)
    for h, a in ((1, 3000.0), (3, 1800.0), (7, 900.0), (12, 500.0)):
        x += a * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi))
    x = gain * x + rng.uniform(-30.0, 30.0, size=n) + dc
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def batch(fs):
    """The eight utterances of the GPU test; the last one is digital silence (a constant) for its second half."""
    utts = [signal(n, fs, seed=10 + i, dc=(-200.0, 0.0, 350.0)[i % 3]) for i, n in enumerate(LENGTHS)]
    utts[-1] = utts[-1].copy()
    utts[-1][LENGTHS[-1] // 2:] = 350
    return utts


def loud_quiet(fs, seconds, seed):
    """Alternating loud and quiet segments (VAD test, command-line test)."""
    rng = np.random.RandomState(seed)
    n = int(fs * seconds)
    x = signal(n, fs, seed, dc=40.0).astype(np.float64)
    gain = np.ones(n)
    pos = 0
    loud = bool(seed % 2)
    while pos < n:
        seg = int(fs * rng.uniform(0.15, 0.45))
        gain[pos:pos + seg] = 1.0 if loud else 0.004
        loud = not loud
        pos += seg
    x = (x - 40.0) * gain + 40.0 + rng.uniform(-4.0, 4.0, size=n)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def silence_frames(num_samples, first_constant, opts):
    """Frames of an utterance whose samples all come from [first_constant, num_samples)."""
    idx = ref_mfcc.frame_indices(num_samples, opts)
    return np.flatnonzero((idx >= first_constant).all(axis=1))
