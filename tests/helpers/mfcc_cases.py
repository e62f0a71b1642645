"""Shared inputs of the MFCC / VAD tests: deterministic int16 signals and the three option sets of the issue, as dictionaries for
the oracle (tests/helpers/ref_mfcc.py) and as `--name=value` config text for the product."""
import numpy as np

import ref_fbank
import ref_mfcc

CONFIGS = {"kaldi_defaults": ref_mfcc.DEFAULTS, "voxceleb": ref_mfcc.VOXCELEB, "sre": ref_mfcc.SRE}
VAD_CONFIGS = {"kaldi_defaults": ref_mfcc.VAD_DEFAULTS, "voxceleb": ref_mfcc.VAD_VOXCELEB}
LENGTHS = [100, 399, 400, 401, 560, 1360, 4000, 16123]

# Option sets at the edges of what csrc/mfcc.hip accepts (tests/test_gpu_frontend_edges.py); (N, S, P) in EDGE_SIZES.
#   wide16ms  the smallest unpadded frame of P = 256 without overlap, the most bins and cepstra, coefficient 0 from the DCT, no
#             lifter, no window, no pre-emphasis, no mean removal, filters from 0 Hz -- one of them covers no FFT bin
#   min129    the shortest frame of P = 256 at a shift of one sample, the fewest bins, pre-emphasis 1, hanning, --high-freq < 0
#   full512   the longest frame without overlap (the largest LDS request), the energy after the window, and an energy floor
#             that the batch straddles: the oracle's windowed log energies of batch(16000) are log(FLT_EPSILON) for the constant
#             half and 16.9 .. 18.6 for the rest, with none between 17.50 and 17.88; log(5e7) = 17.73
#   n257      the shortest frame of P = 512, odd N and an S the sample rate does not divide evenly
EDGE_CONFIGS = {
    "wide16ms": dict(ref_mfcc.DEFAULTS, sample_frequency=16000.0, frame_length=16.0, frame_shift=16.0, num_mel_bins=64, num_ceps=64,
                     low_freq=0.0, use_energy=False, cepstral_lifter=0.0, window_type="rectangular", preemphasis_coefficient=0.0,
                     remove_dc_offset=False),
    "min129": dict(ref_mfcc.DEFAULTS, sample_frequency=8000.0, frame_length=16.125, frame_shift=0.125, num_mel_bins=3, num_ceps=3,
                   use_energy=False, window_type="hanning", preemphasis_coefficient=1.0, high_freq=-500.0),
    "full512": dict(ref_mfcc.DEFAULTS, sample_frequency=16000.0, frame_length=32.0, frame_shift=32.0, use_energy=True,
                    raw_energy=False, energy_floor=5e7, window_type="hamming", snip_edges=False, num_mel_bins=40, num_ceps=7),
    "n257": dict(ref_mfcc.DEFAULTS, sample_frequency=11025.0, frame_length=23.4, frame_shift=7.3, use_energy=False,
                 snip_edges=False),
}
EDGE_SIZES = {"wide16ms": (256, 256, 256), "min129": (129, 1, 256), "full512": (512, 512, 512), "n257": (257, 80, 512)}
EDGE_CUT = {"min129": 700}                # at a shift of one sample the utterances are cut to this many samples


def _frame_options(name):
    """What compute-fbank-feats shares with the MFCC edge set `name`: frame, mel bank and energy options."""
    keep = ("sample_frequency", "frame_length", "frame_shift", "preemphasis_coefficient", "remove_dc_offset", "window_type",
            "snip_edges", "num_mel_bins", "low_freq", "high_freq", "raw_energy", "energy_floor")
    return {k: EDGE_CONFIGS[name][k] for k in keep}


FBANK_EDGE_CONFIGS = {
    # the amplitude spectrum on P = 256 with the frame options of wide16ms (one empty filter), the energy in column 0
    "amp256": dict(ref_fbank.DEFAULTS, use_power=False, use_energy=True, **_frame_options("wide16ms")),
    # no log on N = S = 512, with the frame options, the windowed energy and the floor of full512
    "lin512": dict(ref_fbank.DEFAULTS, use_log_fbank=False, **_frame_options("full512")),
}


def edge_batch(name, o):
    """The batch of an edge set: batch(fs), cut where EDGE_CUT says so."""
    cut = EDGE_CUT.get(name)
    return [u[:cut] for u in batch(o["sample_frequency"])]


def tile_base(off, b, run=16):
    """Pure-Python model of the tile map of csrc/mfcc.hip: utterance b owns the tiles base(b) <= w < base(b + 1)."""
    return int(off[b]) // run + b


def tile_cover(off, run=16):
    """(list of (tile, utterance, first frame, frame count) of the busy tiles, number of idle tiles) for frame offsets `off`."""
    B = len(off) - 1
    busy, idle = [], 0
    for b in range(B):
        T = int(off[b + 1]) - int(off[b])
        for w in range(tile_base(off, b, run), tile_base(off, b + 1, run)):
            t0 = (w - tile_base(off, b, run)) * run
            if t0 >= T:
                idle += 1
            else:
                busy.append((w, b, t0, min(run, T - t0)))
    return busy, idle


def grid_lengths(o):
    """Utterance lengths of the many-tile batch: none, one sample, around half a shift, around one frame, and the lengths that
    give exactly 15, 16, 17, 32 and 33 frames under `o` (one below, at and one above a tile, and the same for two tiles)."""
    n, s, _ = ref_mfcc.frame_sizes(o)
    out = [0, 1, 79, 80, 81, 399, 400, 401, 560]
    for t in (15, 16, 17, 32, 33):
        length = n + (t - 1) * s + 7 if o["snip_edges"] else t * s - s // 2 + 7
        assert ref_mfcc.num_frames(length, o) == t
        out.append(length)
    return out


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
