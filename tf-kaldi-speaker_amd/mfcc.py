"""MFCC features and energy VAD on the GPU (csrc/mfcc.hip): the first step of the reference recipe
(egs/voxceleb/v1/run.sh:57-65), `steps/make_mfcc.sh --mfcc-config conf/mfcc.conf` (Kaldi compute-mfcc-feats) and
`sid/compute_vad_decision.sh` (Kaldi compute-vad-decision).  Option names and defaults are Kaldi's, with one difference:
--dither defaults to 0 here (Kaldi: 1.0, random noise) and any other value is refused, so features are deterministic.
**parity unpinned**: the algorithm is Kaldi's as published (written out in csrc/mfcc.hip); no Kaldi binary pins it."""
import ctypes as C
import io
import struct

import numpy as np

from . import _lib
from ._lib import ptr

WINDOW_TYPES = ("povey", "hamming", "hanning", "rectangular")


def _to_bool(v):
    s = str(v).strip().lower()
    if s in ("true", "t", "1", ""):
        return True
    if s in ("false", "f", "0"):
        return False
    raise ValueError("not a boolean: %r" % v)


class _Options(object):
    """Option set with Kaldi's `--name=value` spelling; FIELDS = {name: (type, default)}."""
    FIELDS = {}

    def __init__(self, **kw):
        for k, (_, default) in self.FIELDS.items():
            setattr(self, k, default)
        for k, v in kw.items():
            self.set(k, v)
        self.validate()

    def set(self, name, value):
        key = name.strip().lstrip("-").replace("-", "_")
        if key not in self.FIELDS:
            raise ValueError("unknown option --%s (known: %s)" % (key.replace("_", "-"),
                                                                 ", ".join("--" + k.replace("_", "-") for k in sorted(self.FIELDS))))
        typ = self.FIELDS[key][0]
        setattr(self, key, _to_bool(value) if typ is bool and not isinstance(value, bool) else typ(value))

    def validate(self):
        pass

    def update_from_config(self, path):
        """Kaldi config file: one `--name=value` per line, `#` comments, blank lines."""
        with open(path, "r") as f:
            for n, line in enumerate(f, 1):
                line = line.split("#", 1)[0].strip()
                if not line:
                    continue
                if not line.startswith("--"):
                    raise ValueError("%s:%d: expected --name=value, got %r" % (path, n, line))
                name, _, value = line[2:].partition("=")
                try:
                    self.set(name, value if _ else "true")
                except ValueError as e:
                    raise ValueError("%s:%d: %s" % (path, n, e))
        self.validate()
        return self

    @classmethod
    def from_config(cls, path):
        return cls().update_from_config(path)

    @classmethod
    def add_arguments(cls, parser):
        for k, (typ, default) in sorted(cls.FIELDS.items()):
            parser.add_argument("--" + k.replace("_", "-"), dest="opt_" + k, default=None, metavar=typ.__name__.upper(),
                                help="Kaldi option (default %s)" % default)

    def update_from_args(self, args):
        for k in self.FIELDS:
            v = getattr(args, "opt_" + k, None)
            if v is not None:
                self.set(k, v)
        self.validate()
        return self

    def as_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}


FRAME_FIELDS = {
    "sample_frequency": (float, 16000.0), "frame_length": (float, 25.0), "frame_shift": (float, 10.0),
    "preemphasis_coefficient": (float, 0.97), "remove_dc_offset": (bool, True), "window_type": (str, "povey"),
    "round_to_power_of_two": (bool, True), "snip_edges": (bool, True), "dither": (float, 0.0),
}


class FrameOptions(_Options):
    """The frame options and geometry compute-mfcc-feats and compute-fbank-feats share (FRAME_FIELDS plus num_mel_bins and
    htk_compat in the subclass's FIELDS)."""

    def validate_frame(self):
        if self.dither != 0.0:
            raise ValueError("--dither=%g is not supported: random dither (Kaldi's default 1.0) is not implemented; "
                             "features here are deterministic, use --dither=0" % self.dither)
        if self.htk_compat:
            raise ValueError("--htk-compat=true is not supported")
        if self.window_type not in WINDOW_TYPES:
            raise ValueError("--window-type must be one of %s" % ", ".join(WINDOW_TYPES))
        if not self.round_to_power_of_two:
            raise ValueError("--round-to-power-of-two=false is not supported")

    def validate_sizes(self):
        if self.num_mel_bins > 64:
            raise ValueError("--num-mel-bins above 64 is not supported")
        if self.padded_length not in (256, 512):
            raise ValueError("frames of %d samples pad to %d: only 256 and 512 are supported" % (self.frame_samples, self.padded_length))

    @property
    def frame_samples(self):
        return int(self.sample_frequency * 0.001 * self.frame_length)

    @property
    def shift_samples(self):
        return int(self.sample_frequency * 0.001 * self.frame_shift)

    @property
    def padded_length(self):
        p = 1
        while p < self.frame_samples:
            p *= 2
        return p

    def num_frames(self, num_samples):
        n, s = self.frame_samples, self.shift_samples
        if self.snip_edges:
            return 0 if num_samples < n else 1 + (num_samples - n) // s
        return (num_samples + s // 2) // s

    def first_sample(self, t):
        """Index of the first sample of frame t (negative indices are reflected)."""
        n, s = self.frame_samples, self.shift_samples
        return t * s + (0 if self.snip_edges else s // 2 - n // 2)

    def frame_fields_into(self, o):
        o.sample_frequency, o.frame_length_ms, o.frame_shift_ms = self.sample_frequency, self.frame_length, self.frame_shift
        o.preemphasis_coefficient = self.preemphasis_coefficient
        o.remove_dc_offset = int(self.remove_dc_offset)
        o.window_type = WINDOW_TYPES.index(self.window_type)
        o.round_to_power_of_two, o.snip_edges, o.dither = int(self.round_to_power_of_two), int(self.snip_edges), self.dither


class MfccOptions(FrameOptions):
    FIELDS = dict(FRAME_FIELDS, **{
        "num_mel_bins": (int, 23), "low_freq": (float, 20.0), "high_freq": (float, 0.0), "num_ceps": (int, 13),
        "cepstral_lifter": (float, 22.0), "use_energy": (bool, True), "energy_floor": (float, 0.0), "raw_energy": (bool, True),
        "htk_compat": (bool, False),
    })

    def validate(self):
        self.validate_frame()
        if self.num_ceps > self.num_mel_bins:
            raise ValueError("--num-ceps=%d exceeds --num-mel-bins=%d" % (self.num_ceps, self.num_mel_bins))
        self.validate_sizes()

    def c_struct(self):
        o = _lib.MfccOpts()
        o.struct_size = C.sizeof(_lib.MfccOpts)
        self.frame_fields_into(o)
        o.num_mel_bins, o.low_freq, o.high_freq, o.num_ceps = self.num_mel_bins, self.low_freq, self.high_freq, self.num_ceps
        o.cepstral_lifter, o.use_energy, o.energy_floor = self.cepstral_lifter, int(self.use_energy), self.energy_floor
        o.raw_energy, o.htk_compat = int(self.raw_energy), int(self.htk_compat)
        return o


class VadOptions(_Options):
    FIELDS = {"vad_energy_threshold": (float, 5.0), "vad_energy_mean_scale": (float, 0.5), "vad_frames_context": (int, 0),
              "vad_proportion_threshold": (float, 0.6)}

    def validate(self):
        if self.vad_frames_context < 0:
            raise ValueError("--vad-frames-context must not be negative")
        if not 0.0 < self.vad_proportion_threshold < 1.0:
            raise ValueError("--vad-proportion-threshold must be inside (0, 1)")


# ------------------------------------------------------------------------------------------------------------ wav input
def parse_wav(data, channel=-1, name="<wav>"):
    """RIFF PCM16 bytes -> (sample rate, int16 vector).  channel -1: the file must be mono; otherwise that channel."""
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("%s: not a RIFF/WAVE file" % name)
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = pos + 8
        if tag == b"fmt ":
            if size < 16:
                raise ValueError("%s: short fmt chunk" % name)
            fmt = struct.unpack("<HHIIHH", data[body:body + 16])
        elif tag == b"data":
            if size in (0, 0xFFFFFFFF) or body + size > len(data):         # streamed output of sox / ffmpeg: data runs to the end
                size = len(data) - body
            pcm = data[body:body + size]
            break
        pos = body + size + (size & 1)
    if fmt is None or pcm is None:
        raise ValueError("%s: no fmt / data chunk" % name)
    audio_format, channels, rate, _, block_align, bits = fmt
    if audio_format != 1 or bits != 16:
        raise ValueError("%s: only 16-bit PCM is supported (format tag %d, %d bits)" % (name, audio_format, bits))
    if channels < 1 or block_align != 2 * channels:
        raise ValueError("%s: inconsistent header (%d channels, block align %d)" % (name, channels, block_align))
    x = np.frombuffer(pcm[:len(pcm) // block_align * block_align], dtype="<i2").reshape(-1, channels)
    if channel < 0:
        if channels != 1:
            raise ValueError("%s has %d channels: pick one with --channel" % (name, channels))
        channel = 0
    if channel >= channels:
        raise ValueError("%s: --channel=%d but the file has %d channel(s)" % (name, channel, channels))
    return int(rate), np.ascontiguousarray(x[:, channel]).astype(np.int16)


def read_wav(spec, channel=-1, sample_frequency=None):
    """The value of a wav.scp line: a path, or a command ending in `|` whose output is the file.  Returns (rate, int16 vector);
    a rate other than sample_frequency (when given) is an error, as in compute-mfcc-feats."""
    spec = spec.strip()
    if spec.endswith("|"):
        from .kaldi_io import popen
        fd = popen(spec[:-1], "rb")
        try:
            data = fd.read()
        finally:
            fd.close()
    else:
        with io.open(spec, "rb") as f:
            data = f.read()
    rate, x = parse_wav(data, channel, spec)
    if sample_frequency is not None and float(rate) != float(sample_frequency):
        raise ValueError("%s: sample rate %d does not match --sample-frequency=%g" % (spec, rate, sample_frequency))
    return rate, x


def read_wav_scp(path):
    """(key, spec) of every line of a wav.scp."""
    with open(path.split(":", 1)[1] if path.startswith("scp:") else path, "r") as f:
        for line in f:
            line = line.strip()
            if line:
                key, _, spec = line.partition(" ")
                yield key, spec.strip()


# ------------------------------------------------------------------------------------------------------------ device
def packed_offsets(opts, wave_dev, sample_offsets):
    """Checks a packed batch (wave_dev: CUDA int16 [samples], sample_offsets: B+1 offsets) against the frame options `opts`.
    Returns (int64 sample offsets, int32 frame offsets [B+1])."""
    import torch
    sample_offsets = np.ascontiguousarray(sample_offsets, dtype=np.int64)
    B = len(sample_offsets) - 1
    if wave_dev.dtype != torch.int16 or not wave_dev.is_contiguous() or wave_dev.dim() != 1:
        raise ValueError("wave_dev must be a contiguous 1-D int16 tensor")
    if B < 0 or sample_offsets[0] != 0 or (np.diff(sample_offsets) < 0).any() or sample_offsets[-1] != wave_dev.shape[0]:
        raise ValueError("sample_offsets must rise from 0 to the number of samples")
    counts = [opts.num_frames(int(n)) for n in np.diff(sample_offsets)]
    total = int(np.sum(counts, dtype=np.int64)) if counts else 0
    if total + B >= 2 ** 31:
        raise ValueError("batch of %d frames is too large: split it" % total)
    return sample_offsets, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


class Mfcc(object):
    """Tables of one option set on one device (xv_mfcc of include/xvec_hip.h)."""

    def __init__(self, opts, device_index=0):
        self.opts = opts
        self.device_index = int(device_index)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        o = opts.c_struct()
        _lib.check(self._lib.xv_mfcc_create(C.byref(o), self.device_index, C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.xv_mfcc_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def compute(self, wave_dev, sample_offsets, ld=None, out=None):
        """wave_dev: CUDA int16 [samples] (B utterances back to back); sample_offsets: B+1 offsets.
        Returns (CUDA float32 [frames, ld], int32 frame offsets [B+1])."""
        import torch
        sample_offsets, frame_offsets = packed_offsets(self.opts, wave_dev, sample_offsets)
        B, total = len(sample_offsets) - 1, int(frame_offsets[-1])
        ld = int(ld or self.opts.num_ceps)
        if ld < self.opts.num_ceps:
            raise ValueError("ld %d is smaller than num_ceps %d" % (ld, self.opts.num_ceps))
        dev = wave_dev.device
        if out is None:
            out = torch.zeros((total, ld), dtype=torch.float32, device=dev) if ld > self.opts.num_ceps else \
                torch.empty((total, ld), dtype=torch.float32, device=dev)
        elif out.shape != (total, ld) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 [%d, %d] tensor" % (total, ld))
        if total == 0:
            return out, frame_offsets
        soff_dev = torch.from_numpy(sample_offsets).to(dev)
        foff_dev = torch.from_numpy(frame_offsets).to(dev)
        stream = _lib.stream(dev.index)
        _lib.check(self._lib.xv_mfcc_compute(self._h, ptr(wave_dev), ptr(soff_dev),
                                             ptr(foff_dev), B, ptr(out), ld,
                                             stream))
        return out, frame_offsets


_cache = {}


def mfcc_packed(wave_dev, sample_offsets, opts, ld=None):
    """compute-mfcc-feats on a packed batch.  wave_dev: CUDA int16 [samples]; sample_offsets: B+1 offsets; opts: MfccOptions.
    Returns (feats_dev CUDA float32 [frames, ld or num_ceps], frame_offsets int32 [B+1])."""
    key = (wave_dev.device.index, tuple(sorted(opts.as_dict().items())))
    m = _cache.get(key)
    if m is None:
        if len(_cache) >= 8:
            _cache.clear()
        m = _cache[key] = Mfcc(opts, wave_dev.device.index)
    return m.compute(wave_dev, sample_offsets, ld=ld)


def vad_packed(feats_dev, frame_offsets, vopts=None):
    """compute-vad-decision on a packed batch: feats_dev CUDA float32 [frames, ld] (column 0 = log energy), frame_offsets B+1.
    Returns vad_dev CUDA float32 [frames] of 0 / 1."""
    import torch
    vopts = vopts or VadOptions()
    lib = _lib.load()
    frame_offsets = np.ascontiguousarray(frame_offsets, dtype=np.int32)
    B = len(frame_offsets) - 1
    if feats_dev.dtype != torch.float32 or feats_dev.dim() != 2 or not feats_dev.is_contiguous():
        raise ValueError("feats_dev must be a contiguous float32 matrix")
    if B < 0 or frame_offsets[0] != 0 or (np.diff(frame_offsets) < 0).any() or frame_offsets[-1] != feats_dev.shape[0]:
        raise ValueError("frame_offsets must rise from 0 to the number of frames")
    dev = feats_dev.device
    vad = torch.empty(int(feats_dev.shape[0]), dtype=torch.float32, device=dev)
    if feats_dev.shape[0] == 0:
        return vad
    foff_dev = torch.from_numpy(frame_offsets).to(dev)
    stream = _lib.stream(dev.index)
    _lib.check(lib.xv_vad_energy(dev.index, ptr(feats_dev), int(feats_dev.shape[1]), ptr(foff_dev),
                                 B, vopts.vad_energy_threshold, vopts.vad_energy_mean_scale, vopts.vad_frames_context,
                                 vopts.vad_proportion_threshold, ptr(vad), stream))
    return vad


def wav_batches(items, opts, batch_samples, channel=-1, on_error=None):
    """Group a (key, wav spec) stream into batches of about batch_samples samples: yields (keys, int16 vector, offsets)."""
    keys, parts, total = [], [], 0
    for key, spec in items:
        try:
            _, x = read_wav(spec, channel, opts.sample_frequency)
        except (ValueError, OSError) as e:
            if on_error is None:
                raise
            on_error(key, e)
            continue
        keys.append(key)
        parts.append(x)
        total += x.shape[0]
        if total >= batch_samples:
            yield keys, np.concatenate(parts), np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
            keys, parts, total = [], [], 0
    if keys:
        yield keys, np.concatenate(parts), np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
