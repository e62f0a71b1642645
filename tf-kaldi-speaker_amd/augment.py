"""Reverberation and additive noise on the GPU (csrc/reverb.hip): the `wav-reverberate ... |` pipelines that stage 2 of the
reference recipes (egs/sre/v1/run.sh:128-170, egs/voxceleb/v2/run_aug.sh) put into wav.scp through Kaldi's
reverberate_data_dir.py and augment_data_dir.py, resolved without a Kaldi installation.

    parse_command(spec)            a wav.scp value -> Plan, or None when it is not a wav-reverberate pipeline
    reverberate_packed(...)        the device call on tensors (xv_reverb of include/xvec_hip.h, which states the rule)
    resolve_batch(specs, fs)       specs -> (int16 CUDA tensor, int64 offsets), every leaf file read once, one device call
    native_batches(items, ...)     the batching loop of compute_mfcc / compute_fbank / extract --native-reverberate
    write_wav(path_or_fd, rate, x) RIFF PCM16 mono

**parity unpinned**: the rule restates wav-reverberate.cc as published; tests/helpers/ref_reverb.py is its float64 oracle.
Out of scope: multi-channel output, resampling, non-PCM16 files, impulse responses above 65536 taps, random selection."""
import ctypes as C
import logging
import os
import shlex
import struct

import numpy as np

from . import _lib
from ._lib import ptr
from .mfcc import _to_bool, read_wav

log = logging.getLogger("xvec.augment")

MAX_TAPS = 65536
STATUS_TEXT = {1: "an additive signal has zero power", 2: "the output has zero power (--normalize-output)"}
_BOOL_WORDS = ("true", "false", "t", "f", "1", "0")

OPTIONS = {
    "impulse_response": str, "additive_signals": str, "snrs": str, "start_times": str,
    "shift_output": bool, "normalize_output": bool, "duration": float, "volume": float,
    "input_wave_channel": int, "rir_channel": int, "noise_channel": int, "multi_channel_output": bool,
}


class Signal(object):
    """One additive signal: a path (or `cmd |`), and the --duration of the nested wav-reverberate pipe it came in (0: none)."""
    __slots__ = ("spec", "duration")

    def __init__(self, spec, duration=0.0):
        self.spec, self.duration = spec, float(duration)

    def __eq__(self, other):
        return isinstance(other, Signal) and (self.spec, self.duration) == (other.spec, other.duration)

    def __repr__(self):
        return "Signal(%r, %r)" % (self.spec, self.duration)


class Plan(object):
    """What one wav-reverberate command line asks for."""
    FIELDS = ("input", "impulse_response", "signals", "snrs", "start_times", "shift_output", "normalize_output", "duration",
              "volume", "input_wave_channel", "rir_channel", "noise_channel")

    def __init__(self, input, impulse_response=None, signals=(), snrs=(), start_times=(), shift_output=True,
                 normalize_output=True, duration=0.0, volume=0.0, input_wave_channel=0, rir_channel=0, noise_channel=0):
        self.input = input
        self.impulse_response = impulse_response
        self.signals = list(signals)
        self.snrs = [float(v) for v in snrs]
        self.start_times = [float(v) for v in start_times]
        self.shift_output, self.normalize_output = bool(shift_output), bool(normalize_output)
        self.duration, self.volume = float(duration), float(volume)
        self.input_wave_channel, self.rir_channel, self.noise_channel = int(input_wave_channel), int(rir_channel), int(noise_channel)
        if not (len(self.signals) == len(self.snrs) == len(self.start_times)):
            raise ValueError("--additive-signals, --snrs and --start-times must have the same number of entries (%d, %d, %d)"
                             % (len(self.signals), len(self.snrs), len(self.start_times)))
        if self.duration < 0 or self.volume < 0:
            raise ValueError("--duration and --volume must not be negative")
        if min(self.input_wave_channel, self.rir_channel, self.noise_channel) < 0:
            raise ValueError("channels must not be negative")

    def as_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def __eq__(self, other):
        return isinstance(other, Plan) and self.as_dict() == other.as_dict()

    def __repr__(self):
        return "Plan(%s)" % ", ".join("%s=%r" % kv for kv in sorted(self.as_dict().items()))


# ------------------------------------------------------------------------------------------------------------ parser
def split_pipeline(text):
    """Split a command line on its top-level `|`: not inside single or double quotes, not after a backslash."""
    parts, cur, quote, i = [], [], None, 0
    while i < len(text):
        ch = text[i]
        if ch == "\\" and quote != "'" and i + 1 < len(text):
            cur.append(text[i:i + 2])
            i += 2
            continue
        if quote:
            if ch == quote:
                quote = None
        elif ch in "'\"":
            quote = ch
        elif ch == "|":
            parts.append("".join(cur))
            cur = []
            i += 1
            continue
        cur.append(ch)
        i += 1
    if quote:
        raise ValueError("unbalanced quote in %r" % text)
    parts.append("".join(cur))
    return parts


def _parse_args(argv, what):
    """`--name=value` / `--name value` options and the positionals of one wav-reverberate command."""
    opts, pos, i = {}, [], 1
    while i < len(argv):
        tok = argv[i]
        i += 1
        if not tok.startswith("--"):
            pos.append(tok)
            continue
        name, eq, value = tok[2:].partition("=")
        key = name.replace("-", "_")
        if key not in OPTIONS:
            raise ValueError("%s: unknown option --%s" % (what, name))
        typ = OPTIONS[key]
        if not eq:
            if typ is bool:
                value = "true"
                if i < len(argv) and argv[i].lower() in _BOOL_WORDS:
                    value = argv[i]
                    i += 1
            elif i < len(argv):
                value = argv[i]
                i += 1
            else:
                raise ValueError("%s: option --%s has no value" % (what, name))
        try:
            opts[key] = _to_bool(value) if typ is bool else typ(value)
        except ValueError:
            raise ValueError("%s: bad value %r for --%s" % (what, value, name))
    return opts, pos


def _parse_signal(entry):
    entry = entry.strip()
    if not entry:
        raise ValueError("empty entry in --additive-signals")
    if not entry.endswith("|"):
        return Signal(entry)
    stages = split_pipeline(entry)
    if len(stages) != 2 or stages[1].strip():
        raise ValueError("an additive signal may be a path or one `wav-reverberate --duration=D path - |`, got %r" % entry)
    argv = shlex.split(stages[0])
    if not argv or os.path.basename(argv[0]) != "wav-reverberate":
        raise ValueError("an additive signal may be a path or one `wav-reverberate --duration=D path - |`, got %r" % entry)
    opts, pos = _parse_args(argv, "nested wav-reverberate")
    if set(opts) != {"duration"} or len(pos) != 2 or pos[1] != "-" or pos[0] == "-" or not opts["duration"] > 0:
        raise ValueError("a nested wav-reverberate may only be `--duration=D path -` with D > 0, got %r" % entry)
    return Signal(pos[0], opts["duration"])


def parse_command(spec):
    """A wav.scp value -> Plan, or None when it is not a pipeline whose last stage is wav-reverberate.  ValueError for a
    wav-reverberate line this module cannot honour."""
    spec = spec.strip()
    if not spec.endswith("|"):
        return None
    try:
        stages = split_pipeline(spec)
    except ValueError:
        return None
    if len(stages) < 2 or stages[-1].strip():
        return None
    try:
        argv = shlex.split(stages[-2])
    except ValueError:
        return None
    if not argv or os.path.basename(argv[0]) != "wav-reverberate":
        return None
    opts, pos = _parse_args(argv, "wav-reverberate")
    if opts.pop("multi_channel_output", False):
        raise ValueError("wav-reverberate: --multi-channel-output=true is not supported")
    if len(pos) != 2:
        raise ValueError("wav-reverberate: expected <input> <output>, got %d positional arguments" % len(pos))
    if pos[1] != "-":
        raise ValueError("wav-reverberate: the output of a pipeline must be `-`, got %r" % pos[1])
    head = [s.strip() for s in stages[:-2]]
    if pos[0] == "-":
        if not head or not all(head):
            raise ValueError("wav-reverberate: the input is `-` but no command feeds it")
        source = " | ".join(head) + " |"
    elif head:
        raise ValueError("wav-reverberate: the input is %r but a command is piped into it" % pos[0])
    else:
        source = pos[0]

    def numbers(key):
        text = opts.pop(key, "").strip()
        try:
            return [float(v) for v in text.split(",")] if text else []
        except ValueError:
            raise ValueError("wav-reverberate: bad list %r for --%s" % (text, key.replace("_", "-")))

    text = opts.pop("additive_signals", "").strip()
    signals = [_parse_signal(e) for e in text.split(",")] if text else []
    snrs, starts = numbers("snrs"), numbers("start_times")
    rir = opts.pop("impulse_response", "").strip() or None
    return Plan(source, rir, signals, snrs, starts, **opts)


# ------------------------------------------------------------------------------------------------------------ wav output
def write_wav(path_or_fd, rate, samples):
    """RIFF PCM16 mono.  path_or_fd: a path, `-` (stdout) or a binary file object."""
    x = np.ascontiguousarray(samples)
    if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError("write_wav takes a 1-D int16 vector")
    body = x.astype("<i2").tobytes()
    head = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, int(rate), 2 * int(rate), 2, 16) \
        + b"data" + struct.pack("<I", len(body))
    if hasattr(path_or_fd, "write"):
        path_or_fd.write(head + body)
    elif path_or_fd == "-":
        import sys
        sys.stdout.buffer.write(head + body)
        sys.stdout.buffer.flush()
    else:
        with open(path_or_fd, "wb") as f:
            f.write(head + body)


# ------------------------------------------------------------------------------------------------------------ device
def tile():
    """(T, C) of the convolution kernel: outputs per workgroup and taps per LDS chunk."""
    t, c = C.c_int(), C.c_int()
    _lib.check(_lib.load().xv_reverb_tile(C.byref(t), C.byref(c)))
    return t.value, c.value


def out_length(n, rir_len, sample_rate, shift_output, duration):
    """n_out of the rule."""
    if duration > 0:
        return int(duration * sample_rate)
    return int(n) if shift_output else int(n) + max(int(rir_len), 1) - 1


def _tables(utts):
    """utts: dicts with wave=(off, len), rir=(off, len) or None, noises=[(off, len, ext_len, snr_db, start_time), ...],
    sample_rate, shift_output, normalize_output, duration, volume -> the two ctypes tables and the output offsets."""
    nn = sum(len(u.get("noises", ())) for u in utts)
    ut = (_lib.ReverbUtt * max(len(utts), 1))()
    nt = (_lib.ReverbNoise * max(nn, 1))()
    offsets, row = [0], 0
    for i, u in enumerate(utts):
        d = ut[i]
        d.wave_off, d.wave_len = int(u["wave"][0]), int(u["wave"][1])
        rir = u.get("rir")
        d.rir_off, d.rir_len = (int(rir[0]), int(rir[1])) if rir else (0, 0)
        d.sample_rate = float(u["sample_rate"])
        d.duration, d.volume = float(u.get("duration", 0.0)), float(u.get("volume", 0.0))
        d.shift_output, d.normalize_output = int(bool(u.get("shift_output", True))), int(bool(u.get("normalize_output", True)))
        d.noise_begin, d.noise_count = row, len(u.get("noises", ()))
        for z in u.get("noises", ()):
            nt[row].off, nt[row].len, nt[row].ext_len = int(z[0]), int(z[1]), int(z[2])
            nt[row].snr_db, nt[row].start_time = float(z[3]), float(z[4])
            row += 1
        d.out_off = offsets[-1]
        d.out_len = out_length(d.wave_len, d.rir_len, d.sample_rate, d.shift_output, d.duration)
        offsets.append(offsets[-1] + max(int(d.out_len), 0))
    return ut, nt, nn, np.asarray(offsets, dtype=np.int64)


def _workspace(lib, ut, B, nt, nn, sizes):
    need = lib.xv_reverb_workspace(ut, B, nt, nn, *sizes)
    if need < 0:
        msg = lib.xv_last_error(None)
        raise ValueError(msg.decode("utf-8", "replace") if msg else "xv_reverb_workspace: %d" % need)
    return int(need)


def workspace_bytes(utts, wave_samples, rir_samples=0, noise_samples=0):
    """Least workspace of reverberate_packed for these tables (validates them: ValueError)."""
    ut, nt, nn, offsets = _tables(utts)
    return _workspace(_lib.load(), ut, len(utts), nt, nn, [int(wave_samples), int(rir_samples), int(noise_samples), int(offsets[-1])])


class Result(object):
    """out_i16 / out_f32: packed CUDA tensors (or None); offsets int64 [B + 1]; status, peak, clipped: int32 numpy [B]."""
    __slots__ = ("out_i16", "out_f32", "offsets", "status", "peak", "clipped")


def reverberate_packed(wave_dev, utts, rir_dev=None, noise_dev=None, want_i16=True, want_f32=False, workspace=None,
                       out_i16=None, out_f32=None, check=True):
    """The device call.  wave_dev / rir_dev / noise_dev: contiguous 1-D int16 CUDA tensors; utts: see _tables.  workspace, out_i16
    and out_f32 may be given (a uint8 tensor of at least the needed bytes, outputs of exactly the packed length).  With
    `check` an utterance whose status is not 0 raises ValueError; the clipped samples are reported in one warning per call."""
    import torch
    lib = _lib.load()
    dev = wave_dev.device
    for t in (wave_dev, rir_dev, noise_dev):
        if t is not None and (t.dtype != torch.int16 or t.dim() != 1 or not t.is_contiguous() or t.device != dev):
            raise ValueError("waves, impulse responses and additive signals must be contiguous 1-D int16 tensors on one device")
    if not utts:
        raise ValueError("reverberate_packed needs at least one utterance")
    ut, nt, nn, offsets = _tables(utts)
    sizes = [int(wave_dev.shape[0]), int(rir_dev.shape[0]) if rir_dev is not None else 0,
             int(noise_dev.shape[0]) if noise_dev is not None else 0, int(offsets[-1])]
    need = _workspace(lib, ut, len(utts), nt, nn, sizes)
    if workspace is None:
        workspace = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dev)
    total = int(offsets[-1])
    if out_i16 is None and want_i16:
        out_i16 = torch.empty(total, dtype=torch.int16, device=dev)
    if out_f32 is None and want_f32:
        out_f32 = torch.empty(total, dtype=torch.float32, device=dev)
    for t, dt in ((out_i16, torch.int16), (out_f32, torch.float32)):
        if t is not None and (t.dtype != dt or t.dim() != 1 or t.shape[0] != total or not t.is_contiguous()):
            raise ValueError("an output must be a contiguous 1-D tensor of %d samples" % total)
    B = len(utts)
    meta = torch.empty((3, B), dtype=torch.int32, device=dev)
    src = lambda t: ptr(t) if t is not None and t.numel() > 0 else None      # noqa: E731
    stream = _lib.stream(dev.index)
    _lib.check(lib.xv_reverb(dev.index, src(wave_dev), sizes[0], src(rir_dev), sizes[1], src(noise_dev), sizes[2], ut, B, nt, nn,
                             ptr(out_i16), ptr(out_f32), total, ptr(meta[0]), ptr(meta[1]), ptr(meta[2]),
                             ptr(workspace), int(workspace.numel()), stream))
    host = meta.cpu().numpy()
    r = Result()
    r.out_i16, r.out_f32, r.offsets = out_i16, out_f32, offsets
    r.status, r.peak, r.clipped = host[0].copy(), host[1].copy(), host[2].copy()
    if check and r.status.any():
        i = int(np.flatnonzero(r.status)[0])
        raise ValueError("utterance %d: %s" % (i, STATUS_TEXT.get(int(r.status[i]), "status %d" % r.status[i])))
    clipped = int(r.clipped.sum(dtype=np.int64))
    if clipped:
        log.warning("[WARNING] clipped %d samples out of total %d in %d utterance(s)", clipped, total, int((r.clipped > 0).sum()))
    return r


# ------------------------------------------------------------------------------------------------------------ files
class BatchBuilder(object):
    """Collects utterances for one device call.  Every leaf file (impulse response, additive signal) is read once."""

    def __init__(self, sample_frequency=None, channel=-1):
        self.fs = float(sample_frequency) if sample_frequency else None
        self.channel = channel
        self.waves, self.utts, self.wave_total = [], [], 0
        self._pools = {"rir": ([], {}, [0]), "noise": ([], {}, [0])}

    def __len__(self):
        return len(self.utts)

    def _rate(self, spec, rate, want):
        if float(rate) != float(want):
            raise ValueError("%s: sample rate %d does not match %g" % (spec, rate, want))

    def _leaf(self, pool, spec, channel, want):
        parts, index, total = self._pools[pool]
        hit = index.get((spec, channel))
        if hit is None:
            rate, x = read_wav(spec, channel)
            if x.shape[0] < 1:
                raise ValueError("%s: no samples" % spec)
            hit = index[(spec, channel)] = (total[0], int(x.shape[0]), rate)
            parts.append(x)
            total[0] += int(x.shape[0])
        self._rate(spec, hit[2], want)
        return hit[0], hit[1]

    def add(self, spec):
        """One wav.scp value: a wav-reverberate pipeline, or a plain path / command (passed through unchanged).
        Raises ValueError / OSError and leaves the batch as it was."""
        plan = parse_command(spec)
        if plan is None:
            rate, x = read_wav(spec, self.channel, self.fs)
            u = {"sample_rate": rate, "shift_output": False, "normalize_output": False}
        else:
            rate, x = read_wav(plan.input, plan.input_wave_channel, self.fs)
            u = {"sample_rate": rate, "shift_output": plan.shift_output, "normalize_output": plan.normalize_output,
                 "duration": plan.duration, "volume": plan.volume}
            if plan.impulse_response:
                u["rir"] = self._leaf("rir", plan.impulse_response, plan.rir_channel, rate)
                if u["rir"][1] > MAX_TAPS:
                    raise ValueError("%s: %d taps, at most %d are supported" % (plan.impulse_response, u["rir"][1], MAX_TAPS))
            u["noises"] = []
            for sig, snr, start in zip(plan.signals, plan.snrs, plan.start_times):
                off, m = self._leaf("noise", sig.spec, plan.noise_channel, rate)
                ext = int(sig.duration * rate) if sig.duration > 0 else m
                if ext < 1:
                    raise ValueError("%s: --duration=%g gives no samples" % (sig.spec, sig.duration))
                if start < 0:
                    raise ValueError("a negative start time (%g) is not supported" % start)
                u["noises"].append((off, m, ext, snr, start))
        if x.shape[0] < 1:
            raise ValueError("%s: no samples" % spec)
        u["wave"] = (self.wave_total, int(x.shape[0]))
        self.waves.append(x)
        self.wave_total += int(x.shape[0])
        self.utts.append(u)

    def run(self, device, check=True):
        """-> Result of reverberate_packed on `device`."""
        import torch

        def up(parts):
            return torch.from_numpy(np.concatenate(parts)).to(device) if parts else None

        return reverberate_packed(up(self.waves), self.utts, up(self._pools["rir"][0]), up(self._pools["noise"][0]), check=check)


def resolve_batch(specs, sample_frequency=None, device="cuda:0", channel=-1):
    """Resolve wav.scp values in one device call: wav-reverberate pipelines by the rule, other values unchanged.
    Returns (int16 CUDA tensor, int64 offsets [B + 1]), ready for mfcc_packed / fbank_packed."""
    b = BatchBuilder(sample_frequency, channel)
    for spec in specs:
        b.add(spec)
    r = b.run(device)
    return r.out_i16, r.offsets


def native_batches(items, opts, batch_samples, channel=-1, on_error=None, device="cuda:0", rates=None):
    """The --native-reverberate twin of mfcc.wav_batches: (key, wav spec) stream -> (keys, int16 CUDA tensor, int64 offsets) per
    batch of about batch_samples input samples.  An utterance that cannot be read or resolved goes to on_error.  `rates`, a dict,
    receives the sample rate of every key."""
    import torch

    def flush(keys, b):
        r = b.run(device, check=on_error is None)
        bad = np.flatnonzero(r.status)
        if not bad.size:
            return keys, r.out_i16, r.offsets
        for i in bad:
            on_error(keys[i], ValueError(STATUS_TEXT.get(int(r.status[i]), "status %d" % r.status[i])))
        keep = [i for i in range(len(keys)) if r.status[i] == 0]
        parts = [r.out_i16[r.offsets[i]:r.offsets[i + 1]] for i in keep]
        off = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in parts])]).astype(np.int64)
        return [keys[i] for i in keep], (torch.cat(parts) if parts else r.out_i16[:0]), off

    keys, b = [], BatchBuilder(opts.sample_frequency, channel)
    for key, spec in items:
        try:
            b.add(spec)
        except (ValueError, OSError) as e:
            if on_error is None:
                raise
            on_error(key, e)
            continue
        keys.append(key)
        if rates is not None:
            rates[key] = int(b.utts[-1]["sample_rate"])
        if b.wave_total >= batch_samples:
            out = flush(keys, b)
            if out[0]:
                yield out
            keys, b = [], BatchBuilder(opts.sample_frequency, channel)
    if keys:
        out = flush(keys, b)
        if out[0]:
            yield out
