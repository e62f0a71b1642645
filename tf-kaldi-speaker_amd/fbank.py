"""Log mel filterbank features on the GPU (fbank_kernel of csrc/mfcc.hip): the first step of the ResNet recipe
(egs/voxceleb/v3/run.sh:54), `steps/make_fbank.sh --fbank-config fbank.conf` (Kaldi compute-fbank-feats).  Option names and
defaults are Kaldi's; as for the MFCC, --dither defaults to 0 and any other value is refused.  Beside the features the kernel
hands out the per-frame log energy, which a file made with --use-energy=false does not carry and the energy VAD needs.
**parity unpinned**: the algorithm is Kaldi's as published (written out in csrc/mfcc.hip); no Kaldi binary pins it."""
import ctypes as C

from . import _lib
from ._lib import ptr
from .mfcc import FRAME_FIELDS, FrameOptions, packed_offsets


class FbankOptions(FrameOptions):
    FIELDS = dict(FRAME_FIELDS, **{
        "num_mel_bins": (int, 23), "low_freq": (float, 20.0), "high_freq": (float, 0.0), "use_energy": (bool, False),
        "energy_floor": (float, 0.0), "raw_energy": (bool, True), "htk_compat": (bool, False), "use_log_fbank": (bool, True),
        "use_power": (bool, True), "subtract_mean": (bool, False),
    })

    def validate(self):
        self.validate_frame()
        if self.subtract_mean:
            raise ValueError("--subtract-mean=true is not supported")
        if self.num_mel_bins < 3:
            raise ValueError("--num-mel-bins must be at least 3")
        self.validate_sizes()

    @property
    def num_feats(self):
        return self.num_mel_bins + int(self.use_energy)

    def c_struct(self):
        o = _lib.FbankOpts()
        o.struct_size = C.sizeof(_lib.FbankOpts)
        self.frame_fields_into(o)
        o.num_mel_bins, o.low_freq, o.high_freq = self.num_mel_bins, self.low_freq, self.high_freq
        o.use_energy, o.energy_floor, o.raw_energy = int(self.use_energy), self.energy_floor, int(self.raw_energy)
        o.htk_compat, o.use_log_fbank, o.use_power = int(self.htk_compat), int(self.use_log_fbank), int(self.use_power)
        return o


class Fbank(object):
    """Tables of one option set on one device (xv_fbank of include/xvec_hip.h)."""

    def __init__(self, opts, device_index=0):
        self.opts = opts
        self.device_index = int(device_index)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        o = opts.c_struct()
        _lib.check(self._lib.xv_fbank_create(C.byref(o), self.device_index, C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.xv_fbank_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def compute(self, wave_dev, sample_offsets, ld=None, out=None, energy=False):
        """wave_dev: CUDA int16 [samples] (B utterances back to back); sample_offsets: B+1 offsets.
        Returns (CUDA float32 [frames, ld], int32 frame offsets [B+1]) and, with energy=True, the per-frame log energy
        (CUDA float32 [frames]) as a third item."""
        import torch
        sample_offsets, frame_offsets = packed_offsets(self.opts, wave_dev, sample_offsets)
        B, total = len(sample_offsets) - 1, int(frame_offsets[-1])
        nf = self.opts.num_feats
        ld = int(ld or nf)
        if ld < nf:
            raise ValueError("ld %d is smaller than num_feats %d" % (ld, nf))
        dev = wave_dev.device
        if out is None:
            out = torch.zeros((total, ld), dtype=torch.float32, device=dev) if ld > nf else \
                torch.empty((total, ld), dtype=torch.float32, device=dev)
        elif out.shape != (total, ld) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 [%d, %d] tensor" % (total, ld))
        log_e = torch.empty(total, dtype=torch.float32, device=dev) if energy else None
        if total > 0:
            soff_dev = torch.from_numpy(sample_offsets).to(dev)
            foff_dev = torch.from_numpy(frame_offsets).to(dev)
            stream = _lib.stream(dev.index)
            _lib.check(self._lib.xv_fbank_compute(self._h, ptr(wave_dev), ptr(soff_dev),
                                                  ptr(foff_dev), B, ptr(out), ld,
                                                  ptr(log_e) if energy else None, stream))
        return (out, frame_offsets, log_e) if energy else (out, frame_offsets)


_cache = {}


def fbank_packed(wave_dev, sample_offsets, opts, ld=None, energy=False):
    """compute-fbank-feats on a packed batch.  wave_dev: CUDA int16 [samples]; sample_offsets: B+1 offsets; opts: FbankOptions.
    Returns (feats_dev CUDA float32 [frames, ld or num_feats], frame_offsets int32 [B+1]) and, with energy=True, the per-frame
    log energy as a third item."""
    key = (wave_dev.device.index, tuple(sorted(opts.as_dict().items())))
    m = _cache.get(key)
    if m is None:
        if len(_cache) >= 8:
            _cache.clear()
        m = _cache[key] = Fbank(opts, wave_dev.device.index)
    return m.compute(wave_dev, sample_offsets, ld=ld, energy=energy)
