"""Fbank without a GPU: the host side of tf_kaldi_speaker_amd.fbank (options, the recipe's config file), the refusals of
xv_fbank_create, which come before its first HIP call, and the invariants of the float64 oracle tests/helpers/ref_fbank.py
against the MFCC oracle it shares its first steps with."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mfcc_cases  # noqa: E402
import ref_fbank  # noqa: E402
import ref_mfcc  # noqa: E402

from tf_kaldi_speaker_amd import fbank as F  # noqa: E402

V3_CONF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fbank_v3.conf")


def test_the_recipe_config():
    raw = open(V3_CONF, "rb").read()
    assert b"#" in raw and not raw.endswith(b"\n")            # trailing comments and no final newline: the reader survives both
    o = F.FbankOptions.from_config(V3_CONF)
    assert (o.window_type, o.num_mel_bins, o.low_freq, o.high_freq) == ("hamming", 40, 20.0, 7600.0)
    assert o.snip_edges is False and o.use_energy is False and o.num_feats == 40
    assert (o.frame_samples, o.shift_samples, o.padded_length) == (400, 160, 512)
    assert [o.num_frames(n) for n in (0, 100, 400, 16123)] == [ref_mfcc.num_frames(n, ref_fbank.V3) for n in (0, 100, 400, 16123)]
    assert {k: v for k, v in o.as_dict().items() if k in ref_fbank.V3} == ref_fbank.V3


def test_defaults_and_the_energy_column():
    o = F.FbankOptions()
    assert o.use_energy is False and o.num_feats == 23 and o.use_log_fbank and o.use_power and o.window_type == "povey"
    assert {k: v for k, v in o.as_dict().items() if k in ref_fbank.DEFAULTS} == ref_fbank.DEFAULTS
    assert F.FbankOptions(use_energy=True).num_feats == 24
    assert F.FbankOptions(**ref_fbank.ENERGY8K).num_feats == 65 == ref_fbank.num_feats(ref_fbank.ENERGY8K)
    assert F.FbankOptions(**ref_fbank.ENERGY8K).padded_length == 256
    s = o.c_struct()
    assert s.struct_size == 19 * 4 and (s.use_energy, s.use_log_fbank, s.use_power, s.num_mel_bins) == (0, 1, 1, 23)


def test_options_from_the_command_line():
    import argparse
    parser = argparse.ArgumentParser()
    F.FbankOptions.add_arguments(parser)
    args = parser.parse_args(["--num-mel-bins=40", "--use-power=false", "--use-energy", "true"])
    o = F.FbankOptions.from_config(V3_CONF).update_from_args(args)
    assert (o.num_mel_bins, o.use_power, o.use_energy, o.window_type, o.num_feats) == (40, False, True, "hamming", 41)


@pytest.mark.parametrize("text,word", [
    ("--htk-compat=true\n", "htk-compat"), ("--dither=1.0\n", "dither"), ("--round-to-power-of-two=false\n", "round-to-power-of-two"),
    ("--frame-length=50\n", "512"), ("--frame-length=5\n--frame-shift=2\n", "256"), ("--num-mel-bins=80\n", "above 64"),
    ("--subtract-mean=true\n", "subtract-mean"), ("--window-type=blackman\n", "window-type"), ("--num-ceps=13\n", "unknown option"),
    ("--num-mel-bins=2\n", "num-mel-bins")])
def test_refused_options(tmp_path, text, word):
    p = tmp_path / "fbank.conf"
    p.write_text(text)
    with pytest.raises(ValueError) as e:
        F.FbankOptions.from_config(str(p))
    assert word in str(e.value)


@pytest.mark.parametrize("kw", [{"htk_compat": True}, {"dither": 0.5}, {"round_to_power_of_two": False}, {"frame_length": 50.0},
                                {"num_mel_bins": 80}])
def test_refusals_use_the_mfcc_messages(kw):
    from tf_kaldi_speaker_amd import mfcc as M
    msgs = []
    for cls in (M.MfccOptions, F.FbankOptions):
        with pytest.raises(ValueError) as e:
            cls(**kw)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]


def test_create_refuses_what_it_cannot_honour():
    """The option checks of xv_fbank_create come before its first HIP call, so they can be exercised without a GPU; the
    messages are the ones xv_mfcc_create gives."""
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib, mfcc as M
    lib = _lib.load()

    def create(fn, o, kw):
        for k, v in kw.items():
            setattr(o, k, v)
        h = ctypes.c_void_p()
        rc = fn(ctypes.byref(o), 0, ctypes.byref(h))
        assert not h.value
        return rc, (lib.xv_last_error(None) or b"").decode()

    for kw, code, word in (({"dither": 1.0}, _lib.XV_ERR_UNSUPPORTED, "dither"), ({"htk_compat": 1}, _lib.XV_ERR_UNSUPPORTED, "htk-compat"),
                           ({"frame_length_ms": 50.0}, _lib.XV_ERR_UNSUPPORTED, "1024"), ({"frame_length_ms": 5.0, "frame_shift_ms": 2.5}, _lib.XV_ERR_UNSUPPORTED, "128"),
                           ({"frame_shift_ms": 30.0}, _lib.XV_ERR_UNSUPPORTED, "frame shift"),
                           ({"num_mel_bins": 65}, _lib.XV_ERR_UNSUPPORTED, "num-mel-bins"), ({"num_mel_bins": 2}, _lib.XV_ERR_UNSUPPORTED, "num-mel-bins"),
                           ({"high_freq": 9000.0}, _lib.XV_ERR_INVALID, "high-freq"),
                           ({"round_to_power_of_two": 0}, _lib.XV_ERR_UNSUPPORTED, "power-of-two")):
        rc, msg = create(lib.xv_fbank_create, F.FbankOptions().c_struct(), kw)
        assert rc == code and word in msg, (kw, rc, msg)
        rc2, msg2 = create(lib.xv_mfcc_create, M.MfccOptions().c_struct(), dict(kw, num_ceps=2) if kw.get("num_mel_bins") == 2 else kw)
        assert rc2 == rc and msg2.split(": ", 1)[1] == msg.split(": ", 1)[1], (kw, msg, msg2)
    rc, msg = create(lib.xv_fbank_create, F.FbankOptions().c_struct(), {"struct_size": 8})
    assert rc == _lib.XV_ERR_INVALID and "struct_size" in msg
    # null pointers, and what needs a handle: refused before any HIP call as well
    h = ctypes.c_void_p()
    assert lib.xv_fbank_create(None, 0, ctypes.byref(h)) == _lib.XV_ERR_INVALID
    assert lib.xv_fbank_compute(None, None, None, None, 1, None, 40, None, None) == _lib.XV_ERR_INVALID
    assert lib.xv_fbank_num_feats(None) == _lib.XV_ERR_INVALID
    assert lib.xv_fbank_num_frames(None, 100) == _lib.XV_ERR_INVALID


# ------------------------------------------------------------------------------------------------ the oracle's own invariants
@pytest.mark.parametrize("name", sorted(ref_fbank.CONFIGS))
def test_oracle_shapes_and_zero_frame_utterances(name):
    o = ref_fbank.CONFIGS[name]
    for x in mfcc_cases.batch(o["sample_frequency"]):
        for dtype in (np.float64, np.float32):
            feats, log_e = ref_fbank.fbank(x, o, dtype=dtype)
            t = ref_mfcc.num_frames(len(x), o)
            assert feats.shape == (t, ref_fbank.num_feats(o)) and log_e.shape == (t,)
            assert feats.dtype == dtype and log_e.dtype == dtype and np.isfinite(feats).all()
    assert ref_fbank.fbank(np.zeros(100, np.int16), ref_fbank.DEFAULTS)[0].shape == (0, 23)           # snip-edges: no frame
    assert ref_fbank.fbank(np.zeros(100, np.int16), ref_fbank.ENERGY8K)[0].shape == (0, 65)


@pytest.mark.parametrize("name", ["v3", "kaldi_defaults"])
def test_log_mel_block_is_the_mfcc_oracles(name):
    o = ref_fbank.CONFIGS[name]
    mo = dict({k: v for k, v in o.items() if k in ref_mfcc.DEFAULTS}, num_ceps=13, cepstral_lifter=22.0, use_energy=True)
    for x in mfcc_cases.batch(o["sample_frequency"]):
        feats, log_e = ref_fbank.fbank(x, o)
        if feats.shape[0] == 0:
            continue
        assert np.array_equal(feats, ref_mfcc.mfcc(x, mo, return_mel=True))
        assert np.array_equal(log_e, ref_mfcc.mfcc(x, mo)[:, 0])


def test_energy_is_column_0_of_the_mfcc_oracle_under_every_energy_option():
    o = ref_fbank.ENERGY8K
    mo = dict({k: v for k, v in o.items() if k in ref_mfcc.DEFAULTS}, num_ceps=13, cepstral_lifter=22.0)
    assert (mo["use_energy"], mo["raw_energy"], mo["energy_floor"], mo["sample_frequency"]) == (True, False, 1.0, 8000.0)
    floored = 0
    for x in mfcc_cases.batch(8000.0):
        feats, log_e = ref_fbank.fbank(x, o)
        want = ref_mfcc.mfcc(x, mo)[:, 0]
        assert np.array_equal(log_e, want) and np.array_equal(feats[:, 0], want)
        floored += int((log_e == 0.0).sum())
        # the side energy does not depend on --use-energy
        assert np.array_equal(ref_fbank.fbank(x, dict(o, use_energy=False))[1], log_e)
        assert np.array_equal(ref_fbank.fbank(x, dict(o, use_energy=False))[0], feats[:, 1:])
    assert floored >= 10                                        # the constant half sits on the floor log(1.0) = 0


def test_linear_output_is_the_exponential_of_the_log_output():
    for x in mfcc_cases.batch(16000.0)[2:6]:
        lin = ref_fbank.fbank(x, ref_fbank.LINEAR)[0]
        log = ref_fbank.fbank(x, ref_fbank.V3)[0]
        assert (lin > ref_fbank.FLT_EPSILON).all() and np.abs(np.log(lin) - log).max() < 1e-12


@pytest.mark.parametrize("name", ["v3", "energy8k"])
def test_amplitude_spectrum_keeps_the_peak_of_a_pure_tone(name):
    o = dict(ref_fbank.CONFIGS[name], use_energy=False, preemphasis_coefficient=0.0)
    fs, m = o["sample_frequency"], o["num_mel_bins"]
    high = o["high_freq"] if o["high_freq"] > 0 else fs / 2 + o["high_freq"]
    points = ref_mfcc.mel(o["low_freq"]) + (ref_mfcc.mel(high) - ref_mfcc.mel(o["low_freq"])) / (m + 1) * np.arange(m + 2)
    for b in (3, m // 2, m - 3):
        f = 700.0 * (np.exp(points[b + 1] / 1127.0) - 1.0)
        x = np.round(8000.0 * np.sin(2 * np.pi * f * np.arange(4000) / fs)).astype(np.int16)
        power = ref_fbank.fbank(x, dict(o, use_power=True))[0]
        amplitude = ref_fbank.fbank(x, dict(o, use_power=False))[0]
        assert (np.argmax(amplitude, axis=1) == np.argmax(power, axis=1)).all(), (name, b)
        if name == "v3":                                         # (64 filters on 128 bins are too narrow to name the bin)
            assert (np.argmax(power, axis=1) == b).all(), (name, b)
        assert (amplitude.max(axis=1) < power.max(axis=1)).all()          # log of a root: half the log, roughly
