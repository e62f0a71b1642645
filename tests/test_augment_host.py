"""Host side of the wav-reverberate route (tf_kaldi_speaker_amd.augment): the parser on the lines reverberate_data_dir.py and
augment_data_dir.py write, its refusals, the float64 oracle's own properties, write_wav, the exported symbols and the table
validation of xv_reverb / xv_reverb_workspace, which runs on the host and launches nothing.  No GPU."""
import ctypes as C
import io
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_reverb as R  # noqa: E402
import reverb_cases as K  # noqa: E402

from tf_kaldi_speaker_amd import augment  # noqa: E402
from tf_kaldi_speaker_amd.augment import Plan, Signal, parse_command  # noqa: E402
from tf_kaldi_speaker_amd.mfcc import parse_wav  # noqa: E402


# ------------------------------------------------------------------------------------------------ parser
def test_reverb_line_of_reverberate_data_dir():
    line = ('wav-reverberate --shift-output=true --impulse-response="sox RIRS_NOISES/simulated_rirs/smallroom/Room001/'
            'Room001-00001.wav -r 8000 -t wav - |" data/swbd/a.wav - |')
    assert parse_command(line) == Plan(
        "data/swbd/a.wav", impulse_response="sox RIRS_NOISES/simulated_rirs/smallroom/Room001/Room001-00001.wav -r 8000 -t wav - |",
        shift_output=True)


def test_foreground_noise_line_with_several_start_times():
    line = ("wav-reverberate --shift-output=true --additive-signals='musan/noise/free-sound/noise-free-sound-0001.wav,"
            "musan/noise/sound-bible/noise-sound-bible-0002.wav,musan/noise/free-sound/noise-free-sound-0003.wav' "
            "--start-times='0,4.25,11.5' --snrs='15,10,0' data/train/utt1.wav - |")
    plan = parse_command(line)
    assert plan.input == "data/train/utt1.wav" and plan.impulse_response is None
    assert plan.signals == [Signal("musan/noise/free-sound/noise-free-sound-0001.wav"),
                            Signal("musan/noise/sound-bible/noise-sound-bible-0002.wav"),
                            Signal("musan/noise/free-sound/noise-free-sound-0003.wav")]
    assert plan.snrs == [15.0, 10.0, 0.0] and plan.start_times == [0.0, 4.25, 11.5]
    assert plan.shift_output and plan.normalize_output and plan.duration == 0.0 and plan.volume == 0.0


def test_background_music_and_babble_lines_with_nested_duration_pipes():
    music = ("wav-reverberate --shift-output=true --additive-signals='wav-reverberate --duration=12.345 "
             "\"musan/music/fma/music-fma-0001.wav\" - |' --start-times='0' --snrs='8' data/train/utt2.wav - |")
    plan = parse_command(music)
    assert plan.signals == [Signal("musan/music/fma/music-fma-0001.wav", 12.345)]
    assert plan.snrs == [8.0] and plan.start_times == [0.0]
    babble = ("wav-reverberate --shift-output=true --additive-signals='wav-reverberate --duration=7.5 \"musan/speech/a.wav\" - |,"
              "wav-reverberate --duration=7.5 \"musan/speech/b.wav\" - |,wav-reverberate --duration=7.5 \"musan/speech/c.wav\" - |' "
              "--start-times='0,0,0' --snrs='17,13,20' data/train/utt3.wav - |")
    plan = parse_command(babble)
    assert plan.signals == [Signal("musan/speech/%s.wav" % c, 7.5) for c in "abc"]
    assert plan.snrs == [17.0, 13.0, 20.0]


def test_sph2pipe_pipeline_keeps_the_stages_before_as_a_command():
    line = ("sph2pipe -f wav -p -c 1 /corpora/sre/x.sph | wav-reverberate --shift-output=true "
            "--impulse-response=\"sox RIRS_NOISES/real_rirs_isotropic_noises/r.wav -r 8000 -t wav - |\" - - |")
    plan = parse_command(line)
    assert plan.input == "sph2pipe -f wav -p -c 1 /corpora/sre/x.sph |"
    assert plan.impulse_response == "sox RIRS_NOISES/real_rirs_isotropic_noises/r.wav -r 8000 -t wav - |"


def test_both_option_spellings_and_every_option():
    a = parse_command("wav-reverberate --shift-output false --normalize-output=false --duration 2.5 --volume=0.3 "
                      "--input-wave-channel=1 --rir-channel 2 --noise-channel=3 --impulse-response r.wav in.wav - |")
    assert a == Plan("in.wav", "r.wav", shift_output=False, normalize_output=False, duration=2.5, volume=0.3,
                     input_wave_channel=1, rir_channel=2, noise_channel=3)
    assert parse_command("wav-reverberate --multi-channel-output=false in.wav - |") == Plan("in.wav")


@pytest.mark.parametrize("line", [
    "a/b.wav",
    "sox a.wav -r 8000 -t wav - |",
    "sph2pipe -f wav -p -c 1 x.sph |",
    "wav-reverberate in.wav out.wav",                       # not a pipe: a path as far as wav.scp goes
    "cat 'wav-reverberate' |",
])
def test_lines_that_are_not_wav_reverberate_pipelines_give_none(line):
    assert parse_command(line) is None


@pytest.mark.parametrize("line,word", [
    ("wav-reverberate --multi-channel-output=true in.wav - |", "multi-channel-output"),
    ("wav-reverberate --frobnicate=3 in.wav - |", "--frobnicate"),
    ("wav-reverberate in.wav out.wav |", "output"),
    ("wav-reverberate in.wav |", "positional"),
    ("wav-reverberate - - |", "no command"),
    ("cat x | wav-reverberate in.wav - |", "piped"),
    ("wav-reverberate --additive-signals='a.wav,b.wav' --snrs='1' --start-times='0,0' in.wav - |", "same number"),
    ("wav-reverberate --additive-signals='a.wav' --snrs='1,2' --start-times='0' in.wav - |", "same number"),
    ("wav-reverberate --additive-signals='wav-reverberate --duration=2 --volume=1 a.wav - |' --snrs='1' --start-times='0' in.wav - |", "nested"),
    ("wav-reverberate --additive-signals='wav-reverberate a.wav - |' --snrs='1' --start-times='0' in.wav - |", "nested"),
    ("wav-reverberate --additive-signals='sox a.wav -t wav - |' --snrs='1' --start-times='0' in.wav - |", "additive signal"),
    ("wav-reverberate --additive-signals='wav-reverberate --duration=2 a.wav out.wav |' --snrs='1' --start-times='0' in.wav - |", "nested"),
    ("wav-reverberate --snrs='x' in.wav - |", "bad list"),
    ("wav-reverberate --duration=abc in.wav - |", "bad value"),
    ("wav-reverberate --duration=-1 in.wav - |", "negative"),
])
def test_refusals_raise_value_error(line, word):
    with pytest.raises(ValueError) as e:
        parse_command(line)
    assert word in str(e.value)


# ------------------------------------------------------------------------------------------------ the oracle against itself
def _signal(n, seed, amp=3000):
    return np.clip(np.random.RandomState(seed).standard_normal(n) * amp, -32768, 32767).astype(np.int16)


def test_oracle_unit_impulse_is_the_identity():
    x = _signal(500, 1)
    r = R.reverberate(x, 16000, h=np.array([32767], dtype=np.int16), normalize_output=True)
    assert r.p == 0 and r.n_out == 500
    assert np.abs(r.out - x).max() < 1e-9                 # 32767 / 32768 x, normalised back to the power of x
    r = R.reverberate(x, 16000, h=None)
    assert np.array_equal(r.out, x.astype(np.float64)) and r.scale == 1.0 and r.E == r.p_before


def test_oracle_shifted_delta_with_shift_output_returns_x():
    x = _signal(700, 2)
    h = np.zeros(40, dtype=np.int16)
    h[23] = 16384
    r = R.reverberate(x, 8000, h=h, shift_output=True)
    assert r.p == 23 and r.n_out == 700
    # 0.5 x, normalised: the power after is taken over all Y = N + L - 1 samples of y, so x comes back times sqrt(Y / N)
    assert np.abs(r.out - x * np.sqrt(739.0 / 700.0)).max() < 1e-9
    r = R.reverberate(x, 8000, h=h, shift_output=True, normalize_output=False)
    assert np.array_equal(r.out, 0.5 * x)
    r = R.reverberate(x, 8000, h=h, shift_output=False, normalize_output=False)
    assert r.n_out == 739 and np.array_equal(r.out[23:723], 0.5 * x) and not r.out[:23].any() and not r.out[723:].any()


def test_oracle_signed_maximum_is_the_peak():
    h = np.array([10, -30000, 200, 200, 5], dtype=np.int16)
    assert R.reverberate(_signal(50, 3), 8000, h=h).p == 2


def test_oracle_duration_without_rir_wraps_x():
    x = _signal(100, 4)
    r = R.reverberate(x, 1000, duration=0.2505)
    assert r.n_out == 250 and np.array_equal(r.out, x[np.arange(250) % 100].astype(np.float64))
    assert R.reverberate(x, 1000, duration=0.03).n_out == 30


def test_oracle_volume_overrides_normalisation_and_normalisation_keeps_the_power():
    x = _signal(900, 5)
    h = _signal(120, 6, 8000)
    noise = [(_signal(300, 7), 5.0, 0.01, 650)]
    r = R.reverberate(x, 8000, h=h, noises=noise, volume=0.25, normalize_output=True)
    assert r.scale == 0.25
    r = R.reverberate(x, 8000, h=h, noises=noise, shift_output=False)
    assert r.n_out == r.Y and abs(np.mean(r.out ** 2) / r.p_before - 1.0) < 1e-12
    with pytest.raises(ValueError):
        R.reverberate(x, 8000, noises=[(np.zeros(10, dtype=np.int16), 5.0, 0.0, None)])
    with pytest.raises(ValueError):
        R.reverberate(np.zeros(10, dtype=np.int16), 8000)


def test_oracle_noise_level_is_the_snr_against_the_early_energy():
    x = _signal(4000, 8)
    v = _signal(4000, 9, 500)
    r0 = R.reverberate(x, 8000, normalize_output=False)
    r = R.reverberate(x, 8000, noises=[(v, 10.0, 0.0, None)], normalize_output=False)
    added = r.out - r0.out
    assert abs(np.mean(added ** 2) / r0.p_before - 0.1) < 1e-12


def test_gpu_cases_keep_the_share_of_samples_too_close_to_a_threshold_under_the_cap():
    """tests/test_gpu_reverb.py sets aside, for the clipped count, the samples whose reference lies within the bound of a
    saturation threshold: at most 1 % of an utterance, from the oracle alone."""
    _built()
    cases = K.all_cases(*augment.tile())
    assert len(cases) > 50
    for c in cases.values():
        r = K.ref(c)
        assert K.close_mask(r).sum() <= K.CLOSE_CAP * max(r.n_out, 1), c["name"]
        assert np.all(np.isfinite(r.bound)), c["name"]
    assert K.ref(cases["emit_volume_saturates"]).clipped > 20


# ------------------------------------------------------------------------------------------------ wav files
def test_write_wav_parse_wav_round_trip(tmp_path):
    x = _signal(1234, 10, 20000)
    buf = io.BytesIO()
    augment.write_wav(buf, 8000, x)
    rate, y = parse_wav(buf.getvalue())
    assert rate == 8000 and np.array_equal(x, y)
    path = str(tmp_path / "a.wav")
    augment.write_wav(path, 16000, x[:1])
    rate, y = parse_wav(open(path, "rb").read())
    assert rate == 16000 and np.array_equal(x[:1], y)
    with pytest.raises(ValueError):
        augment.write_wav(buf, 8000, x.astype(np.float32))


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def _built():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    return g, _lib


def test_reverb_symbols_are_declared_listed_and_exported(repo_root):
    g, _lib = _built()
    assert "reverb.hip" in g.SOURCES
    hdr = open(os.path.join(repo_root, "include", "xvec_hip.h")).read()
    for struct, mirror in (("xv_reverb_utt", _lib.ReverbUtt), ("xv_reverb_noise", _lib.ReverbNoise)):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1))
        fields = []
        for typ, names in re.findall(r"(int64_t|int32_t|double)\s+([^;]+);", body):
            fields += [(n.strip(), {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}[typ]) for n in names.split(",")]
        assert fields == list(mirror._fields_), struct
    t, c = augment.tile()
    assert (t, c) == tuple(int(re.search(r"#define %s (\d+)" % n, hdr).group(1)) for n in ("XV_REVERB_TILE", "XV_REVERB_CHUNK"))
    assert t % 256 == 0 and c % 8 == 0
    # the rule is written out in the header and in the kernel file
    src = open(os.path.join(g.CSRC, "reverb.hip")).read()
    for text in (hdr, src):
        assert "P_before = (sum x^2) / N" in text and "trunc(0.05 fs)" in text


def _good():
    u = {"wave": (0, 1000), "rir": (0, 300), "noises": [(0, 500, 700, 10.0, 0.1)], "sample_rate": 8000.0}
    return [u, {"wave": (1000, 50), "sample_rate": 8000.0, "shift_output": False, "duration": 0.5}]


def _workspace(utts, sizes=None, mutate=None):
    _, _lib = _built()
    lib = _lib.load()
    ut, nt, nn, off = augment._tables(utts)
    if mutate:
        mutate(ut, nt)
    sizes = sizes or (1050, 300, 500, int(off[-1]))
    return lib.xv_reverb_workspace(ut, len(utts), nt, nn, *sizes), (ut, nt, nn, sizes)


def test_workspace_of_a_good_table_and_its_layout_inputs():
    need, _ = _workspace(_good())
    assert need > 4 * (1000 + 300 - 1 + 50)
    # n_out: N with shift_output, trunc(duration fs) with --duration
    _, (ut, _, _, _) = _workspace(_good())
    assert (ut[0].out_len, ut[1].out_len, ut[1].out_off) == (1000, 4000, 1000)


def _set(field, value, row=0, noise=False):
    def f(ut, nt):
        setattr((nt if noise else ut)[row], field, value)
    return f


@pytest.mark.parametrize("mutate,code", [
    (_set("wave_len", 0), -1),
    (_set("wave_len", 2 ** 31), -1),
    (_set("wave_off", 10), -1),                      # runs into the second utterance: offsets must rise
    (_set("wave_off", 900, row=1), -1),
    (_set("wave_len", 51, row=1), -1),               # leaves the buffer
    (_set("rir_len", 65537), -2),
    (_set("rir_len", 301), -1),
    (_set("rir_off", -1), -1),
    (_set("out_len", 999), -1),                      # not the rule's n_out
    (_set("out_off", 5, row=1), -1),                 # overlaps the first output
    (_set("sample_rate", 0.0), -1),
    (_set("sample_rate", float("nan")), -1),
    (_set("duration", -1.0), -1),
    (_set("volume", float("inf")), -1),
    (_set("noise_count", 2), -1),
    (_set("noise_begin", 2, row=1), -1),             # an empty range, but past the end of the table
    (_set("len", 0, noise=True), -1),
    (_set("ext_len", 0, noise=True), -1),
    (_set("ext_len", 2 ** 31, noise=True), -1),
    (_set("off", 1, noise=True), -1),
    (_set("snr_db", float("nan"), noise=True), -1),
    (_set("start_time", -0.5, noise=True), -1),
])
def test_bad_tables_are_errors_not_crashes(mutate, code):
    need, (ut, nt, nn, sizes) = _workspace(_good(), mutate=mutate)
    assert need == code
    _, _lib = _built()
    lib = _lib.load()
    # xv_reverb makes the same checks before it touches the device: the pointers are never followed
    one = C.c_void_p(256)
    rc = lib.xv_reverb(0, one, sizes[0], one, sizes[1], one, sizes[2], ut, 2, nt, nn, one, one, sizes[3], one, one, one, one,
                       1 << 40, None)
    assert rc == code
    assert b"xv_reverb" in lib.xv_last_error(None)


def test_bad_sizes_null_pointers_and_a_small_workspace():
    _, _lib = _built()
    lib = _lib.load()
    need, (ut, nt, nn, sizes) = _workspace(_good())
    assert lib.xv_reverb_workspace(ut, 0, nt, nn, *sizes) == -1
    assert lib.xv_reverb_workspace(None, 2, nt, nn, *sizes) == -1
    assert lib.xv_reverb_workspace(ut, 2, None, nn, *sizes) == -1
    assert lib.xv_reverb_workspace(ut, 2, nt, nn, 1049, *sizes[1:]) == -1
    assert lib.xv_reverb_workspace(ut, 2, nt, nn, *sizes[:3], sizes[3] - 1) == -1
    one = C.c_void_p(256)
    args = lambda **kw: [kw.get("dev", 0), kw.get("waves", one), sizes[0], one, sizes[1], one, sizes[2], ut, 2, nt, nn,  # noqa: E731
                         kw.get("o16", one), kw.get("o32", one), sizes[3], kw.get("status", one), one, one, kw.get("ws", one),
                         kw.get("ws_bytes", need), None]
    assert lib.xv_reverb(*args(ws_bytes=need - 1)) == _lib.XV_ERR_WORKSPACE
    assert lib.xv_reverb(*args(ws=None)) == _lib.XV_ERR_WORKSPACE
    assert lib.xv_reverb(*args(waves=None)) == _lib.XV_ERR_INVALID
    assert lib.xv_reverb(*args(status=None)) == _lib.XV_ERR_INVALID
    assert lib.xv_reverb(*args(o16=None, o32=None)) == _lib.XV_ERR_INVALID
    assert lib.xv_reverb(*args(ws=C.c_void_p(260))) == _lib.XV_ERR_INVALID
    assert lib.xv_reverb_tile(None, None) == _lib.XV_ERR_INVALID
