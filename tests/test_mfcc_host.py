"""MFCC / energy VAD without a GPU: the definition (frame geometry, known answers) on the float64 oracle
tests/helpers/ref_mfcc.py and on the host side of tf_kaldi_speaker_amd.mfcc (options, config files, wav reader), plus the
refusals of xv_mfcc_create, which come before its first HIP call."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mfcc_cases  # noqa: E402
import ref_mfcc  # noqa: E402

from tf_kaldi_speaker_amd import mfcc as M  # noqa: E402

EPS = float(np.finfo(np.float32).eps)
LENGTHS = [0, 100, 399, 400, 401, 560, 4000]


@pytest.mark.parametrize("snip,expect", [(True, [0, 0, 0, 1, 1, 2, 23]), (False, [0, 1, 2, 3, 3, 4, 25])])
def test_frame_counts_and_first_samples(snip, expect):
    o = dict(ref_mfcc.DEFAULTS, snip_edges=snip)
    po = M.MfccOptions(snip_edges=snip)
    assert ref_mfcc.frame_sizes(o) == (400, 160, 512)
    assert (po.frame_samples, po.shift_samples, po.padded_length) == (400, 160, 512)
    for L, T in zip(LENGTHS, expect):
        assert ref_mfcc.num_frames(L, o) == T, L
        assert po.num_frames(L) == T, L
        idx = ref_mfcc.frame_indices(L, o)
        assert idx.shape == (T, 400)
        if T:
            assert idx.min() >= 0 and idx.max() < L
        for t in range(T):
            first = t * 160 if snip else t * 160 - 120
            assert po.first_sample(t) == first
            if first >= 0:
                assert idx[t, 0] == first
            else:
                assert idx[t, 0] == -first - 1 or L < -first      # one reflection unless the utterance is shorter than that
            assert ref_mfcc.mfcc(np.zeros(L, np.int16), o).shape == (T, 13)


def test_short_utterance_is_reflected_repeatedly():
    """L = 100 without snip_edges: one frame of 400 samples starting at -120, every index folded back into [0, 100)."""
    o = dict(ref_mfcc.DEFAULTS, snip_edges=False)
    idx = ref_mfcc.frame_indices(100, o)
    assert idx.shape == (1, 400)
    assert idx[0, 0] == 80                      # -120 -> 119 -> 80
    assert idx[0, 120] == 0 and idx[0, 219] == 99 and idx[0, 220] == 99 and idx[0, 319] == 0 and idx[0, 320] == 0
    assert idx[0, 399] == 79                    # 279 -> -80 -> 79


@pytest.mark.parametrize("name", sorted(mfcc_cases.CONFIGS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constant_signal_known_answer(name, dtype):
    o = mfcc_cases.CONFIGS[name]
    x = np.full(3000, 1234, np.int16)
    row = np.zeros(o["num_ceps"])
    row[0] = np.log(EPS)
    got = ref_mfcc.mfcc(x, o, dtype=dtype)
    assert got.shape[0] == ref_mfcc.num_frames(3000, o) > 0
    tol = 1e-9 if dtype == np.float64 else 1e-3
    assert np.abs(got - row).max() <= tol
    row[0] = np.sqrt(o["num_mel_bins"]) * np.log(EPS)
    got = ref_mfcc.mfcc(x, dict(o, use_energy=False), dtype=dtype)
    assert np.abs(got - row).max() <= tol * 10


@pytest.mark.parametrize("name", sorted(mfcc_cases.CONFIGS))
def test_pure_tone_peaks_in_its_mel_bin(name):
    o = mfcc_cases.CONFIGS[name]
    fs, m = o["sample_frequency"], o["num_mel_bins"]
    high = o["high_freq"] if o["high_freq"] > 0 else fs / 2 + o["high_freq"]
    points = ref_mfcc.mel(o["low_freq"]) + (ref_mfcc.mel(high) - ref_mfcc.mel(o["low_freq"])) / (m + 1) * np.arange(m + 2)
    for b in (3, m // 2, m - 3):
        f = 700.0 * (np.exp(points[b + 1] / 1127.0) - 1.0)
        x = np.round(8000.0 * np.sin(2 * np.pi * f * np.arange(4000) / fs)).astype(np.int16)
        log_mel = ref_mfcc.mfcc(x, dict(o, preemphasis_coefficient=0.0), return_mel=True)
        assert (np.argmax(log_mel, axis=1) == b).all(), (name, b)


def test_mel_bank_shape_and_dct_rows():
    for o in mfcc_cases.CONFIGS.values():
        w = ref_mfcc.mel_bank(o)
        assert w.shape == (o["num_mel_bins"], ref_mfcc.frame_sizes(o)[2] // 2)
        assert (w >= 0).all() and (w <= 1).all() and (w.sum(axis=1) > 0).all()
        first = np.array([np.flatnonzero(r)[0] for r in w])
        assert (np.diff(first) >= 0).all()
        d = ref_mfcc.dct_matrix(o["num_mel_bins"], o["num_mel_bins"])
        assert np.abs(d @ d.T - np.eye(o["num_mel_bins"])).max() < 1e-12
        assert np.allclose(d[0], np.sqrt(1.0 / o["num_mel_bins"]))
    assert abs(ref_mfcc.lifter(ref_mfcc.DEFAULTS)[11] - 12.0) < 1e-12       # 1 + 11 sin(pi / 2)


def test_vad_on_a_hand_made_energy_track():
    # mean 4 -> threshold 5 + 0.5 * 4 = 7; frames above it: 2, 3, 5
    e = np.array([1.0, 1.0, 10.0, 10.0, 1.0, 10.0, 1.0, 1.0, 1.0, 4.0])
    assert e.mean() == 4.0
    feats = np.stack([e, np.zeros_like(e)], axis=1)
    assert ref_mfcc.vad_threshold(feats) == 7.0
    above = (e > 7.0).astype(np.float32)
    assert (ref_mfcc.vad(feats) == above).all()                              # context 0: the frame itself
    # context 2, proportion 0.6: window counts 3 4 5 5 5 5 5 5 4 3 (clipped at both ends); voiced counts 1 2 2 3 3 2 1 1 0 0
    got = ref_mfcc.vad(feats, dict(vad_frames_context=2, vad_proportion_threshold=0.6))
    # 3 of 5 is exactly 0.6 * 5: voiced (>=); 2 of 4 and 1 of 3 are not
    assert got.tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 0, 0]
    got = ref_mfcc.vad(feats, dict(vad_frames_context=2, vad_proportion_threshold=0.5))
    assert got.tolist() == [0, 1, 0, 1, 1, 0, 0, 0, 0, 0]                    # 2 of 4 is exactly 0.5 * 4
    got = ref_mfcc.vad(feats, ref_mfcc.VAD_VOXCELEB)                         # any voiced frame in the window
    assert got.tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    assert ref_mfcc.vad(np.zeros((0, 3))).shape == (0,)


def test_config_parsing(tmp_path):
    p = tmp_path / "mfcc.conf"
    p.write_text("# voxceleb\n--sample-frequency=16000\n--frame-length=25 # ms\n\n--low-freq=20\n--high-freq=7600\n"
                 "--num-mel-bins=30\n--num-ceps=30\n--snip-edges=false\n")
    o = M.MfccOptions.from_config(str(p))
    assert (o.num_mel_bins, o.num_ceps, o.snip_edges, o.high_freq, o.dither) == (30, 30, False, 7600.0, 0.0)
    want = dict(ref_mfcc.VOXCELEB, round_to_power_of_two=True, dither=0.0, htk_compat=False)
    assert o.as_dict() == want
    p.write_text(mfcc_cases.config_text(ref_mfcc.SRE))
    assert M.MfccOptions.from_config(str(p)).as_dict() == dict(ref_mfcc.SRE, round_to_power_of_two=True, dither=0.0, htk_compat=False)
    v = tmp_path / "vad.conf"
    v.write_text("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n--vad-proportion-threshold=0.12\n--vad-frames-context=2\n")
    assert M.VadOptions.from_config(str(v)).as_dict() == ref_mfcc.VAD_VOXCELEB
    assert M.VadOptions().as_dict() == ref_mfcc.VAD_DEFAULTS
    assert {k: v for k, v in M.MfccOptions().as_dict().items() if k in ref_mfcc.DEFAULTS} == ref_mfcc.DEFAULTS
    for text, word in (("--num-mel-bin=30\n", "unknown option"), ("--htk-compat=true\n", "htk-compat"), ("--dither=1.0\n", "dither"),
                       ("--dither=0.5\n", "dither"), ("--num-ceps=40\n", "num-ceps"), ("--frame-length=50\n", "512"),
                       ("--window-type=blackman\n", "window-type"), ("num-ceps=3\n", "expected --name=value"),
                       ("--vad-energy-threshold=5\n", "unknown option")):
        p.write_text(text)
        with pytest.raises(ValueError) as e:
            M.MfccOptions.from_config(str(p))
        assert word in str(e.value), text
    p.write_text("--dither=0\n--htk-compat=false\n--window-type=hamming\n")
    assert M.MfccOptions.from_config(str(p)).window_type == "hamming"


def _write_wav(path, x, rate=16000, width=2):
    x = np.asarray(x)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if x.ndim == 1 else x.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(x.astype("<i2" if width == 2 else "u1").tobytes())


def test_wav_reader(tmp_path):
    x = mfcc_cases.signal(1234, 16000.0, seed=1)
    _write_wav(tmp_path / "a.wav", x)
    rate, got = M.read_wav(str(tmp_path / "a.wav"))
    assert rate == 16000 and got.dtype == np.int16 and (got == x).all()
    rate, got = M.read_wav("cat %s |" % (tmp_path / "a.wav"), sample_frequency=16000.0)
    assert rate == 16000 and (got == x).all()
    with pytest.raises(ValueError, match="sample rate"):
        M.read_wav(str(tmp_path / "a.wav"), sample_frequency=8000.0)
    st = np.stack([x, -x], axis=1)
    _write_wav(tmp_path / "st.wav", st)
    with pytest.raises(ValueError, match="--channel"):
        M.read_wav(str(tmp_path / "st.wav"))
    assert (M.read_wav(str(tmp_path / "st.wav"), channel=0)[1] == x).all()
    assert (M.read_wav(str(tmp_path / "st.wav"), channel=1)[1] == -x).all()
    with pytest.raises(ValueError, match="--channel=2"):
        M.read_wav(str(tmp_path / "st.wav"), channel=2)
    _write_wav(tmp_path / "u8.wav", np.arange(100) % 200, width=1)
    with pytest.raises(ValueError, match="16-bit PCM"):
        M.read_wav(str(tmp_path / "u8.wav"))
    (tmp_path / "junk.wav").write_bytes(b"not a wav file at all")
    with pytest.raises(ValueError, match="RIFF"):
        M.read_wav(str(tmp_path / "junk.wav"))
    (tmp_path / "wav.scp").write_text("u1 %s\nu2 cat %s |\n" % (tmp_path / "a.wav", tmp_path / "a.wav"))
    items = list(M.read_wav_scp("scp:" + str(tmp_path / "wav.scp")))
    assert items == [("u1", str(tmp_path / "a.wav")), ("u2", "cat %s |" % (tmp_path / "a.wav"))]
    batches = list(M.wav_batches(items, M.MfccOptions(), batch_samples=2000))
    assert len(batches) == 1 and batches[0][0] == ["u1", "u2"] and batches[0][2].tolist() == [0, 1234, 2468]
    assert len(list(M.wav_batches(items, M.MfccOptions(), batch_samples=1000))) == 2


def test_create_refuses_what_it_cannot_honour():
    """The option checks of xv_mfcc_create come before its first HIP call, so they can be exercised without a GPU."""
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()

    def create(**kw):
        o = M.MfccOptions().c_struct()
        for k, v in kw.items():
            setattr(o, k, v)
        h = ctypes.c_void_p()
        rc = lib.xv_mfcc_create(ctypes.byref(o), 0, ctypes.byref(h))
        assert not h.value
        return rc, (lib.xv_last_error(None) or b"").decode()

    for kw, code, word in (({"dither": 1.0}, _lib.XV_ERR_UNSUPPORTED, "dither"), ({"htk_compat": 1}, _lib.XV_ERR_UNSUPPORTED, "htk-compat"),
                           ({"frame_length_ms": 50.0}, _lib.XV_ERR_UNSUPPORTED, "1024"), ({"frame_length_ms": 5.0, "frame_shift_ms": 2.5}, _lib.XV_ERR_UNSUPPORTED, "128"),
                           ({"frame_shift_ms": 30.0}, _lib.XV_ERR_UNSUPPORTED, "frame shift"),
                           ({"num_mel_bins": 65, "num_ceps": 13}, _lib.XV_ERR_UNSUPPORTED, "num-mel-bins"),
                           ({"num_ceps": 24}, _lib.XV_ERR_INVALID, "num-ceps"), ({"high_freq": 9000.0}, _lib.XV_ERR_INVALID, "high-freq"),
                           ({"round_to_power_of_two": 0}, _lib.XV_ERR_UNSUPPORTED, "power-of-two"), ({"struct_size": 8}, _lib.XV_ERR_INVALID, "struct_size")):
        rc, msg = create(**kw)
        assert rc == code and word in msg, (kw, rc, msg)


# ------------------------------------------------------------------------- what tests/test_gpu_frontend_edges.py stands on
@pytest.mark.parametrize("proportion,above,voiced", [(0.6, 15, 0.0), (0.28, 7, 1.0), (0.56, 14, 1.0)])
def test_vad_decides_exact_counts_in_float_as_kaldi_does(proportion, above, voiced):
    """A full window of 25 frames (context 12): the only window sizes up to 41 and proportions 0.01 .. 0.99 at which the float
    product window * proportion lands on the other side of the count than the double product does."""
    e = np.full(25, 4.0)
    e[np.arange(above) * 25 // above] = 6.0                            # spread over the window; the constant threshold is 5
    assert int((e > 5.0).sum()) == above
    o = dict(vad_energy_threshold=5.0, vad_energy_mean_scale=0.0, vad_frames_context=12, vad_proportion_threshold=proportion)
    got = ref_mfcc.vad(e[:, None], o)
    assert got[12] == voiced
    assert (above >= 25 * proportion) != bool(voiced)                   # the double comparison says the opposite
    assert (np.float32(above) >= np.float32(25) * np.float32(proportion)) == bool(voiced)
    # one frame more (less) above the threshold and both comparisons agree again
    e2 = e.copy()
    e2[np.flatnonzero(e2 < 5.0 if not voiced else e2 > 5.0)[0]] = 6.0 if not voiced else 4.0
    assert ref_mfcc.vad(e2[:, None], o)[12] == 1.0 - voiced


def test_float_and_double_vad_comparisons_differ_in_three_places_only():
    differ = []
    for p in range(1, 100):
        for w in range(1, 42):
            for c in range(w + 1):
                if (np.float32(c) >= np.float32(w) * np.float32(p / 100.0)) != (c >= w * (p / 100.0)):
                    differ.append((p, w, c))
    assert differ == [(28, 25, 7), (56, 25, 14), (60, 25, 15)]


@pytest.mark.parametrize("name", sorted(mfcc_cases.EDGE_CONFIGS))
def test_edge_sets_have_the_sizes_they_are_named_for(name):
    o = mfcc_cases.EDGE_CONFIGS[name]
    po = M.MfccOptions(**o)
    assert ref_mfcc.frame_sizes(o) == mfcc_cases.EDGE_SIZES[name]
    assert (po.frame_samples, po.shift_samples, po.padded_length) == mfcc_cases.EDGE_SIZES[name]
    assert {k: v for k, v in po.as_dict().items() if k in o} == o
    counts = [ref_mfcc.num_frames(len(u), o) for u in mfcc_cases.edge_batch(name, o)]
    assert sum(counts) > 40 and max(counts) < 600


def test_edge_sets_cover_every_option_value_between_them():
    sets = list(mfcc_cases.EDGE_CONFIGS.values())
    seen = lambda key: {o[key] for o in sets}                                                             # noqa: E731
    assert {"hanning", "rectangular", "hamming"} <= seen("window_type")
    assert {0.0, 1.0} <= seen("preemphasis_coefficient")
    assert seen("remove_dc_offset") == {True, False} and seen("raw_energy") == {True, False}
    assert seen("use_energy") == {True, False} and seen("snip_edges") == {True, False}
    assert 0.0 in seen("cepstral_lifter") and 0.0 in seen("low_freq") and min(seen("high_freq")) < 0
    assert {3, 64} <= seen("num_mel_bins") and max(seen("energy_floor")) > 0
    assert any(s == n for n, s, _ in mfcc_cases.EDGE_SIZES.values()) and any(s == 1 for _, s, _ in mfcc_cases.EDGE_SIZES.values())
    assert {n for n, _, _ in mfcc_cases.EDGE_SIZES.values()} == {129, 256, 257, 512}
    assert any(n % 2 and s % 2 == 0 and n > 129 for n, s, _ in mfcc_cases.EDGE_SIZES.values())
    import ref_fbank
    f = mfcc_cases.FBANK_EDGE_CONFIGS
    assert not f["amp256"]["use_power"] and ref_mfcc.frame_sizes(f["amp256"])[2] == 256
    assert not f["lin512"]["use_log_fbank"] and ref_mfcc.frame_sizes(f["lin512"]) == (512, 512, 512)
    for o in f.values():
        assert set(o) == set(ref_fbank.DEFAULTS)


def test_wide16ms_has_a_mel_filter_without_an_fft_bin():
    w = ref_mfcc.mel_bank(mfcc_cases.EDGE_CONFIGS["wide16ms"])
    assert w.shape == (64, 128)
    empty = int((w.sum(axis=1) == 0).sum())
    assert empty >= 1
    for name in ("min129", "full512", "n257"):
        assert (ref_mfcc.mel_bank(mfcc_cases.EDGE_CONFIGS[name]).sum(axis=1) > 0).all()
    # such a filter gives log(FLT_EPSILON) on every frame
    x = mfcc_cases.signal(2000, 16000.0, seed=3)
    log_mel = ref_mfcc.mfcc(x, mfcc_cases.EDGE_CONFIGS["wide16ms"], return_mel=True)
    assert int((log_mel == np.log(EPS)).all(axis=0).sum()) == empty


def test_full512_energy_floor_splits_the_batch():
    """From the oracle alone: windowed energies of the batch on both sides of the floor, none within 1e-3 of it."""
    o = mfcc_cases.EDGE_CONFIGS["full512"]
    floor = np.log(o["energy_floor"])
    raw = np.concatenate([ref_mfcc.mfcc(x, dict(o, energy_floor=0.0))[:, 0] for x in mfcc_cases.edge_batch("full512", o)])
    assert np.abs(raw - floor).min() > 1e-3
    assert (raw > floor).sum() >= 10 and (raw < floor).sum() >= 10
    assert ((raw < floor) & (raw > np.log(EPS) + 1.0)).sum() >= 3       # floored frames that are not digital silence
    got = np.concatenate([ref_mfcc.mfcc(x, o)[:, 0] for x in mfcc_cases.edge_batch("full512", o)])
    assert np.array_equal(got, np.maximum(raw, floor))


def test_tile_map_covers_every_frame_exactly_once():
    """Pure-Python model of the tile map of csrc/mfcc.hip: base(b) = off[b] // 16 + b, tile w belongs to utterance b iff
    base(b) <= w < base(b + 1).  Every frame lies in exactly one (tile, slot), a busy tile's frames are one utterance's, and at
    most B tiles are idle -- what the many-tile GPU test relies on when it sizes its batch by off[B] // 16 + B."""
    rng = np.random.RandomState(5)
    for trial in range(60):
        B = int(rng.randint(1, 70))
        counts = rng.randint(0, 70, size=B)
        counts[rng.rand(B) < 0.3] = 0
        if trial % 4 == 0:
            counts[:int(rng.randint(0, B + 1))] = 0                    # a run of empty utterances at the start
        if trial % 5 == 0:
            counts[B // 2:B // 2 + 9] = 0                              # ... in the middle
        if trial % 7 == 0:
            counts[rng.rand(B) < 0.5] = 16 * rng.randint(1, 4)        # exact multiples of the run
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        tiles = int(off[-1]) // 16 + B
        assert mfcc_cases.tile_base(off, 0) == 0 and mfcc_cases.tile_base(off, B) == tiles
        busy, idle = mfcc_cases.tile_cover(off)
        assert len(busy) + idle == tiles and idle <= B
        hits = np.zeros(int(off[-1]), dtype=np.int64)
        for w, b, t0, nf in busy:
            assert 0 <= w < tiles and 1 <= nf <= 16 and t0 % 16 == 0 and t0 + nf <= counts[b]
            hits[off[b] + t0:off[b] + t0 + nf] += 1
        assert (hits == 1).all()
        assert sorted(w for w, _, _, _ in busy) == sorted(set(w for w, _, _, _ in busy))
        # the binary search of the kernel: the last b with base(b) <= w
        bases = [mfcc_cases.tile_base(off, b) for b in range(B)]
        for w, b, _, _ in busy:
            lo, hi = 0, B - 1
            while lo < hi:
                mid = (lo + hi + 1) >> 1
                if bases[mid] <= w:
                    lo = mid
                else:
                    hi = mid - 1
            assert lo == b


def test_grid_lengths_hit_the_tile_edges():
    for o in (ref_mfcc.VOXCELEB, ref_mfcc.DEFAULTS):
        lengths = mfcc_cases.grid_lengths(o)
        counts = [ref_mfcc.num_frames(n, o) for n in lengths]
        assert lengths[:9] == [0, 1, 79, 80, 81, 399, 400, 401, 560] and counts[9:] == [15, 16, 17, 32, 33]
        # the first frame appears at 400 samples with snip_edges and at 80 (half a shift) without
        assert counts[:9] == ([0, 0, 0, 0, 0, 0, 1, 1, 2] if o["snip_edges"] else [0, 0, 0, 1, 1, 2, 3, 3, 4])
