"""xv_reverb (csrc/reverb.hip) and tf_kaldi_speaker_amd.augment on the GPU against the float64 oracle
tests/helpers/ref_reverb.py.  The utterances (tests/helpers/reverb_cases.py) are sized from the kernel's tile T and chunk C.

Bound on the float32 output, quoted from the header of csrc/reverb.hip, u = 2^-24:
    A[n]   = sum_k |h_k||x_{n-k}| + sum_j |g_j v_j| at that sample
    eps[n] = (L + J + 12) u A[n] + eta_E sum_j |g_j v_j[n]|,   eta_E = (e - s) u ||A_e||_2 / ||e||_2
    delta  = ||eps||_2 / ||y||_2 + 8u
    |out - ref| <= scale eps[n] + |ref| delta
(L + J + 12) u A bounds the float32 sum in any order plus the gains' own roundings; eta_E is the relative error sqrt(E)
inherits from an early convolution computed in float32 (A_e, e: the sums of absolute terms and the values of the early
convolution); it multiplies the additive part only and vanishes for J = 0.
int16: |out_i16 - clamp(ref)| < 1 + bound; the clipped count equals the oracle's over the samples farther than the bound
from a saturation threshold, of which at most 1 % may be set aside (tests/test_augment_host.py checks that cap on the
CPU, from the oracle alone)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import reverb_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 512                         # canary samples / bytes on either side of every output and of the workspace


def _tc():
    from tf_kaldi_speaker_amd import augment
    return augment.tile()


def _cases():
    return K.all_cases(*_tc())


def _pack(cases):
    """Packed int16 arrays and the utterance tables of reverberate_packed; equal arrays are stored once."""
    waves, pools, utts, woff = [], {"rir": ([], {}, [0]), "noise": ([], {}, [0])}, [], 0

    def leaf(pool, a):
        parts, index, total = pools[pool]
        key = (a.shape[0], a.tobytes())
        if key not in index:
            index[key] = total[0]
            parts.append(a)
            total[0] += a.shape[0]
        return index[key], a.shape[0]

    for c in cases:
        u = dict(c["opts"], wave=(woff, c["x"].shape[0]), sample_rate=c["fs"])
        waves.append(c["x"])
        woff += c["x"].shape[0]
        if c["h"] is not None:
            u["rir"] = leaf("rir", c["h"])
        u["noises"] = []
        for v, snr, start, ext in c["noises"]:
            off, m = leaf("noise", v)
            u["noises"].append((off, m, m if ext is None else ext, snr, start))
        utts.append(u)
    cat = lambda parts: np.concatenate(parts) if parts else None      # noqa: E731
    return np.concatenate(waves), cat(pools["rir"][0]), cat(pools["noise"][0]), utts


def run(cases, extra_ws=0):
    """One xv_reverb call on `cases` with canaries around both outputs and the workspace (asserted untouched).
    -> list of (out_f32, out_i16, status, peak, clipped) per utterance, numpy."""
    import torch
    from tf_kaldi_speaker_amd import augment
    waves, rirs, noises, utts = _pack(cases)
    dev = "cuda:0"
    up = lambda a: torch.from_numpy(a).to(dev) if a is not None else None      # noqa: E731
    need = augment.workspace_bytes(utts, waves.shape[0], 0 if rirs is None else rirs.shape[0], 0 if noises is None else noises.shape[0])
    total = sum(K.ref(c).n_out for c in cases)
    ws = torch.full((need + extra_ws + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    o16 = torch.full((total + 2 * GUARD,), 0x5A5A, dtype=torch.int16, device=dev)
    o32 = torch.full((total + 2 * GUARD,), -7.25, dtype=torch.float32, device=dev)
    r = augment.reverberate_packed(up(waves), utts, up(rirs), up(noises), workspace=ws[GUARD:GUARD + need + extra_ws],
                                   out_i16=o16[GUARD:GUARD + total], out_f32=o32[GUARD:GUARD + total], check=False)
    torch.cuda.synchronize()
    ws, o16, o32 = ws.cpu().numpy(), o16.cpu().numpy(), o32.cpu().numpy()
    assert (ws[:GUARD] == 0xA5).all() and (ws[GUARD + need + extra_ws:] == 0xA5).all(), "workspace canary"
    assert (o16[:GUARD] == 0x5A5A).all() and (o16[GUARD + total:] == 0x5A5A).all(), "int16 canary"
    assert (o32[:GUARD] == -7.25).all() and (o32[GUARD + total:] == -7.25).all(), "float32 canary"
    assert r.offsets[-1] == total
    out = []
    for i in range(len(cases)):
        a, b = GUARD + int(r.offsets[i]), GUARD + int(r.offsets[i + 1])
        out.append((o32[a:b].copy(), o16[a:b].copy(), int(r.status[i]), int(r.peak[i]), int(r.clipped[i])))
    return out


def check(c, got):
    """One utterance against the oracle: status, peak, the float32 bound, the int16 bound, the clipped count."""
    o32, o16, status, peak, clipped = got
    r = K.ref(c)
    name = c["name"]
    assert status == 0 and peak == r.p, (name, status, peak, r.p)
    assert o32.shape[0] == r.n_out == o16.shape[0], name
    err = np.abs(o32.astype(np.float64) - r.out)
    worst = float((err / np.maximum(r.bound, 1e-300)).max()) if err.size else 0.0
    print("%s: n_out %d, max |err| %.3e, max err / bound %.3f, clipped %d (oracle %d)" % (name, r.n_out, err.max() if err.size else 0.0,
                                                                                         worst, clipped, r.clipped))
    assert np.all(err <= r.bound), (name, worst)
    assert np.all(np.abs(o16.astype(np.float64) - np.clip(r.out, -32768.0, 32767.0)) < 1.0 + r.bound), name
    close = K.close_mask(r)
    sure = int((r.clip_mask & ~close).sum())
    assert sure <= clipped <= sure + int(close.sum()), (name, clipped, sure, int(close.sum()))
    return worst


# ------------------------------------------------------------------------------------------------ convolution edges
def test_every_n_by_l_edge():
    T, C = _tc()
    Ns, Ls = K.conv_lengths(T, C)
    cases = [c for n, c in _cases().items() if n.startswith("conv_")]
    assert len(cases) == len(Ns) * len(Ls) + 1
    assert {c["x"].shape[0] for c in cases} >= set(Ns) and {c["h"].shape[0] for c in cases} >= set(Ls)
    assert {c["fs"] for c in cases} == {8000, 16000}
    assert any(c["h"].shape[0] > c["x"].shape[0] for c in cases)
    for c, got in zip(cases, run(cases)):
        check(c, got)


def test_peak_positions_and_the_signed_maximum():
    cs = _cases()
    cases = [c for n, c in cs.items() if n.startswith("peak_")]
    L = cs["peak_first"]["h"].shape[0]
    want = {"peak_first": 0, "peak_last": L - 1, "peak_near_start": 3, "peak_near_end": L - 4, "peak_middle": L // 2,
            "peak_signed": 40, "peak_tie": 0}
    assert int(np.abs(cs["peak_signed"]["h"].astype(np.int32)).argmax()) == 90
    for c, got in zip(cases, run(cases)):
        assert got[3] == want[c["name"]], c["name"]
        check(c, got)


# ------------------------------------------------------------------------------------------------ mixing and emission
def test_mixing_and_emission_cases():
    cs = _cases()
    cases = [c for n, c in cs.items() if n.startswith(("mix_", "emit_", "plain"))]
    got = run(cases)
    by = {c["name"]: g for c, g in zip(cases, got)}
    for c, g in zip(cases, got):
        check(c, g)
    # a start at or past Y adds nothing: the bits of the utterance without additive signals
    for name in ("mix_start_at_Y", "mix_start_past_Y"):
        assert np.array_equal(by[name][0].view(np.int32), by["mix_none"][0].view(np.int32)), name
        assert np.array_equal(by[name][1], by["mix_none"][1]), name
    # no RIR, no normalisation: the input comes back as it went in
    assert np.array_equal(by["plain"][1], cs["plain"]["x"]) and by["plain"][4] == 0
    # the volume case does saturate, in both directions, and the count is the oracle's
    r = K.ref(cs["emit_volume_saturates"])
    assert r.clipped > 20 and (r.out > 40000).any() and (r.out < -40000).any()
    o16 = by["emit_volume_saturates"][1]
    assert o16.max() == 32767 and o16.min() == -32768
    # lengths: duration below / equal / above, the tail without the shift
    x, h = cs["mix_none"]["x"], cs["mix_none"]["h"]
    N, Y = x.shape[0], x.shape[0] + h.shape[0] - 1
    assert [K.ref(cs[n]).n_out for n in ("emit_duration_below_N", "emit_duration_equal_N", "emit_duration_above_Y_shift",
                                         "emit_duration_above_Y_no_shift", "emit_no_shift", "mix_none")] == \
        [N - 700, N, 2 * Y + 77, 2 * Y + 77, Y, N]
    # the wrap: the samples behind Y repeat the ones Y before them, bit for bit
    for name in ("emit_duration_above_Y_shift", "emit_duration_above_Y_no_shift"):
        o = by[name][0].view(np.int32)
        assert np.array_equal(o[Y:2 * Y], o[:Y]) and np.array_equal(o[2 * Y:], o[:77]), name


def test_status_of_a_silent_additive_signal_and_of_a_silent_output():
    from tf_kaldi_speaker_amd import augment
    T, C = _tc()
    good = K.case(K.sig(300, 1), 8000, K.rir(20, 2))
    silent_noise = K.case(K.sig(300, 3), 8000, None, [(np.zeros(64, dtype=np.int16), 10.0, 0.0, None)])
    silent = K.case(np.zeros(T + 3, dtype=np.int16), 8000, K.rir(20, 4))
    for i, c in enumerate((good, silent_noise, silent)):
        c["name"] = "status_%d" % i
    # the references of the failing ones are errors in the oracle too
    for c in (silent_noise, silent):
        with pytest.raises(ValueError):
            K.ref(c)
        c["ref"] = type("N", (), {"n_out": c["x"].shape[0]})()
    got = run([good, silent_noise, silent])
    check(good, got[0])
    assert [g[2] for g in got] == [0, 1, 2]
    for g in got[1:]:
        assert not g[0].any() and not g[1].any() and g[4] == 0            # zeros, never inf
    waves, rirs, noises, utts = _pack([good, silent_noise])
    import torch
    with pytest.raises(ValueError, match="utterance 1: an additive signal has zero power"):
        augment.reverberate_packed(torch.from_numpy(waves).cuda(), utts, torch.from_numpy(rirs).cuda(), torch.from_numpy(noises).cuda())


# ------------------------------------------------------------------------------------------------ purity and bounds
def _bits(g):
    return g[0].view(np.int32).tobytes() + g[1].tobytes() + repr(g[2:5]).encode()


def test_an_utterance_gives_the_same_bits_alone_in_a_batch_on_a_repeat_and_with_a_larger_workspace():
    cs = _cases()
    T, C = _tc()
    probe = cs["mix_two_overlapping"]
    find = lambda prefix: next(c for n, c in cs.items() if n.startswith(prefix))      # noqa: E731
    others = [find("conv_N%d_L%d_" % (3 * T + 5, 2 * C + 3)), cs["mix_no_rir"], cs["mix_none"], cs["emit_volume_saturates"],
              cs["peak_signed"], find("conv_N1_L1_")]
    assert any(c["h"] is None for c in others) and any(not c["noises"] for c in others)
    alone = run([probe])[0]
    check(probe, alone)
    first = run([probe] + others + [probe])
    assert len(first) == 8
    assert _bits(first[0]) == _bits(alone) and _bits(first[-1]) == _bits(alone)
    again = run([probe] + others + [probe])
    assert [_bits(g) for g in again] == [_bits(g) for g in first]
    wide = run([probe] + others + [probe], extra_ws=123 * 256)
    assert [_bits(g) for g in wide] == [_bits(g) for g in first]
    for c, g in zip(others, first[1:-1]):
        check(c, g)


# ------------------------------------------------------------------------------------------------ the Python layer
def _write_files(tmp_path):
    from tf_kaldi_speaker_amd import augment
    fs = 8000
    T, C = _tc()
    files = {"a": K.sig(T + 100, 501), "b": K.sig(900, 502), "c": K.sig(2 * T + 7, 503), "rir": K.rir(C + 9, 504),
             "music": K.sig(1300, 505, 900.0), "noise": K.sig(400, 506, 1200.0)}
    paths = {}
    for name, x in files.items():
        paths[name] = str(tmp_path / (name + ".wav"))
        augment.write_wav(paths[name], fs, x)
    lines = [
        ("plain", paths["a"]),
        ("reverb", 'wav-reverberate --shift-output=true --impulse-response="%s" %s - |' % (paths["rir"], paths["b"])),
        ("noise", "wav-reverberate --shift-output=true --additive-signals='wav-reverberate --duration=%.7f \"%s\" - |,%s' "
                  "--start-times='0,0.05' --snrs='8,12' %s - |" % ((2 * T + 7 + 0.5) / fs, paths["music"], paths["noise"], paths["c"])),
    ]
    return fs, files, paths, lines


def test_resolve_batch_on_wav_files_equals_reverberate_packed_on_the_arrays(tmp_path):
    import torch
    from tf_kaldi_speaker_amd import augment
    fs, files, paths, lines = _write_files(tmp_path)
    out, off = augment.resolve_batch([spec for _, spec in lines], fs)
    T, C = _tc()
    cases = [K.case(files["a"], fs, None, normalize_output=False, shift_output=False),
             K.case(files["b"], fs, files["rir"]),
             K.case(files["c"], fs, None, [(files["music"], 8.0, 0.0, 2 * T + 7), (files["noise"], 12.0, 0.05, None)])]
    waves, rirs, noises, utts = _pack(cases)
    r = augment.reverberate_packed(torch.from_numpy(waves).cuda(), utts, torch.from_numpy(rirs).cuda(), torch.from_numpy(noises).cuda())
    assert np.array_equal(off, r.offsets) and out.dtype == torch.int16 and out.is_cuda
    assert torch.equal(out, r.out_i16)
    assert np.array_equal(out[:off[1]].cpu().numpy(), files["a"])
    for i, c in enumerate(cases):
        c["name"] = "file_%d" % i
        ref = K.ref(c)
        assert np.all(np.abs(out[off[i]:off[i + 1]].cpu().numpy() - np.clip(ref.out, -32768, 32767)) < 1.0 + ref.bound)
    with pytest.raises(ValueError, match="sample rate"):
        augment.resolve_batch([lines[1][1]], 16000)


def test_compute_mfcc_native_reverberate_equals_mfcc_of_the_resolved_batch(tmp_path):
    from tf_kaldi_speaker_amd import augment, compute_mfcc, kaldi_io
    from tf_kaldi_speaker_amd.mfcc import MfccOptions, mfcc_packed
    fs, files, paths, lines = _write_files(tmp_path)
    scp = str(tmp_path / "wav.scp")
    with open(scp, "w") as f:
        for key, spec in lines:
            f.write("%s %s\n" % (key, spec))
    ark = str(tmp_path / "feats.ark")
    rc = compute_mfcc.main(["--native-reverberate", "--sample-frequency=%d" % fs, "scp:" + scp, "ark:" + ark])
    assert rc == 0
    got = dict(kaldi_io.read_mat_ark(ark))
    out, off = augment.resolve_batch([spec for _, spec in lines], fs)
    feats, foff = mfcc_packed(out, off, MfccOptions(sample_frequency=fs))
    feats = feats.cpu().numpy()
    assert list(got) == [k for k, _ in lines]
    for i, (key, _) in enumerate(lines):
        assert foff[i + 1] > foff[i]
        assert np.array_equal(got[key].view(np.int32), feats[foff[i]:foff[i + 1]].view(np.int32)), key


def test_extract_wav_input_native_reverberate_equals_extract_on_the_written_files(tmp_path):
    """extract --wav-input --native-reverberate on the pipelines gives the x-vectors, bit for bit, of extract --wav-input on
    the wav files augment_wav writes from the same pipelines (both in this process: the flag is the same hook as compute_mfcc's)."""
    import mfcc_cases
    from tf_kaldi_speaker_amd import augment, augment_wav, extract, kaldi_io, model_io, synth
    fs = 16000
    o, vo = mfcc_cases.CONFIGS["voxceleb"], mfcc_cases.VAD_CONFIGS["voxceleb"]
    paths = {}
    for name, x in (("a", mfcc_cases.loud_quiet(16000.0, 1.3, 71)), ("b", mfcc_cases.loud_quiet(16000.0, 1.1, 72)),
                    ("rir", K.rir(700, 73)), ("noise", K.sig(5000, 74, 60.0))):
        paths[name] = str(tmp_path / (name + ".wav"))
        augment.write_wav(paths[name], fs, x)
    scp = str(tmp_path / "wav.scp")
    with open(scp, "w") as f:
        f.write("s1-plain %s\n" % paths["a"])
        f.write('s1-rev wav-reverberate --shift-output=true --impulse-response="%s" %s - |\n' % (paths["rir"], paths["b"]))
        f.write("s2-noise wav-reverberate --shift-output=true --additive-signals='wav-reverberate --duration=1.3 \"%s\" - |' "
                "--start-times='0' --snrs='15' %s - |\n" % (paths["noise"], paths["a"]))
    (tmp_path / "mfcc.conf").write_text(mfcc_cases.config_text(o))
    (tmp_path / "vad.conf").write_text(mfcc_cases.config_text(vo))
    params = dict(synth.TDNN_STAT_PARAMS, num_nodes_pooling_layer=160, num_nodes_last_layer=48)
    model_io.save_model(str(tmp_path / "exp"), params, 30, synth.synth_weights(params, 30, seed=3, channels=64), step=1)
    assert augment_wav.main(["--sample-frequency", "16000", "scp:" + scp, str(tmp_path / "wav")]) == 0
    base = ["--gpu", "0", "--node", "tdnn6_dense", "--precision", "f32", "--cmn-window", "300", "--wav-input",
            "--mfcc-config", str(tmp_path / "mfcc.conf"), "--vad-config", str(tmp_path / "vad.conf")]
    extract.main(base + ["--native-reverberate", str(tmp_path / "exp"), "scp:" + scp, "ark:" + str(tmp_path / "native.ark")])
    extract.main(base + [str(tmp_path / "exp"), "scp:" + str(tmp_path / "wav" / "wav.scp"), "ark:" + str(tmp_path / "files.ark")])
    a = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "native.ark")))
    b = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "files.ark")))
    assert [k for k, _ in a] == ["s1-plain", "s1-rev", "s2-noise"] == [k for k, _ in b]
    for (k, x), (_, y) in zip(a, b):
        assert np.isfinite(x).all() and np.array_equal(x.view(np.int32), y.view(np.int32)), k
    assert not np.array_equal(a[0][1], a[2][1])                 # the additive signal did change the utterance
