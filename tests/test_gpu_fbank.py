"""GPU: fbank features and their side energy (fbank_kernel of csrc/mfcc.hip) against the float64 oracle
tests/helpers/ref_fbank.py, for the ResNet recipe's fbank.conf, the Kaldi defaults, an 8 kHz set with the energy column, the
energy floor and the amplitude spectrum, and the linear (no log) output; the energy VAD decided on the side energy; and the
wav -> feats / vad -> ResNet x-vector command lines.

Feature tolerance, measured as in tests/test_gpu_mfcc.py: e32 is the largest absolute difference between the oracle's float32
mode (float32 tables, scipy.fft.rfft on float32) and its float64 mode on the same batch; the GPU must be within 4 x e32 of the
float64 oracle.  The linear output spans twelve decades, so there both sides are compared after log(max(., FLT_EPSILON))."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mfcc_cases  # noqa: E402
import ref_fbank  # noqa: E402
import ref_mfcc  # noqa: E402

from oracle import ref_frontend, ref_numpy  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
V3_CONF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fbank_v3.conf")
_ref = {}


def _options(name):
    from tf_kaldi_speaker_amd import fbank as F
    if name == "v3":                                              # the fixture itself
        return F.FbankOptions.from_config(V3_CONF)
    if name == "linear":                                          # v3 with --use-log-fbank=false
        return F.FbankOptions(**dict(F.FbankOptions.from_config(V3_CONF).as_dict(), use_log_fbank=False))
    return F.FbankOptions(**ref_fbank.CONFIGS[name])


def _comparable(name, feats):
    """What the tolerance is measured on: the features, or their floored log for the linear output."""
    if ref_fbank.CONFIGS[name]["use_log_fbank"]:
        return np.asarray(feats, dtype=np.float64)
    return np.log(np.maximum(np.asarray(feats, dtype=np.float64), EPS))


def reference(name):
    """Oracle results of the eight-utterance batch, computed once per option set: (utterances, float64 features, float64
    energies, e32)."""
    if name not in _ref:
        o = ref_fbank.CONFIGS[name]
        utts = mfcc_cases.batch(o["sample_frequency"])
        f64 = [ref_fbank.fbank(x, o) for x in utts]
        f32 = [ref_fbank.fbank(x, o, dtype=np.float32) for x in utts]
        e32 = max(max(np.abs(_comparable(name, a[0]) - _comparable(name, b[0])).max(), np.abs(a[1].astype(np.float64) - b[1]).max())
                  for a, b in zip(f32, f64) if b[0].shape[0])
        _ref[name] = (utts, [f for f, _ in f64], [e for _, e in f64], float(e32))
    return _ref[name]


def _pack(utts):
    import torch
    off = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)
    return torch.from_numpy(np.concatenate(utts)).cuda(), off


def _mfcc_twin(o):
    """MFCC options with the frame, --raw-energy and --energy-floor options of the fbank set `o` and the energy in coefficient 0."""
    from tf_kaldi_speaker_amd import mfcc as M
    keep = ("sample_frequency", "frame_length", "frame_shift", "preemphasis_coefficient", "remove_dc_offset", "window_type",
            "snip_edges", "raw_energy", "energy_floor")
    return M.MfccOptions(use_energy=True, **{k: o[k] for k in keep})


@pytest.mark.parametrize("extra_ld", [0, 5])
@pytest.mark.parametrize("name", sorted(ref_fbank.CONFIGS))
def test_fbank_matches_the_oracle(name, extra_ld):
    import torch
    from tf_kaldi_speaker_amd import fbank as F
    o = ref_fbank.CONFIGS[name]
    utts, f64, en64, e32 = reference(name)
    opts = _options(name)
    assert {k: v for k, v in opts.as_dict().items() if k in o} == o
    nf = ref_fbank.num_feats(o)
    assert opts.num_feats == nf
    wave_dev, soff = _pack(utts)
    ld = nf + extra_ld
    feats, foff, energy = F.fbank_packed(wave_dev, soff, opts, ld=ld, energy=True)
    counts = [ref_mfcc.num_frames(len(u), o) for u in utts]
    assert foff.dtype == np.int32 and foff.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert counts[0] == (0 if o["snip_edges"] else 1)                 # 100 samples: no frame, or one made of reflections
    assert feats.shape == (sum(counts), ld) and feats.dtype == torch.float32
    assert energy.shape == (sum(counts),) and energy.dtype == torch.float32
    got, got_e = feats.cpu().numpy(), energy.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(got_e).all()
    if extra_ld:
        assert (got[:, nf:] == 0).all()                                # the columns beyond num_feats are not written
    err = float(np.abs(_comparable(name, got[:, :nf]) - _comparable(name, np.concatenate(f64))).max())
    err_e = float(np.abs(got_e - np.concatenate(en64)).max())
    print("[fbank] %s ld=%d: e32 %.3e, GPU max abs error %.3e, side energy %.3e (bound %.3e)" % (name, ld, e32, err, err_e, 4 * e32))
    assert err <= 4 * e32
    assert err_e <= 4 * e32
    # digital silence: the second half of the last utterance
    sil = mfcc_cases.silence_frames(len(utts[-1]), len(utts[-1]) // 2, o)
    assert len(sil) >= 10
    row = np.full(nf, np.log(EPS))
    floor = max(np.log(EPS), np.log(o["energy_floor"])) if o["energy_floor"] > 0 else np.log(EPS)
    if o["use_energy"]:
        row[0] = floor
    assert np.abs(_comparable(name, got[foff[-2] + sil, :nf]) - row).max() <= 1e-5
    assert np.abs(got_e[foff[-2] + sil] - floor).max() <= 1e-5
    # without the side output the features are the same bits, and so is a second run
    plain, foff2 = F.fbank_packed(wave_dev, soff, opts, ld=ld)
    assert torch.equal(plain, feats) and (foff2 == foff).all()
    again, _, energy_again = F.fbank_packed(wave_dev, soff, opts, ld=ld, energy=True)
    assert torch.equal(feats, again) and torch.equal(energy, energy_again)


@pytest.mark.parametrize("name", ["v3", "energy8k"])
def test_side_energy_is_the_mfcc_energy_bit_for_bit(name):
    import torch
    from tf_kaldi_speaker_amd import fbank as F, mfcc as M
    o = ref_fbank.CONFIGS[name]
    utts = reference(name)[0]
    wave_dev, soff = _pack(utts)
    feats, foff, energy = F.fbank_packed(wave_dev, soff, _options(name), energy=True)
    cep, moff = M.mfcc_packed(wave_dev, soff, _mfcc_twin(o))
    assert (foff == moff).all() and foff[-1] > 100
    assert torch.equal(energy, cep[:, 0].contiguous())
    if o["use_energy"]:
        assert torch.equal(feats[:, 0].contiguous(), energy)
    # ... and it does not depend on --use-energy
    flipped = F.FbankOptions(**dict(o, use_energy=not o["use_energy"]))
    feats2, _, energy2 = F.fbank_packed(wave_dev, soff, flipped, energy=True)
    assert torch.equal(energy2, energy)
    a, b = (feats[:, 1:], feats2) if o["use_energy"] else (feats, feats2[:, 1:])
    assert torch.equal(a.contiguous(), b.contiguous())


@pytest.mark.parametrize("name", sorted(mfcc_cases.VAD_CONFIGS))
def test_vad_from_the_side_energy_equals_the_oracle_on_every_frame(name):
    import torch
    from tf_kaldi_speaker_amd import fbank as F, mfcc as M
    fname = {"kaldi_defaults": "kaldi_defaults", "voxceleb": "v3"}[name]
    o, vo = ref_fbank.CONFIGS[fname], mfcc_cases.VAD_CONFIGS[name]
    utts = [mfcc_cases.loud_quiet(16000.0, sec, 30 + i) for i, sec in enumerate((1.0, 2.3, 3.1, 0.6))]
    en64 = [ref_fbank.fbank(x, o)[1][:, None] for x in utts]
    for e in en64:                                                       # from the oracle alone: no frame near the threshold
        assert np.abs(e[:, 0] - ref_mfcc.vad_threshold(e, vo)).min() > 1e-3
    want = np.concatenate([ref_mfcc.vad(e, vo) for e in en64])
    assert 0.2 < want.mean() < 0.8
    wave_dev, soff = _pack(utts)
    _, foff, energy = F.fbank_packed(wave_dev, soff, _options(fname), energy=True)
    vad = M.vad_packed(energy.view(-1, 1), foff, M.VadOptions(**vo))
    assert vad.dtype == torch.float32 and vad.shape == (foff[-1],)
    assert (vad.cpu().numpy() == want).all()


def _run(cmd, env, cwd, ok=True):
    r = subprocess.run(cmd, env=env, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


def test_command_lines_wav_to_resnet_xvector(tmp_path, repo_root):
    from tf_kaldi_speaker_amd import kaldi_io, model_io, synth
    o, vo = ref_fbank.V3, mfcc_cases.VAD_CONFIGS["voxceleb"]
    utts = [mfcc_cases.loud_quiet(16000.0, sec, 40 + i) for i, sec in enumerate((1.7, 1.2, 2.2, 0.9))] + [np.zeros(40, np.int16)]
    keys = ["spk%d-utt%d" % (i // 2, i) for i in range(len(utts))]
    data = tmp_path / "data"
    data.mkdir()
    with open(str(data / "wav.scp"), "w") as scp:
        for i, (k, x) in enumerate(zip(keys, utts)):
            path = str(tmp_path / (k + ".wav"))
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(x.astype("<i2").tobytes())
            scp.write("%s %s\n" % (k, path if i % 2 else "cat %s |" % path))
    (tmp_path / "fbank_v3.conf").write_bytes(open(V3_CONF, "rb").read())
    (tmp_path / "vad.conf").write_text(mfcc_cases.config_text(vo))
    # an MFCC configuration with the frame options of fbank_v3.conf: its C0 is the energy the fbank pass hands out
    (tmp_path / "mfcc.conf").write_text(mfcc_cases.config_text(dict(ref_mfcc.VOXCELEB, window_type="hamming")))
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cwd = str(tmp_path)
    r = _run([os.path.join(repo_root, "bin", "make_fbank.sh"), "--fbank-config", "fbank_v3.conf", "--vad-config", "vad.conf", "data"], env, cwd)
    assert keys[4] in r.stderr and "no frames" in r.stderr           # the 40-sample utterance is warned about and skipped
    assert os.path.isfile(str(data / "data" / "raw_fbank_data.ark")) and os.path.isfile(str(data / "data" / "vad_data.ark"))
    feats = list(kaldi_io.read_mat_scp(str(data / "feats.scp")))
    vads = {k: kaldi_io.read_vec_flt(rx) for k, rx in (line.split(" ", 1) for line in open(str(data / "vad.scp")).read().splitlines())}
    assert [k for k, _ in feats] == keys[:4] and sorted(vads) == sorted(keys[:4])
    assert open(str(data / "utt2num_frames")).read().split() == [s for k, f in feats for s in (k, str(f.shape[0]))]
    f64 = [ref_fbank.fbank(x, o) for x in utts[:4]]
    e32 = max(np.abs(ref_fbank.fbank(x, o, dtype=np.float32)[0].astype(np.float64) - f).max() for x, (f, _) in zip(utts, f64))
    ref_feats = []
    for (k, got), (want, energy) in zip(feats, f64):
        assert got.dtype == np.float32 and got.shape == want.shape and got.shape[1] == 40
        assert np.abs(got - want).max() <= 4 * e32
        assert np.abs(energy - ref_mfcc.vad_threshold(energy[:, None], vo)).min() > 1e-3
        v = ref_mfcc.vad(energy[:, None], vo)
        assert (vads[k] == v).all()
        ref_feats.append(ref_frontend.select_voiced(ref_frontend.sliding_cmn(want.astype(np.float32), 300), v))
    # a synthetic ResNet-18 through the feature files, through the wavs, and through the wavs with the VAD of an MFCC pass
    params = dict(synth.RESNET_PARAMS)
    weights = synth.synth_resnet_weights(params, seed=3, width=8)
    model_io.save_model(str(tmp_path / "exp"), params, 40, weights, step=1)
    base = [sys.executable, "-m", "tf_kaldi_speaker_amd.extract", "--gpu", "0", "--node", "tdnn6_dense", "--precision", "f32",
            "--cmn-window", "300"]
    wav = ["--wav-input", "--fbank-config", "fbank_v3.conf", "--vad-config", "vad.conf"]
    _run(base + ["--scp-input", "--vad-rspecifier", "scp:data/vad.scp", "exp", "scp:data/feats.scp", "ark:files.ark"], env, cwd)
    _run(base + wav + ["exp", "scp:data/wav.scp", "ark:wav.ark"], env, cwd)
    _run(base + wav + ["--mfcc-config", "mfcc.conf", "exp", "scp:data/wav.scp", "ark:wav_mfcc_vad.ark"], env, cwd)
    a = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "files.ark")))
    b = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "wav.ark")))
    c = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "wav_mfcc_vad.ark")))
    assert [k for k, _ in a] == keys[:4] == [k for k, _ in b] == [k for k, _ in c]
    for (k, x), (_, y), (_, z), f in zip(a, b, c, ref_feats):
        assert np.linalg.norm(x - y) <= 1e-6 * np.linalg.norm(x), k
        assert np.linalg.norm(x - z) <= 1e-6 * np.linalg.norm(x), k
        want = ref_numpy.predict(f, weights, params, 40)
        for got in (x, y, z):
            assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-4, k
    # a 30-dim TDNN cannot take 40 fbank features: refused, naming both widths
    tparams = dict(synth.TDNN_STAT_PARAMS, num_nodes_pooling_layer=160, num_nodes_last_layer=48)
    model_io.save_model(str(tmp_path / "tdnn"), tparams, 30, synth.synth_weights(tparams, 30, seed=3, channels=64), step=1)
    r = _run(base + wav + ["tdnn", "scp:data/wav.scp", "ark:never.ark"], env, cwd, ok=False)
    assert "30" in r.stderr and "40" in r.stderr and "fbank_v3.conf" in r.stderr
    assert not os.path.exists(str(tmp_path / "never.ark"))
    # frame options that do not match: the VAD of the MFCC pass does not fit, both files are named
    (tmp_path / "mfcc_snip.conf").write_text(mfcc_cases.config_text(dict(ref_mfcc.VOXCELEB, snip_edges=True)))
    r = _run(base + wav + ["--mfcc-config", "mfcc_snip.conf", "exp", "scp:data/wav.scp", "ark:mismatch.ark"], env, cwd, ok=False)
    assert "fbank_v3.conf" in r.stderr and "mfcc_snip.conf" in r.stderr
