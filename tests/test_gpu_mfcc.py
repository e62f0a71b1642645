"""GPU: MFCC features and the energy VAD (csrc/mfcc.hip) against the float64 oracle tests/helpers/ref_mfcc.py, for the Kaldi
defaults and the voxceleb and sre recipe configurations, and the wav -> feats / vad -> x-vector command lines.

Feature tolerance: no feature tolerance is given anywhere, so it is measured.  e32 is the largest absolute difference between a
float32 restatement of the pipeline (float32 tables, scipy.fft.rfft on float32) and the float64 oracle on the same batch; the GPU
must be within 4 x e32 of the float64 oracle (the factor covers another butterfly order and the hardware log)."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mfcc_cases  # noqa: E402
import ref_mfcc  # noqa: E402

from oracle import ref_frontend, ref_numpy  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
_ref = {}


def reference(name):
    """Oracle results of the eight-utterance batch, computed once per configuration."""
    if name not in _ref:
        o = mfcc_cases.CONFIGS[name]
        utts = mfcc_cases.batch(o["sample_frequency"])
        f64 = [ref_mfcc.mfcc(x, o) for x in utts]
        f32 = [ref_mfcc.mfcc(x, o, dtype=np.float32) for x in utts]
        e32 = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(f32, f64) if b.shape[0])
        _ref[name] = (utts, f64, float(e32))
    return _ref[name]


def _pack(utts):
    import torch
    off = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)
    return torch.from_numpy(np.concatenate(utts)).cuda(), off


@pytest.mark.parametrize("extra_ld", [0, 5])
@pytest.mark.parametrize("name", sorted(mfcc_cases.CONFIGS))
def test_mfcc_matches_the_oracle(name, extra_ld):
    import torch
    from tf_kaldi_speaker_amd import mfcc as M
    o = mfcc_cases.CONFIGS[name]
    utts, f64, e32 = reference(name)
    opts = M.MfccOptions(**o)
    wave_dev, soff = _pack(utts)
    ld = o["num_ceps"] + extra_ld
    feats, foff = M.mfcc_packed(wave_dev, soff, opts, ld=ld)
    counts = [ref_mfcc.num_frames(len(u), o) for u in utts]
    assert foff.dtype == np.int32 and foff.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    if o["snip_edges"]:
        assert counts[:2] == [0, 0]
    else:
        assert counts[0] == 1
    assert feats.shape == (sum(counts), ld) and feats.dtype == torch.float32
    got = feats.cpu().numpy()
    assert np.isfinite(got).all()
    if extra_ld:
        assert (got[:, o["num_ceps"]:] == 0).all()                     # the columns beyond num_ceps are not written
    want = np.concatenate(f64)
    err = float(np.abs(got[:, :o["num_ceps"]] - want).max())
    print("[mfcc] %s ld=%d: e32 %.3e, GPU max abs error %.3e (bound %.3e)" % (name, ld, e32, err, 4 * e32))
    assert err <= 4 * e32
    # digital silence: the second half of the last utterance
    sil = mfcc_cases.silence_frames(len(utts[-1]), len(utts[-1]) // 2, o)
    assert len(sil) >= 10
    row = np.zeros(o["num_ceps"])
    row[0] = np.log(EPS)
    assert np.abs(got[foff[-2] + sil, :o["num_ceps"]] - row).max() <= 1e-5
    # a second run gives the same bits
    again, _ = M.mfcc_packed(wave_dev, soff, opts, ld=ld)
    assert torch.equal(feats, again)


@pytest.mark.parametrize("name", sorted(mfcc_cases.VAD_CONFIGS))
def test_vad_equals_the_oracle_on_every_frame(name):
    import torch
    from tf_kaldi_speaker_amd import mfcc as M
    o, vo = mfcc_cases.CONFIGS[name], mfcc_cases.VAD_CONFIGS[name]
    utts = [mfcc_cases.loud_quiet(16000.0, sec, 30 + i) for i, sec in enumerate((1.0, 2.3, 3.1, 0.6))]
    feats64 = [ref_mfcc.mfcc(x, o) for x in utts]
    for f in feats64:                                                    # from the oracle alone: no frame near the threshold
        assert np.abs(f[:, 0] - ref_mfcc.vad_threshold(f, vo)).min() > 1e-3
    want = np.concatenate([ref_mfcc.vad(f, vo) for f in feats64])
    assert 0.2 < want.mean() < 0.8
    wave_dev, soff = _pack(utts)
    feats, foff = M.mfcc_packed(wave_dev, soff, M.MfccOptions(**o), ld=o["num_ceps"] + 2)
    vad = M.vad_packed(feats, foff, M.VadOptions(**vo))
    assert vad.dtype == torch.float32 and vad.shape == (foff[-1],)
    assert (vad.cpu().numpy() == want).all()
    assert torch.equal(vad, M.vad_packed(feats, foff, M.VadOptions(**vo)))


def _run(cmd, env, cwd):
    r = subprocess.run(cmd, env=env, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_command_lines_wav_to_xvector(tmp_path, repo_root):
    from tf_kaldi_speaker_amd import kaldi_io, model_io, synth
    o, vo = mfcc_cases.CONFIGS["voxceleb"], mfcc_cases.VAD_CONFIGS["voxceleb"]
    utts = [mfcc_cases.loud_quiet(16000.0, sec, 40 + i) for i, sec in enumerate((1.7, 2.6, 3.4, 2.1))] + [np.zeros(40, np.int16)]
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
    (tmp_path / "mfcc.conf").write_text(mfcc_cases.config_text(o))
    (tmp_path / "vad.conf").write_text(mfcc_cases.config_text(vo))
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cwd = str(tmp_path)
    r = _run([os.path.join(repo_root, "bin", "make_mfcc.sh"), "--mfcc-config", "mfcc.conf", "--vad-config", "vad.conf", "data"], env, cwd)
    assert keys[4] in r.stderr and "no frames" in r.stderr           # the 40-sample utterance is warned about and skipped
    feats = list(kaldi_io.read_mat_scp(str(data / "feats.scp")))
    vads = {k: kaldi_io.read_vec_flt(rx) for k, rx in (line.split(" ", 1) for line in open(str(data / "vad.scp")).read().splitlines())}
    assert [k for k, _ in feats] == keys[:4] and sorted(vads) == sorted(keys[:4])
    assert open(str(data / "utt2num_frames")).read().split() == [s for k, f in feats for s in (k, str(f.shape[0]))]
    f64 = [ref_mfcc.mfcc(x, o) for x in utts[:4]]
    e32 = max(np.abs(ref_mfcc.mfcc(x, o, dtype=np.float32).astype(np.float64) - f).max() for x, f in zip(utts, f64))
    ref_feats = []
    for (k, got), want in zip(feats, f64):
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.abs(got - want).max() <= 4 * e32
        assert np.abs(want[:, 0] - ref_mfcc.vad_threshold(want, vo)).min() > 1e-3
        v = ref_mfcc.vad(want, vo)
        assert (vads[k] == v).all()
        ref_feats.append(ref_frontend.select_voiced(ref_frontend.sliding_cmn(want.astype(np.float32), 300), v))
    # the feature files through the existing front-end route, and the same wavs through --wav-input
    params = dict(synth.TDNN_STAT_PARAMS, num_nodes_pooling_layer=160, num_nodes_last_layer=48)
    weights = synth.synth_weights(params, 30, seed=3, channels=64)
    model_io.save_model(str(tmp_path / "exp"), params, 30, weights, step=1)
    base = [sys.executable, "-m", "tf_kaldi_speaker_amd.extract", "--gpu", "0", "--node", "tdnn6_dense", "--precision", "f32",
            "--cmn-window", "300"]
    _run(base + ["--scp-input", "--vad-rspecifier", "scp:data/vad.scp", "exp", "scp:data/feats.scp", "ark:files.ark"], env, cwd)
    _run(base + ["--wav-input", "--mfcc-config", "mfcc.conf", "--vad-config", "vad.conf", "exp", "scp:data/wav.scp", "ark:wav.ark"], env, cwd)
    a = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "files.ark")))
    b = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "wav.ark")))
    assert [k for k, _ in a] == keys[:4] == [k for k, _ in b]
    for (k, x), (_, y), f in zip(a, b, ref_feats):
        assert np.linalg.norm(x - y) <= 1e-6 * np.linalg.norm(x), k
        want = ref_numpy.predict(f, weights, params, 30)
        assert np.linalg.norm(x - want) / np.linalg.norm(want) <= 1e-4, k
        assert np.linalg.norm(y - want) / np.linalg.norm(want) <= 1e-4, k
