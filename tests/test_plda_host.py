"""Host side of the PLDA scoring feature (no GPU): the algebra of the oracle against the generative model, the expansion
the GPU evaluates against the plda.cc form, Kaldi Plda file I/O, smoothing, minDCF, the histogram range of the EER and
the argument errors of the command line."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_plda  # noqa: E402


@pytest.mark.parametrize("d", [3, 150, 200, 512])
def test_oracle_forms_agree(d):
    """plda.cc's LogLikelihoodRatio equals the log ratio of the joint 2 x 2 Gaussian over the marginals, 1e-9 relative."""
    rng = np.random.default_rng(100 + d)
    _, _, psi = ref_plda.random_model(rng, d)
    n = rng.integers(1, 31, 40)
    e, t = 1.5 * rng.standard_normal((40, d)), 1.5 * rng.standard_normal((50, d))
    a, b = ref_plda.llr(psi, e, n, t), ref_plda.llr_gaussian(psi, e, n, t)
    scale = np.maximum(np.abs(a), 1.0)
    print("d = %d: scores %.1f..%.1f, max relative difference %.2e" % (d, a.min(), a.max(), np.max(np.abs(a - b) / scale)))
    assert np.max(np.abs(a - b) / scale) <= 1e-9
    ia, ib = rng.integers(0, 40, 300), rng.integers(0, 50, 300)
    assert np.max(np.abs(ref_plda.llr_pairs(psi, e, n, t, ia, ib) - a[ia, ib]) / scale[ia, ib]) <= 1e-12


@pytest.mark.parametrize("d", [3, 200])
def test_expansion_tables_match_the_oracle(d):
    """s = sum A t + sum W t^2 + rho with the float64 tables of plda.tables is the plda.cc form."""
    from tf_kaldi_speaker_amd import plda
    rng = np.random.default_rng(7 + d)
    _, _, psi = ref_plda.random_model(rng, d)
    e, t = rng.standard_normal((9, d)), rng.standard_normal((11, d))
    for n in (1, 5, 30):
        tab = plda.tables(psi, n)
        s = (e * tab["a"]) @ t.T + ((t * t) @ tab["w"])[None, :] + (tab["logdet"] + (e * e) @ tab["q"])[:, None]
        want = ref_plda.llr(psi, e, n, t)
        assert np.max(np.abs(s - want) / np.maximum(np.abs(want), 1.0)) <= 1e-11
        assert np.allclose(tab["inv"], 1.0 / (psi + 1.0 / n), rtol=1e-15)


def _model(d, seed=3):
    from tf_kaldi_speaker_amd import plda
    return plda.Plda(*ref_plda.random_model(np.random.default_rng(seed), d))


@pytest.mark.parametrize("binary", [True, False])
def test_round_trip_is_bit_exact(tmp_path, binary):
    from tf_kaldi_speaker_amd import plda
    m = _model(17)
    path = str(tmp_path / "plda")
    plda.write_plda(path, m, binary=binary)
    r = plda.read_plda(path)
    for a, b in ((m.mean, r.mean), (m.transform, r.transform), (m.psi, r.psi)):
        assert a.dtype == np.float64 and b.dtype == np.float64 and a.shape == b.shape
        assert a.tobytes() == b.tobytes()
    r2 = plda.read_plda("cat %s |" % path)           # a pipe, as "ivector-copy-plda ... - |"
    assert r2.transform.tobytes() == m.transform.tobytes()
    if not binary:
        assert open(path).read().startswith("<Plda>  [ ")


def _hand_bytes(vec_tag=b"DV ", mat_tag=b"DM ", fmt="d"):
    mean, psi = [0.5, -1.0, 2.0], [4.0, 1.0, 0.25]
    transform = [[1.0, 2.0, 3.0], [0.0, 1.0, 4.0], [0.0, 0.0, 1.0]]
    b = b"\0B<Plda> " + vec_tag + b"\x04" + struct.pack("<i", 3) + struct.pack("<3" + fmt, *mean)
    b += mat_tag + b"\x04" + struct.pack("<i", 3) + b"\x04" + struct.pack("<i", 3) + struct.pack("<9" + fmt, *sum(transform, []))
    b += vec_tag + b"\x04" + struct.pack("<i", 3) + struct.pack("<3" + fmt, *psi) + b"</Plda> "
    return b, np.array(mean), np.array(transform), np.array(psi)


def test_hand_assembled_binary_file(tmp_path):
    from tf_kaldi_speaker_amd import plda
    data, mean, transform, psi = _hand_bytes()
    (tmp_path / "hand").write_bytes(data)
    m = plda.read_plda(str(tmp_path / "hand"))
    assert np.array_equal(m.mean, mean) and np.array_equal(m.transform, transform) and np.array_equal(m.psi, psi)
    assert m.dim == 3
    plda.write_plda(str(tmp_path / "again"), m)
    assert (tmp_path / "again").read_bytes() == data
    # float payloads are accepted and widened
    fdata = _hand_bytes(b"FV ", b"FM ", "f")[0]
    (tmp_path / "hand32").write_bytes(fdata)
    m32 = plda.read_plda(str(tmp_path / "hand32"))
    assert m32.transform.dtype == np.float64 and np.array_equal(m32.transform, transform) and np.array_equal(m32.psi, psi)
    # the text form
    (tmp_path / "text").write_text("<Plda>  [ 0.5 -1 2 ]\n [\n  1 2 3\n  0 1 4\n  0 0 1 ]\n [ 4 1 0.25 ]\n</Plda> ")
    mt = plda.read_plda(str(tmp_path / "text"))
    assert np.array_equal(mt.mean, mean) and np.array_equal(mt.transform, transform) and np.array_equal(mt.psi, psi)


def test_malformed_files_raise(tmp_path):
    from tf_kaldi_speaker_amd import kaldi_io, plda
    data = _hand_bytes()[0]

    def read(b):
        (tmp_path / "bad").write_bytes(b)
        return plda.read_plda(str(tmp_path / "bad"))

    with pytest.raises(kaldi_io.BadInputFormat, match="</Plda>"):
        read(data[:-len(b"</Plda> ")])
    with pytest.raises(kaldi_io.BadInputFormat, match="<Plda>"):
        read(data.replace(b"<Plda> ", b"<Lda> "))
    with pytest.raises(kaldi_io.BadInputFormat):
        read(data[:60])                                                                  # cut inside the matrix
    with pytest.raises(kaldi_io.UnknownVectorHeader):
        read(data.replace(b"DV ", b"XV ", 1))
    with pytest.raises(kaldi_io.BadInputFormat, match="2 x 3"):
        plda.Plda(np.zeros(3), np.zeros((2, 3)), np.ones(2))
    with pytest.raises(kaldi_io.BadInputFormat, match="dimension 4"):
        plda.Plda(np.zeros(4), np.eye(3), np.ones(3))
    with pytest.raises(kaldi_io.BadInputFormat, match="dimension 2"):
        plda.Plda(np.zeros(3), np.eye(3), np.ones(2))
    with pytest.raises(kaldi_io.BadInputFormat, match="negative"):
        plda.Plda(np.zeros(3), np.eye(3), np.array([1.0, -0.5, 0.1]))
    with pytest.raises(kaldi_io.BadInputFormat, match="</Plda>"):
        read(b"<Plda>  [ 0.5 -1 2 ]\n [\n  1 2 3\n  0 1 4\n  0 0 1 ]\n [ 4 1 0.25 ]\n")
    with pytest.raises(kaldi_io.BadInputFormat, match="lengths"):
        read(b"<Plda>  [ 0.5 -1 2 ]\n [\n  1 2 3\n  0 1\n  0 0 1 ]\n [ 4 1 0.25 ]\n</Plda> ")


def test_smoothing():
    from tf_kaldi_speaker_amd import plda
    m = _model(12)
    s0 = plda.smooth(m, 0.0)
    assert s0.psi.tobytes() == m.psi.tobytes() and s0.transform.tobytes() == m.transform.tobytes() and s0.mean.tobytes() == m.mean.tobytes()
    s = plda.smooth(m, 0.3)
    mean, transform, psi = ref_plda.smooth(m.mean, m.transform, m.psi, 0.3)
    assert np.allclose(s.psi, psi, rtol=1e-15) and np.allclose(s.transform, transform, rtol=1e-15) and np.array_equal(s.mean, mean)
    assert np.allclose(s.psi, m.psi / (1.0 + 0.3 * m.psi), rtol=1e-15)
    with pytest.raises(ValueError):
        plda.smooth(m, -0.1)


def test_min_dcf_matches_brute_force():
    from tf_kaldi_speaker_amd import scoring
    rng = np.random.default_rng(9)
    s = np.concatenate([np.round(rng.normal(1.0, 1.0, 120), 1), np.round(rng.normal(-1.0, 1.0, 380), 1)])     # ties
    t = np.concatenate([np.ones(120, bool), np.zeros(380, bool)])
    for p_target, c_miss, c_fa in ((0.01, 1.0, 1.0), (0.001, 1.0, 1.0), (0.5, 1.0, 1.0), (0.05, 10.0, 1.0), (0.3, 1.0, 2.5)):
        got, thr = scoring.min_dcf(s, t, p_target, c_miss, c_fa)
        want = ref_plda.min_dcf(s, t, p_target, c_miss, c_fa)
        assert abs(got - want) <= 1e-15 * max(1.0, want), (p_target, got, want)
        # the returned threshold realises the minimum
        p_miss, p_fa = np.mean(s[t] < thr), np.mean(s[~t] >= thr)
        cost = (c_miss * p_miss * p_target + c_fa * p_fa * (1 - p_target)) / min(c_miss * p_target, c_fa * (1 - p_target))
        assert abs(cost - got) <= 1e-12
    assert 0.0 < scoring.min_dcf(s, t, 0.5)[0] < 1.0
    dcf, thr = scoring.min_dcf([3.0, 2.5, 2.5, -1.0, -1.0, -4.0], [True, True, True, False, False, False], 0.01)
    assert dcf == 0.0 and -1.0 < thr <= 2.5
    assert scoring.min_dcf([1.0, 2.0], [False, True], 0.01, 1.0, 1.0)[0] == 0.0
    assert scoring.min_dcf([2.0, 1.0], [False, True], 0.01)[0] == 1.0          # never better than the constant decision
    with pytest.raises(ValueError):
        scoring.min_dcf([1.0, 2.0], [True, True])
    with pytest.raises(ValueError):
        scoring.min_dcf([1.0, 2.0], [True, False], p_target=1.5)


def test_eer_from_histograms_default_range_is_unchanged():
    """Three bins by hand (tests/test_scoring_host.py): eer 3/8 at threshold 0 over [-1, 1]; the same counts over
    [-30, 60) cross at the same place of the range, and a fixed pair keeps the exact values of the two-argument call."""
    from tf_kaldi_speaker_amd import scoring
    assert scoring.eer_from_histograms([1, 1, 2], [2, 1, 1]) == (0.375, 0.0)
    eer, thr = scoring.eer_from_histograms([1, 1, 2], [2, 1, 1], lo=-30.0, hi=60.0)
    assert eer == 0.375 and abs(thr - 15.0) < 1e-12
    rng = np.random.default_rng(2)
    hs, hd = rng.integers(0, 50, 256) * (np.arange(256) > 100), rng.integers(0, 500, 256) * (np.arange(256) < 160)
    a = scoring.eer_from_histograms(hs, hd)
    b = scoring.eer_from_histograms(hs, hd, -1.0, 1.0)
    assert a == b
    g = np.concatenate([[0], np.cumsum(hs)]) / hs.sum() - (hd.sum() - np.concatenate([[0], np.cumsum(hd)])) / hd.sum()
    k = int(np.argmax(g[1:] >= 0.0))
    t = -g[k] / (g[k + 1] - g[k])
    assert a[1] == float(-1.0 + (2.0 / 256) * (k + t))                         # the expression of the two-argument version
    with pytest.raises(ValueError):
        scoring.eer_from_histograms(hs, hd, 1.0, 1.0)


def test_score_plda_argument_errors_exit_2(tmp_path, repo_root):
    (tmp_path / "trials").write_text("a b\nc d\n")
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""), HIP_VISIBLE_DEVICES="")
    base = [sys.executable, "-m", "tf_kaldi_speaker_amd.score_plda"]
    tail = ["no_such_plda", "ark:no_such.ark", "ark:no_such.ark", str(tmp_path / "trials"), "-"]
    for extra in (["--eer"], ["--min-dcf", "0.01"]):
        r = subprocess.run(base + extra + tail, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, r.stderr[-2000:]
        assert "target / nontarget" in r.stderr
    for bad in ("abc", "1.5", "0.01,0", "0.01,1,1,1", ""):
        r = subprocess.run(base + ["--min-dcf", bad] + tail, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, (bad, r.stderr[-2000:])
        assert "P_TARGET" in r.stderr
    r = subprocess.run(base + ["--smoothing", "2"] + tail, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2


def test_library_refuses_bad_plda_arguments_before_the_first_hip_call():
    import ctypes
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    buf, dbuf, ibuf = (ctypes.c_float * 4096)(), (ctypes.c_double * 4096)(), (ctypes.c_int32 * 16)()
    out = (ctypes.c_float * 4096)()
    h1, h2 = (ctypes.c_uint64 * 256)(), (ctypes.c_uint64 * 256)()
    p, dp, ip, op = (ctypes.cast(b, ctypes.c_void_p) for b in (buf, dbuf, ibuf, out))
    ph1, ph2 = ctypes.cast(h1, ctypes.c_void_p), ctypes.cast(h2, ctypes.c_void_p)
    for k in (0, 2049):
        assert lib.xv_plda_matrix(0, p, max(k, 1), 1, p, p, max(k, 1), 1, None, k, op, 1, None) == _lib.XV_ERR_UNSUPPORTED
        assert lib.xv_plda_pairs(0, p, max(k, 1), 1, p, p, max(k, 1), 1, None, k, ip, ip, 1, op, None) == _lib.XV_ERR_UNSUPPORTED
        assert lib.xv_plda_histogram(0, p, max(k, 1), 1, p, ip, p, max(k, 1), 1, None, ip, k, -1.0, 1.0, 256, ph1, ph2, None) == _lib.XV_ERR_UNSUPPORTED
    assert lib.xv_plda_matrix(0, p, 4, 1, None, p, 4, 1, None, 4, op, 1, None) == _lib.XV_ERR_INVALID              # rho missing
    assert lib.xv_plda_matrix(0, p, 3, 1, p, p, 4, 1, None, 4, op, 1, None) == _lib.XV_ERR_INVALID                 # lda < k
    assert lib.xv_plda_histogram(0, p, 4, 1, p, ip, p, 4, 1, None, ip, 4, 1.0, 1.0, 256, ph1, ph2, None) == _lib.XV_ERR_INVALID
    assert lib.xv_plda_histogram(0, p, 4, 1, p, ip, p, 4, 1, None, ip, 4, -1.0, 1.0, 1000, ph1, ph2, None) == _lib.XV_ERR_INVALID
    assert lib.xv_plda_prepare(0, p, 4, 1, 4, None, 0, 5, 1, 0, 0, dp, dp, 1, None, op, 5, None, 0, None, None) == _lib.XV_ERR_INVALID   # d_in != d
    assert lib.xv_plda_prepare(0, p, 4, 1, 4, p, 5, 4, 1, 0, 0, dp, dp, 1, None, p, 4, None, 0, None, None) == _lib.XV_ERR_INVALID      # in place
    assert lib.xv_plda_prepare(0, p, 4, 1, 4, None, 0, 4, 3, 0, 0, dp, dp, 1, None, op, 4, None, 0, None, None) == _lib.XV_ERR_INVALID   # norm
    assert lib.xv_plda_prepare(0, p, 4, 1, 4, None, 0, 4, 1, 0, 1, dp, dp, 1, None, None, 0, op, 4, None, None) == _lib.XV_ERR_INVALID   # ldp < 2 d
    assert lib.xv_plda_prepare(0, p, 4096, 1, 4096, None, 0, 4096, 1, 0, 0, dp, dp, 1, None, op, 4096, None, 0, None, None) == _lib.XV_ERR_UNSUPPORTED


def test_plda_without_a_device_raises(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from tf_kaldi_speaker_amd import plda
    m = _model(8)
    x = np.ones((4, 8), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        plda.prepare_test(m, x)
    with pytest.raises(ValueError, match="dimension"):
        plda.prepare_enroll(m, np.ones((4, 9), np.float32))
    with pytest.raises(ValueError, match="num_utts"):
        plda.prepare_enroll(m, x, num_utts=[1, 2, 3])
    with pytest.raises(ValueError, match=">= 1"):
        plda.prepare_enroll(m, x, num_utts=[1, 2, 0, 4])
