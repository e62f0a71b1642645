"""CPU: cohort score normalisation without a device: the float64 oracle's own invariants, snorm.normalize against numbers
worked out by hand, the argument checks of xv_cohort_stats through the built library (they come before the first HIP call),
the workspace size, and the parsing of the new options of score_cos / score_plda."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_snorm  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ oracle
def test_oracle_top_k_m_is_top_k_0():
    rng = np.random.default_rng(0)
    s = rng.standard_normal((7, 31))
    a, b = ref_snorm.cohort_stats(s, 31), ref_snorm.cohort_stats(s, 0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_oracle_tripled_cohort_leaves_the_statistics():
    rng = np.random.default_rng(1)
    s = rng.standard_normal((5, 40))
    s3 = np.concatenate([s, s, s], axis=1)
    for k in (3, 12, 30):
        m1, d1, c1 = ref_snorm.cohort_stats(s, k // 3)
        m3, d3, c3 = ref_snorm.cohort_stats(s3, k)
        assert np.allclose(m1, m3, rtol=1e-14, atol=0) and np.allclose(d1, d3, rtol=1e-12, atol=1e-15)
        assert np.array_equal(3 * c1, c3)


def test_oracle_by_hand_with_exclusion():
    s = np.array([[1.0, 5.0, 3.0, 9.0], [2.0, 2.0, 2.0, 2.0]])
    mean, std, count = ref_snorm.cohort_stats(s, 2, labels=["a", "b"], cohort_labels=["x", "x", "x", "a"])
    assert list(count) == [2, 2]
    assert mean[0] == 4.0 and std[0] == 1.0            # 9 is excluded for row 0: top two are 5 and 3
    assert mean[1] == 2.0 and std[1] == 0.0
    mean, std, count = ref_snorm.cohort_stats(s, 3, labels=["a", "b"], cohort_labels=["a", "a", "a", "a"])
    assert count[0] == 0 and np.isnan(mean[0]) and np.isnan(std[0]) and count[1] == 3


# ------------------------------------------------------------------------------------------------ normalize
def _stats(mean, std):
    from tf_kaldi_speaker_amd import snorm
    return snorm.CohortStats(np.array(mean, np.float32), np.array(std, np.float32), np.ones(len(mean), np.int32))


def test_normalize_modes_by_hand():
    from tf_kaldi_speaker_amd import snorm
    ze, zt = _stats([1.0, 0.0], [2.0, 0.5]), _stats([0.5, -1.0, 3.0], [0.25, 4.0, 1.0])
    s = np.array([3.0, 1.0, -1.0], np.float32)
    ia, ib = [0, 1, 0], [1, 0, 2]
    z = snorm.normalize(s, ia, ib, ze, zt, mode="z")
    t = snorm.normalize(s, ia, ib, ze, zt, mode="t")
    both = snorm.normalize(s, ia, ib, ze, zt, mode="s")
    assert np.array_equal(z, np.array([1.0, 2.0, -1.0], np.float32))
    assert np.array_equal(t, np.array([1.0, 2.0, -4.0], np.float32))
    assert np.array_equal(both, np.array([1.0, 2.0, -2.5], np.float32))
    assert np.array_equal(snorm.normalize(s, ia, ib, ze, None, mode="z"), z)      # the unused side may be absent
    assert np.array_equal(snorm.normalize(s, ia, ib, None, zt, mode="t"), t)
    want = ref_snorm.normalize(s, np.array(ia), np.array(ib), (ze.mean.astype(float), ze.std.astype(float)),
                               (zt.mean.astype(float), zt.std.astype(float)), "s")
    assert np.array_equal(both.astype(np.float64), want)
    import torch
    tt = snorm.normalize(torch.from_numpy(s), ia, ib, ze, zt, mode="s")
    assert isinstance(tt, torch.Tensor) and np.array_equal(tt.numpy(), both)
    with pytest.raises(ValueError):
        snorm.normalize(s, ia, ib, ze, zt, mode="as2")
    with pytest.raises(ValueError):
        snorm.normalize(s, ia, ib, None, zt, mode="s")


@pytest.mark.parametrize("bad", [0.0, float("nan")])
def test_normalize_refuses_a_used_row_without_a_std(bad):
    from tf_kaldi_speaker_amd import snorm
    ze, zt = _stats([1.0, 0.0, 2.0], [2.0, bad, 1.0]), _stats([0.5, -1.0], [0.25, 4.0])
    s = np.array([3.0, 1.0], np.float32)
    with pytest.raises(ValueError, match="enrolment row 1 "):
        snorm.normalize(s, [0, 1], [1, 0], ze, zt, mode="s")
    out = snorm.normalize(s, [0, 2], [1, 0], ze, zt, mode="s")                     # row 1 is not used: silence
    assert np.all(np.isfinite(out))
    out = snorm.normalize(s, [0, 1], [1, 0], ze, zt, mode="t")                     # nor is the enrolment side under "t"
    assert np.all(np.isfinite(out))
    with pytest.raises(ValueError, match="test row 0 "):
        snorm.normalize(s, [0, 2], [1, 0], zt._replace(), _stats([0.5, -1.0], [bad, 4.0]), mode="t")


# ------------------------------------------------------------------------------------------------ C ABI
def test_library_refuses_bad_arguments_before_the_first_hip_call(lib):
    """top_k > m is XV_ERR_INVALID, k = 0 and k = 2049 are XV_ERR_UNSUPPORTED, labels on one side only are XV_ERR_INVALID and
    a workspace one byte short is XV_ERR_WORKSPACE: on a box without a GPU too, because the checks come before any HIP call."""
    from tf_kaldi_speaker_amd import _lib
    buf = (ctypes.c_float * 64)()
    ibuf = (ctypes.c_int32 * 64)()
    p, ip = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    n, m, k = 2, 5, 4
    need = lib.xv_cohort_stats_workspace(n, m, 0)
    assert need >= 128 * m * 4

    def call(n=n, m=m, k=k, top_k=0, la=None, lb=None, ws=p, ws_bytes=need, mean=p, std=p, a=p, lda=None):
        return lib.xv_cohort_stats(0, a, max(k, 1) if lda is None else lda, n, None, la, p, max(k, 1), m, None, lb, k, top_k, mean,
                                   std, None, ws, ws_bytes, None)
    assert call(top_k=m + 1) == _lib.XV_ERR_INVALID
    assert call(top_k=-1) == _lib.XV_ERR_INVALID
    assert call(k=0) == _lib.XV_ERR_UNSUPPORTED
    assert call(k=2049) == _lib.XV_ERR_UNSUPPORTED
    assert call(la=ip) == _lib.XV_ERR_INVALID
    assert call(lb=ip) == _lib.XV_ERR_INVALID
    assert call(ws_bytes=need - 1) == _lib.XV_ERR_WORKSPACE
    assert call(ws=None) == _lib.XV_ERR_WORKSPACE
    assert call(mean=None) == _lib.XV_ERR_INVALID
    assert call(a=None) == _lib.XV_ERR_INVALID
    assert call(lda=k - 1) == _lib.XV_ERR_INVALID
    assert call(m=2 ** 31) == _lib.XV_ERR_INVALID
    assert call(n=0, ws=None, ws_bytes=0, mean=None, std=None) == _lib.XV_OK     # nothing to do, nothing touched
    assert b"xv_cohort_stats" in lib.xv_last_error(None)


def test_workspace_is_monotone_and_at_least_one_panel(lib):
    last = -1
    for m in (0, 1, 3, 4, 5, 127, 128, 129, 1000, 12288, 12289, 100000, 2 ** 31 - 1):
        w = lib.xv_cohort_stats_workspace(1000, m, 300 if m >= 300 else 0)
        assert w >= 128 * m * 4 and w >= last
        assert w == lib.xv_cohort_stats_workspace(1, m, 0)          # one panel serves any n and top_k
        last = w
    assert lib.xv_cohort_stats_workspace(-1, 5, 0) < 0
    assert lib.xv_cohort_stats_workspace(5, 2 ** 31, 0) < 0


def test_cohort_stats_without_a_device_raises(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from tf_kaldi_speaker_amd import snorm
    x = np.zeros((2, 4), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        snorm.cohort_stats(x, x, top_k=1)
    with pytest.raises(ValueError):
        snorm.cohort_stats(x, np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError):
        snorm.cohort_stats(x, x, labels=[0, 1])


# ------------------------------------------------------------------------------------------------ command line
def _parser(tool):
    import argparse
    from tf_kaldi_speaker_amd import score_cos
    ap = argparse.ArgumentParser(prog=tool)
    score_cos.add_snorm_options(ap)
    return ap, score_cos


def test_option_parsing():
    ap, score_cos = _parser("score_cos")
    a = ap.parse_args([])
    score_cos.check_snorm_options(ap, a)
    assert a.cohort == "" and a.norm is None and a.top_k is None and a.exclude_utt2spk == ""
    a = ap.parse_args(["--cohort", "ark:c.ark"])
    score_cos.check_snorm_options(ap, a)
    assert (a.cohort, a.norm, a.top_k, a.exclude_utt2spk) == ("ark:c.ark", "s", 0, "")
    a = ap.parse_args(["--cohort", "scp:c.scp", "--norm", "z", "--top-k", "300", "--exclude-utt2spk", "utt2spk"])
    score_cos.check_snorm_options(ap, a)
    assert (a.cohort, a.norm, a.top_k, a.exclude_utt2spk) == ("scp:c.scp", "z", 300, "utt2spk")
    for argv in (["--norm", "s"], ["--top-k", "0"], ["--exclude-utt2spk", "f"], ["--cohort", "c", "--top-k", "-1"]):
        with pytest.raises(SystemExit):
            score_cos.check_snorm_options(ap, ap.parse_args(argv))
    with pytest.raises(SystemExit):
        ap.parse_args(["--cohort", "c", "--norm", "as2"])


def test_exclusion_labels(tmp_path):
    from tf_kaldi_speaker_amd import score_cos
    (tmp_path / "utt2spk").write_text("e0 A\nt1 A\nc0 A\nc2 B\n\n")
    spk = score_cos.read_utt2spk(str(tmp_path / "utt2spk"))
    l1, l2, lc = score_cos.exclusion_labels(spk, {"e0": 0, "e1": 1}, {"t0": 0, "t1": 1}, {"c0": 0, "c1": 1, "c2": 2, "e1": 3})
    assert l1[0] == l2[1] == lc[0] and lc[2] != lc[0]
    # keys that are not in the file are never excluded, not even by the same key in another table
    assert l1[1] not in set(lc) and l2[0] not in set(lc) and len(set(lc)) == 4
    (tmp_path / "bad").write_text("e0 A extra\n")
    with pytest.raises(ValueError):
        score_cos.read_utt2spk(str(tmp_path / "bad"))


@pytest.mark.parametrize("tool", ["score_cos", "score_plda"])
def test_both_tools_know_the_options(tool, capsys):
    import importlib
    mod = importlib.import_module("tf_kaldi_speaker_amd." + tool)
    with pytest.raises(SystemExit) as e:
        mod.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--cohort", "--norm", "--top-k", "--exclude-utt2spk"):
        assert opt in text


def test_run_without_a_cohort_is_the_existing_path(lib, tmp_path, monkeypatch):
    """score_cos on a small table without --cohort: the device calls are stood in for by numpy (no GPU here), and the bytes
    written are those of the same write_scores call on the same scores; nothing of snorm is touched."""
    from tf_kaldi_speaker_amd import native_ark, score_cos, scoring, snorm
    rng = np.random.default_rng(5)
    keys = ["utt%02d" % i for i in range(12)]
    x = rng.standard_normal((12, 16)).astype(np.float32)
    w = native_ark.VectorWriter("ark:%s" % (tmp_path / "x.ark"))
    w.write(keys, x)
    w.close()
    lines = ["%s %s %s" % (keys[i], keys[j], "target" if i % 3 == j % 3 else "nontarget") for i in range(12) for j in range(i)]
    (tmp_path / "trials").write_text("\n".join(lines) + "\n")

    def prepare(v, mean=None, transform=None, normalize=True, eps=0.0, device=0, as_tensor=False):
        v = np.asarray(v, np.float32)
        return v / np.sqrt(np.sum(v * v, axis=1, keepdims=True))

    def pairs(a, b, ia, ib, device=0, as_tensor=False):
        return np.sum(a[ia] * b[ib], axis=1, dtype=np.float32)

    def never(*a, **k):
        raise AssertionError("score normalisation was entered without --cohort")
    monkeypatch.setattr(scoring, "prepare", prepare)
    monkeypatch.setattr(scoring, "cosine_pairs", pairs)
    monkeypatch.setattr(snorm, "cohort_stats", never)
    monkeypatch.setattr(snorm, "normalize", never)
    rc = score_cos.main(["--eer", str(tmp_path / "trials"), "ark:%s" % (tmp_path / "x.ark"), "ark:%s" % (tmp_path / "x.ark"),
                         str(tmp_path / "scores")])
    assert rc == 0
    k1, k2 = [ln.split()[0] for ln in lines], [ln.split()[1] for ln in lines]
    row = {k: i for i, k in enumerate(keys)}
    xp = prepare(x)
    want = pairs(xp, xp, np.array([row[k] for k in k1]), np.array([row[k] for k in k2]))
    score_cos.write_scores("score_cos", str(tmp_path / "want"), k1, k2, list(range(len(lines))), want)
    assert (tmp_path / "scores").read_bytes() == (tmp_path / "want").read_bytes()
