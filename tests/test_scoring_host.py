"""Host side of the cosine scoring feature (no GPU): EER from histograms, trial parsing, argument checks of the Python
layer and of the library (which come before the first HIP call), and the oracle of the feature against oracle/ref_post."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_score  # noqa: E402

from oracle import ref_post  # noqa: E402


def test_eer_perfect_separation_is_zero():
    from tf_kaldi_speaker_amd import scoring
    hs, hd = np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    hd[1], hd[2], hs[6] = 5, 7, 4
    eer, thr = scoring.eer_from_histograms(hs, hd)
    assert eer == 0.0
    assert -1.0 + 3 * 0.25 <= thr <= -1.0 + 6 * 0.25          # every threshold between the two groups has no error


def test_eer_identical_histograms_is_half():
    from tf_kaldi_speaker_amd import scoring
    h = np.array([1, 4, 2, 9, 3, 0, 5, 8], np.uint64)
    eer, _ = scoring.eer_from_histograms(h, h.copy())
    assert abs(eer - 0.5) < 1e-15


def test_eer_three_bins_by_hand():
    """nbins = 3 (edges -1, -1/3, 1/3, 1), h_same = [1, 1, 2], h_diff = [2, 1, 1].
    FRR at the edges 0..3: 0, 1/4, 1/2, 1;  FAR: 1, 1/2, 1/4, 0;  g = FRR - FAR: -1, -1/4, 1/4, 1.
    The first edge k + 1 with g >= 0 is 2, so the crossing bin is k = 1: t = (1/4) / (1/4 + 1/4) = 1/2,
    eer = 1/4 + (1/2)(1/2 - 1/4) = 3/8 (FAR side: 1/2 + (1/2)(1/4 - 1/2) = 3/8), threshold = -1/3 + (1/2)(2/3) = 0."""
    from tf_kaldi_speaker_amd import scoring
    eer, thr = scoring.eer_from_histograms([1, 1, 2], [2, 1, 1])
    assert abs(eer - 0.375) < 1e-15
    assert abs(thr) < 1e-15
    with pytest.raises(ValueError):
        scoring.eer_from_histograms([0, 0, 0], [2, 1, 1])


def test_exact_eer_matches_the_oracle_sweep():
    from tf_kaldi_speaker_amd import scoring
    rng = np.random.default_rng(5)
    same = np.round(rng.normal(0.3, 0.2, 300), 2)           # rounding makes ties
    diff = np.round(rng.normal(0.0, 0.2, 900), 2)
    got = scoring.exact_eer(np.concatenate([same, diff]), np.concatenate([np.ones(300, bool), np.zeros(900, bool)]))
    assert got == ref_score.exact_eer(same, diff)
    assert 0.1 < got < 0.4


def test_trials_parsing(tmp_path):
    from tf_kaldi_speaker_amd import scoring
    p = tmp_path / "trials"
    p.write_text("a b\n\n  \nc d\n")
    assert scoring.read_trials(str(p)) == (["a", "c"], ["b", "d"], None)
    p.write_text("a b target\nc d nontarget\n\ne f target\n")
    assert scoring.read_trials(str(p)) == (["a", "c", "e"], ["b", "d", "f"], [True, False, True])
    p.write_text("a b target\nc d nontarget\nbroken\n")
    with pytest.raises(ValueError, match=":3:"):
        scoring.read_trials(str(p))
    p.write_text("a b target\nc d maybe\n")
    with pytest.raises(ValueError, match=":2:"):
        scoring.read_trials(str(p))
    p.write_text("a b target\nc d\n")
    with pytest.raises(ValueError, match=":2:"):
        scoring.read_trials(str(p))


def test_transform_column_rule_raises_before_any_device_call():
    from tf_kaldi_speaker_amd import scoring
    assert scoring.check_transform(512, (200, 512)) == (200, 512)
    assert scoring.check_transform(512, (200, 513)) == (200, 513)
    x = np.zeros((3, 512), np.float32)
    for cols in (511, 514, 200):
        with pytest.raises(ValueError, match="columns"):       # a ValueError, not the RuntimeError of a missing device
            scoring.prepare(x, transform=np.zeros((200, cols), np.float32))
    with pytest.raises(ValueError):
        scoring.prepare(x, mean=np.zeros(511, np.float32))
    with pytest.raises(ValueError):
        scoring.score_histograms(x, np.zeros(3), nbins=1000)
    assert list(scoring.select_rows(1234, 500)) == list(range(0, 1234, 1234 // 500))
    assert list(scoring.select_rows(400, 500)) == list(range(400))


def test_library_refuses_bad_arguments_before_the_first_hip_call():
    """d = 0 and d = 2049 are XV_ERR_UNSUPPORTED, an nbins that is not a power of two and a transform with a wrong column
    count are XV_ERR_INVALID: on a box without a GPU too, because the checks come before any HIP call."""
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    ibuf = (ctypes.c_int32 * 16)()
    h1, h2 = (ctypes.c_uint64 * 65536)(), (ctypes.c_uint64 * 65536)()
    p, ip = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    ph1, ph2 = ctypes.cast(h1, ctypes.c_void_p), ctypes.cast(h2, ctypes.c_void_p)
    for d in (0, 2049, -3):
        assert lib.xv_score_matrix(0, p, max(d, 1), 1, p, max(d, 1), 1, d, p, 1, None) == _lib.XV_ERR_UNSUPPORTED
        assert lib.xv_score_pairs(0, p, max(d, 1), 1, p, max(d, 1), 1, d, ip, ip, 1, p, None) == _lib.XV_ERR_UNSUPPORTED
        assert lib.xv_score_histogram(0, p, max(d, 1), 1, ip, p, max(d, 1), 1, ip, d, 1, 256, ph1, ph2, None) == _lib.XV_ERR_UNSUPPORTED
    assert b"2048" in lib.xv_last_error(None)
    for nbins in (0, 128, 1000, 65537, 131072):
        assert lib.xv_score_histogram(0, p, 4, 1, ip, p, 4, 1, ip, 4, 1, nbins, ph1, ph2, None) == _lib.XV_ERR_INVALID
    # transform columns: d_in or d_in + 1
    assert lib.xv_score_prepare(0, p, 8, 1, 8, None, p, 10, 4, 10, 1, 0.0, ph1, 4, None) == _lib.XV_ERR_INVALID
    assert lib.xv_score_prepare(0, p, 8, 1, 8, None, None, 0, 4, 0, 1, 0.0, ph1, 4, None) == _lib.XV_ERR_INVALID      # d_out != d_in
    assert lib.xv_score_prepare(0, p, 8, 1, 8, None, p, 9, 4, 9, 1, 0.0, p, 4, None) == _lib.XV_ERR_INVALID          # in place
    assert lib.xv_score_matrix(0, None, 4, 1, p, 4, 1, 4, p, 1, None) == _lib.XV_ERR_INVALID
    assert lib.xv_score_matrix(0, p, 3, 1, p, 4, 1, 4, p, 1, None) == _lib.XV_ERR_INVALID                             # lda < d


def test_scoring_without_a_device_raises(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # what a box without a GPU answers
    from tf_kaldi_speaker_amd import scoring
    x = np.ones((4, 16), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.prepare(x)
    with pytest.raises(RuntimeError):
        scoring.cosine_matrix(x, x)
    with pytest.raises(RuntimeError):
        scoring.cosine_pairs(x, x, [0], [1])
    with pytest.raises(RuntimeError):
        scoring.score_histograms(x, [0, 0, 1, 1], nbins=256)
    with pytest.raises(RuntimeError):
        scoring.pairwise_eer(x, [0, 0, 1, 1])


def test_oracle_normalisation_agrees_with_ref_post():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((50, 64)) * np.exp2(rng.integers(-20, 21, (50, 1)))).astype(np.float32)
    x[7] = 0.0
    got = ref_score.prepare(x, normalize=True, eps=0.0)
    want = ref_post.normalize_length(x, scaleup=False)
    assert np.all(got[7] == 0.0)
    assert np.max(np.abs(got - want.astype(np.float64))) <= 2.0 ** -24       # ref_post rounds its result to float32
    assert np.max(np.abs(np.linalg.norm(got[np.arange(50) != 7], axis=1) - 1.0)) < 1e-14
    # the eps form of misc/utils.py:317 and the affine column of transform-vec
    e = ref_score.prepare(x[:3], eps=1e-12)
    assert np.allclose(e, x[:3].astype(np.float64) / np.sqrt(np.sum(x[:3].astype(np.float64) ** 2, axis=1, keepdims=True) + 1e-12), rtol=1e-15)
    t = rng.standard_normal((5, 65))
    y = ref_score.prepare(x[:3], mean=x[0], transform=t, normalize=False)
    assert np.allclose(y[0], t[:, -1])
