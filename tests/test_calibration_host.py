"""Host side of the calibration (tf_kaldi_speaker_amd.calibration / .calibrate): the numpy oracle against itself, the Newton
driver on the oracle's statistics, the argument checks, the model file, the score-file join and the one reference-held pin,
equal-weight fusion against the stored output of the reference's misc/utils/average_score.py.  No GPU."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_calibration as R  # noqa: E402

from tf_kaldi_speaker_amd import calibrate, calibration, scoring  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ the oracle against itself
@pytest.mark.parametrize("k", [1, 3, 8])
def test_oracle_gradient_and_hessian_match_central_differences(k):
    s, t = R.fixture(k, 300, 40 + k)
    f = R.objective(s, t, 0.05)
    rs = np.random.RandomState(k)
    theta = np.concatenate([np.full(k, 1.0 / k), [0.0]]) + 0.05 * rs.standard_normal(k + 1) / (1.0 + np.arange(k + 1))
    F, g, H = f(theta)
    assert np.allclose(H, H.T, rtol=1e-13, atol=0.0)
    for i in range(k + 1):
        e = np.zeros(k + 1)
        e[i] = 1e-5
        num_g = (f(theta + e)[0] - f(theta - e)[0]) / 2e-5
        assert abs(num_g - g[i]) <= 1e-8 * max(1.0, abs(g[i])) + 1e-6 * abs(g[i]), (i, num_g, g[i])
        num_h = (f(theta + e)[1] - f(theta - e)[1]) / 2e-5
        assert np.all(np.abs(num_h - H[i]) <= 1e-6 * np.abs(H[i]) + 1e-8 * np.abs(H).max()), (i, num_h, H[i])


def test_oracle_sums_skip_and_count_rows_that_are_not_finite():
    s, t = R.fixture(2, 50, 3)
    s2 = np.concatenate([s, [[np.inf, 0.0], [0.0, np.nan]]]).astype(np.float32)
    t2 = np.concatenate([t, [True, False]])
    a = R.stats(s, t, [0.5, 0.5, 0.0], -1.0, 0.1, 0.2, [0.0])
    b = R.stats(s2, t2, [0.5, 0.5, 0.0], -1.0, 0.1, 0.2, [0.0])
    assert (a["bad"], b["bad"]) == (0, 2)
    for key in ("F", "n_tar", "n_non"):
        assert a[key] == b[key]
    for key in ("g", "H", "miss", "fa"):
        assert np.array_equal(a[key], b[key])


# ------------------------------------------------------------------------------------------------ the Newton driver
@pytest.mark.parametrize("k,prior", R.FIT_CASES)
def test_newton_on_oracle_statistics_converges(k, prior):
    s, t, theta, report, lam = R.fit_case(k, prior, calibration.newton)
    assert lam >= 1e-4, lam                                   # the bounds of the GPU fit test mean nothing without it
    assert 1 <= report.iterations <= 50 and report.decrement <= 1e-14 and np.isfinite(report.F)
    assert np.all(np.isfinite(theta))
    F, g, H = R.objective(s, t, prior)(theta)
    assert F == report.F
    assert float(g @ np.linalg.solve(H, g)) <= 4e-14
    # a minimum: the objective does not fall along any coordinate
    for i in range(k + 1):
        for sign in (-1.0, 1.0):
            e = np.zeros(k + 1)
            e[i] = sign * 1e-3
            assert R.objective(s, t, prior)(theta + e)[0] > F
    # the start point is what the issue states, and the first evaluation is made there
    seen = []

    def spy(th):
        seen.append(th.copy())
        return R.objective(s, t, prior)(th)
    calibration.newton(spy, k, max_iter=60)
    assert np.array_equal(seen[0], np.concatenate([np.full(k, 1.0 / k), [0.0]]))


def test_separable_scores_raise_within_max_iter():
    rs = np.random.RandomState(0)
    t = rs.rand(400) < 0.3
    s = np.where(t, 1.0 + rs.rand(400), -1.0 - rs.rand(400)).astype(np.float32)[:, None]        # every target above every non-target
    calls = []

    def stats(theta):
        calls.append(1)
        return R.objective(s, t, 0.05)(theta)
    with pytest.raises(RuntimeError):
        calibration.newton(stats, 1, max_iter=50)
    assert len(calls) <= 51 * 42                              # max_iter steps of at most 41 halvings: it cannot loop forever


def test_newton_refuses_statistics_that_are_not_finite_or_not_positive_definite():
    with pytest.raises(RuntimeError):
        calibration.newton(lambda th: (float("inf"), np.ones(2), np.eye(2)), 1)
    with pytest.raises(RuntimeError):
        calibration.newton(lambda th: (1.0, np.ones(2), -np.eye(2)), 1)
    with pytest.raises(RuntimeError):                          # a gradient that promises a decrease the objective never delivers
        calibration.newton(lambda th: (1.0, np.ones(2), np.eye(2)), 1)


def test_argument_checks_come_before_the_device():
    s, t = R.fixture(2, 20, 1)
    for prior in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            calibration.fit(s, t, prior=prior)
        with pytest.raises(ValueError):
            calibration.Model([1.0], 0.0, prior)
    for targets in (np.ones(20, bool), np.zeros(20, bool)):
        with pytest.raises(ValueError):
            calibration.fit(s, targets)
        with pytest.raises(ValueError):
            calibration.cllr(s[:, 0], targets)
        with pytest.raises(ValueError):
            calibration.act_dcf(s[:, 0], targets, 0.01)
    with pytest.raises(ValueError):
        calibration.act_dcf(s[:, 0], t, 1.0)
    with pytest.raises(ValueError):
        calibration.Model(np.ones(9))
    with pytest.raises(ValueError):
        calibration.Model([])


# ------------------------------------------------------------------------------------------------ files
def test_model_file_round_trip_is_exact(tmp_path):
    rs = np.random.RandomState(2)
    m = calibration.Model(rs.standard_normal(8) * 10.0 ** rs.randint(-8, 8, 8), math.pi * 1e-7, 1.0 / 3.0)
    path = str(tmp_path / "model")
    calibration.write_model(path, m)
    text = open(path).read()
    assert re.fullmatch(r"prior \S+\nbias \S+\n(weight \S+\n){8}", text)
    back = calibration.read_model(path)
    assert np.array_equal(back.weights, m.weights) and back.bias == m.bias and back.prior == m.prior
    for bad in ("prior 0.5\nbias 0\n", "prior 0.5\nweight 1\n", "bias 0\nweight 1\n", "prior 0.5\nbias 0\nweight x\n",
                "prior 0.5\nprior 0.5\nbias 0\nweight 1\n", "prior 2\nbias 0\nweight 1\n", "prior 0.5\nbias 0\nweight 1 2\n"):
        open(path, "w").write(bad)
        with pytest.raises(ValueError):
            calibration.read_model(path)


def test_score_file_join_skips_and_counts_missing_trials(tmp_path, capsys):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    open(a, "w").write("s1 u1 0.5\ns1 u2 -1\n\ns2 u1 2e-3\ns2 u3 7\n")
    open(b, "w").write("s2 u1 4\ns1 u1 1.5\ns9 u9 0\ns2 u3 -7\n")
    pa, ta = calibrate.read_scores(a)
    pb, tb = calibrate.read_scores(b)
    assert pa == [("s1", "u1"), ("s1", "u2"), ("s2", "u1"), ("s2", "u3")] and ta[("s2", "u1")] == 2e-3
    trials = [("s1", "u1"), ("s3", "u1"), ("s2", "u3"), ("s1", "u2"), ("s2", "u1")]
    kept, s = calibrate.join_scores("tool", trials, [ta, tb])
    assert kept == [0, 2, 4]
    assert s.dtype == np.float32 and np.array_equal(s, np.array([[0.5, 1.5], [7, -7], [2e-3, 4]], np.float32))
    assert "tool: skipped 2 of 5 trials" in capsys.readouterr().err
    kept, s = calibrate.join_scores("tool", trials, [ta])
    assert kept == [0, 2, 3, 4] and s.shape == (4, 1)
    assert calibrate.join_scores("tool", [("x", "y")], [ta, tb]) == (None, None)
    assert "no trial is left" in capsys.readouterr().err
    open(a, "w").write("s1 u1 0.5 extra\n")
    with pytest.raises(ValueError):
        calibrate.read_scores(a)
    # nothing left: a non-zero exit status, before any device is needed
    open(a, "w").write("s1 u1 0.5\n")
    open(b, "w").write("k1 k2 target\nk3 k4 nontarget\n")
    assert calibrate.main(["train", b, str(tmp_path / "m"), a]) == 1
    assert calibrate.main(["eval", b, a]) == 1
    calibration.write_model(str(tmp_path / "m"), calibration.Model([1.0, 1.0]))
    assert calibrate.main(["apply", str(tmp_path / "m"), str(tmp_path / "o"), a]) == 2        # one file for two systems


# ------------------------------------------------------------------------------------------------ the metrics
def test_act_dcf_is_never_below_min_dcf():
    rs = np.random.RandomState(7)
    for trial in range(20):
        n = int(rs.randint(2, 400))
        t = rs.rand(n) < 0.3
        t[0], t[1] = True, False
        l = (rs.standard_normal(n) * 4.0 + np.where(t, 1.0, -1.0) * rs.rand() * 5.0).astype(np.float32)
        if trial % 3 == 0:
            l = np.round(l)                                   # ties, and scores equal to a threshold
        for p, cm, cf in ((0.01, 1.0, 1.0), (0.5, 1.0, 1.0), (0.001, 10.0, 1.0), (0.05, 1.0, 3.0)):
            act = R.act_dcf(l, t, p, cm, cf)
            assert act >= scoring.min_dcf(l, t, p, cm, cf)[0], (trial, p)
    # a threshold that equals a score: llr >= eta is a false accept, llr < eta is not a miss
    l, t = np.array([0.0, 0.0], np.float32), np.array([True, False])
    assert R.act_dcf(l, t, 0.5) == 1.0 / 0.5 * 0.5


def test_cllr_of_llr_zero_is_exactly_one():
    t = np.array([True] * 4 + [False] * 8)
    assert R.cllr(np.zeros(12, np.float32), t) == 1.0
    s, t = R.fixture(1, 500, 9)
    st = R.stats(s, t, [1.0, 0.0], 0.0, 0.5 / t.sum(), 0.5 / (~t).sum())
    assert abs(st["F"] / math.log(2.0) - R.cllr(s[:, 0], t)) <= 1e-14        # Cllr is F / ln 2 at prior 0.5, K = 1, theta = (1, 0)


def test_equal_weight_fusion_reproduces_the_reference_average_score():
    def column(name):
        return calibrate.read_scores(os.path.join(GOLDEN, "average_score_%s.txt" % name))
    (pa, ta), (pb, tb), (po, to) = column("a"), column("b"), column("out")
    assert pa == pb == po and len(pa) == 40
    kept, s = calibrate.join_scores("test", pa, [ta, tb])
    m = calibration.Model([0.5, 0.5], 0.0)
    got = R.fuse(s, m.theta).astype(np.float64)
    want = np.array([to[p] for p in pa])
    err = np.abs(got - want)
    bound = 5e-7 + 2.0 ** -24 * np.abs(want)
    assert np.all(err <= bound), (err / bound).max()
    assert np.abs(want).max() > 10.0 and np.abs(want).min() < 0.1       # both terms of the bound are the larger one somewhere


# ------------------------------------------------------------------------------------------------ exports
def test_calibration_symbols_are_declared_listed_and_exported(repo_root):
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    assert "calibrate.hip" in g.SOURCES and g.NO_SCRATCH["calibrate.hip"] == "logreg_stats_kernel"
    w = lib.xv_logreg_workspace
    assert w(0, 1) == 0 and w(0, 8) == 0
    for k in (1, 3, 8):
        per = (1 + (k + 1) + (k + 1) * (k + 2) // 2 + 19) * 8
        assert [w(n, k) for n in (1, 16384, 16385, 70000)] == [per, per, 2 * per, 5 * per]
    assert w(5, 0) == _lib.XV_ERR_UNSUPPORTED and w(5, 9) == _lib.XV_ERR_UNSUPPORTED and w(-1, 1) == _lib.XV_ERR_INVALID
    # argument checks come before the first HIP call: they answer without a device
    f = lib.xv_logreg_stats
    theta = (ctypes.c_double * 9)()
    assert f(0, 8, 9, 4, 9, 8, theta, 0.0, 1.0, 1.0, None, 0, 8, 8, 8, 1 << 20, None) == _lib.XV_ERR_UNSUPPORTED
    assert f(0, 8, 2, 4, 3, 8, theta, 0.0, 1.0, 1.0, None, 0, 8, 8, 8, 1 << 20, None) == _lib.XV_ERR_INVALID       # lds < k
    assert f(0, 8, 3, 4, 3, 8, theta, 0.0, 1.0, 1.0, None, 9, 8, 8, 8, 1 << 20, None) == _lib.XV_ERR_INVALID       # 9 thresholds
    assert f(0, 8, 3, 4, 3, 8, theta, 0.0, 1.0, 1.0, None, 0, 8, 8, 8, 8, None) == _lib.XV_ERR_WORKSPACE
    h = lib.xv_score_fuse
    assert h(0, 8, 9, 4, 9, theta, 8, None) == _lib.XV_ERR_UNSUPPORTED and h(0, 8, 2, 4, 3, theta, 8, None) == _lib.XV_ERR_INVALID
