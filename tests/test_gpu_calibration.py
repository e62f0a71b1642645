"""xv_logreg_stats / xv_score_fuse (csrc/calibrate.hip) and tf_kaldi_speaker_amd.calibration on the GPU against the float64
numpy oracle tests/helpers/ref_calibration.py.

Bound of the statistics: for every entry of F, g and H, |gpu - oracle| <= 1e-12 * sum_i |term_i|, the oracle (math.fsum:
exactly rounded sums) supplying both sides.  Device exp and log1p in double are good to a few ulp and a term is a handful of
roundings (about 1e-15 relative); a thread adds at most 64 terms serially, and the trees above it are 6 + 2 + at most a few
levels deep (less than 1e-13); 1e-12 leaves three orders over that and is far below what a wrong term or a dropped row
would cause.  The one case of 65 chunks (more partials than the lanes of the wave that adds them) takes numpy's pairwise
sums as the oracle instead (error below 21 * 2^-53 of the same sum of absolute terms, for 2^20 rows: still 400 times below
the bound), to keep the test quick.  Counts are exact.

"theta at the optimum" is the oracle's own fit (calibration.newton on the oracle's statistics) of the host fixture of the
same K at prior 0.05: the scores of every N below are drawn by the same recipe, so that theta sits where the sigmoids are
neither saturated nor linear.  N = 2 is one trial of each class.

Bit-for-bit with rows that are not finite: a sum's order is fixed by the row numbers, so the list without the two rows is
the same list when they are its last two rows (asserted bit for bit); with the two rows in the middle every later row
changes its place in the order, and the bound above is asserted instead."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_calibration as R  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 16384                      # rows per workgroup of logreg_stats_kernel
SIZES = [2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 70001]
PRIOR = 0.05
TAU = math.log(PRIOR / (1.0 - PRIOR))


def _nd(k):
    return 1 + (k + 1) + (k + 1) * (k + 2) // 2


def raw_stats(sd, n, k, td, theta, tau, c_tar, c_non, thr=(), extra_ws=0):
    """xv_logreg_stats through the C ABI on device tensors, with a workspace of exactly the least size plus `extra_ws`,
    filled with 0xff -> (stats [nd] float64, counts [19] int64) as numpy."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    need = lib.xv_logreg_workspace(n, k)
    assert need >= 0
    ws = torch.full((need + extra_ws + 8,), 255, dtype=torch.uint8, device=sd.device)
    out = torch.full((_nd(k),), float("nan"), dtype=torch.float64, device=sd.device)
    cnt = torch.full((19,), -1, dtype=torch.int64, device=sd.device)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    stream = torch.cuda.current_stream(0).cuda_stream
    _lib.check(lib.xv_logreg_stats(0, C.c_void_p(sd.data_ptr()), sd.stride(0) if sd.dim() == 2 and n > 1 else max(k, sd.shape[-1]),
                                   n, k, C.c_void_p(td.data_ptr()), C.c_void_p(theta.ctypes.data), tau, c_tar, c_non,
                                   C.c_void_p(thr.ctypes.data) if thr.size else None, thr.size, C.c_void_p(out.data_ptr()),
                                   C.c_void_p(cnt.data_ptr()), C.c_void_p(ws.data_ptr()), need + extra_ws, C.c_void_p(stream)))
    return out.cpu().numpy(), cnt.cpu().numpy()


def unpack(o, k):
    H = np.zeros((k + 1, k + 1))
    H[np.triu_indices(k + 1)] = o[k + 2:]
    return o[0], o[1:k + 2], H + np.triu(H, 1).T


def on_device(s, t, pad=0):
    """scores -> device tensor; with `pad` the rows sit in a [n, k + pad] buffer whose other columns are NaN."""
    import torch
    s = np.asarray(s, dtype=np.float32)
    if pad:
        buf = np.full((s.shape[0], s.shape[1] + pad), np.nan, dtype=np.float32)
        buf[:, :s.shape[1]] = s
        sd = torch.from_numpy(buf).to("cuda:0")[:, :s.shape[1]]
    else:
        sd = torch.from_numpy(np.ascontiguousarray(s)).to("cuda:0")
    td = torch.from_numpy(np.ascontiguousarray(np.asarray(t) != 0).view(np.uint8)).to("cuda:0")
    return sd, td


def thetas(k):
    from tf_kaldi_speaker_amd import calibration
    return [np.concatenate([np.full(k, 1.0 / k), [0.0]]), R.fit_case(k, PRIOR, calibration.newton)[2]]


def thresholds(s, theta):
    lf = R.fuse(s, theta).astype(np.float64)
    return [lf[0], lf[1], 0.0, -3.5, 4.25, lf[len(lf) // 2], 1e30, -1e30]


def assert_close(got, want, k, what):
    F, g, H = unpack(got, k)
    assert np.all(np.isfinite(got)), what
    assert abs(F - want["F"]) <= 1e-12 * want["aF"], (what, "F", F, want["F"])
    assert np.all(np.abs(g - want["g"]) <= 1e-12 * want["ag"]), (what, "g", np.abs(g - want["g"]) / want["ag"])
    assert np.all(np.abs(H - want["H"]) <= 1e-12 * want["aH"]), (what, "H", np.abs(H - want["H"]) / want["aH"])
    return max(abs(F - want["F"]) / want["aF"], (np.abs(g - want["g"]) / want["ag"]).max(),
               (np.abs(H - want["H"]) / want["aH"]).max())


def assert_counts(cnt, want, nthr, what):
    assert (cnt[0], cnt[1], cnt[2]) == (want["n_tar"], want["n_non"], want["bad"]), what
    assert np.array_equal(cnt[3:3 + nthr], want["miss"]) and np.array_equal(cnt[11:11 + nthr], want["fa"]), what
    assert not cnt[3 + nthr:11].any() and not cnt[11 + nthr:].any(), what


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_stats_match_the_oracle(n, k):
    s, t = R.fixture(k, n, 100 * k + n % 97)
    c_tar, c_non = R.class_weights(t, PRIOR)
    worst = 0.0
    for which, theta in enumerate(thetas(k)):
        thr = thresholds(s, theta)
        want = R.stats(s, t, theta, TAU, c_tar, c_non, thr)
        assert want["bad"] == 0 and want["n_tar"] >= 1 and want["n_non"] >= 1
        for pad in (0, 3):
            sd, td = on_device(s, t, pad)
            got, cnt = raw_stats(sd, n, k, td, theta, TAU, c_tar, c_non, thr)
            worst = max(worst, assert_close(got, want, k, (n, k, which, pad)))
            assert_counts(cnt, want, 8, (n, k, which, pad))
    print("n %d k %d: worst |gpu - oracle| / sum |term| = %.3g" % (n, k, worst))


@pytest.mark.parametrize("k", [1, 3])
def test_stats_with_more_partials_than_one_wave_adds(k):
    n = 65 * CHUNK + 1
    s, t = R.fixture(k, n, 5 + k)
    c_tar, c_non = R.class_weights(t, PRIOR)
    theta = thetas(k)[1]
    thr = thresholds(s, theta)[:3]
    want = R.stats(s, t, theta, TAU, c_tar, c_non, thr, exact=False)
    sd, td = on_device(s, t)
    got, cnt = raw_stats(sd, n, k, td, theta, TAU, c_tar, c_non, thr)
    print("n %d k %d: worst %.3g" % (n, k, assert_close(got, want, k, (n, k))))
    assert_counts(cnt, want, 3, (n, k))


def test_stats_python_call_and_empty_list():
    import torch
    from tf_kaldi_speaker_amd import calibration
    s, t = R.fixture(3, 1000, 8)
    theta = thetas(3)[1]
    c_tar, c_non = R.class_weights(t, PRIOR)
    thr = thresholds(s, theta)[:5]
    sd, td = on_device(s, t, 3)
    raw, cnt = raw_stats(sd, 1000, 3, td, theta, TAU, c_tar, c_non, thr)
    for scores, targets in ((s, t), (sd, td), (sd, t)):
        st = calibration.logreg_stats(scores, targets, theta, PRIOR, thresholds=thr)
        F, g, H = unpack(raw, 3)
        assert st.F == F and np.array_equal(st.g, g) and np.array_equal(st.H, H)
        assert (st.n_tar, st.n_non, st.bad) == tuple(cnt[:3])
        assert np.array_equal(st.miss, cnt[3:8]) and np.array_equal(st.fa, cnt[11:16])
    # n = 0: zeros, and no workspace
    empty = torch.empty((0, 3), dtype=torch.float32, device="cuda:0")
    got, cnt = raw_stats(empty, 0, 3, torch.empty((0,), dtype=torch.uint8, device="cuda:0"), theta, TAU, 1.0, 1.0, thr)
    assert not got.any() and not np.signbit(got).any() and not cnt.any()
    with pytest.raises(calibration._lib.XvError) as e:
        calibration._lib.check(calibration._lib.load().xv_logreg_stats(0, None, 9, 0, 9, None, None, 0.0, 1.0, 1.0, None, 0, None,
                                                                     None, None, 0, None))
    assert e.value.code == calibration._lib.XV_ERR_UNSUPPORTED


def test_extreme_scores_stay_finite():
    s = np.array([[3e4], [-3e4], [3e4], [-3e4]], np.float32)
    t = np.array([True, True, False, False])
    sd, td = on_device(s, t)
    got, cnt = raw_stats(sd, 4, 1, td, [1.0, 0.0], TAU, 1.0, 1.0, [0.0])
    F, g, H = unpack(got, 1)
    assert np.all(np.isfinite(got))
    # softplus is its argument where that is positive and 0 elsewhere: rows 1 and 2 contribute -z and z
    assert F == (3e4 - TAU) + (3e4 + TAU)
    assert g[0] == 6e4 and g[1] == 0.0               # r = -1 for the target at -3e4, +1 for the non-target at +3e4, 0 elsewhere
    assert not H.any()
    assert tuple(cnt[:3]) == (2, 2, 0) and cnt[3] == 1 and cnt[11] == 1
    want = R.stats(s, t, [1.0, 0.0], TAU, 1.0, 1.0, [0.0])
    assert_close(got, dict(want, aH=np.ones((2, 2))), 1, "extremes")


def test_rows_that_are_not_finite_are_counted_and_left_out():
    k, n = 3, 300
    s, t = R.fixture(k, n, 21)
    theta = thetas(k)[1]
    c_tar, c_non = R.class_weights(t, PRIOR)
    thr = thresholds(s, theta)
    sd, td = on_device(s, t)
    clean, clean_cnt = raw_stats(sd, n, k, td, theta, TAU, c_tar, c_non, thr)
    bad_rows = np.array([[1.0, np.inf, 2.0], [np.nan, 0.0, 0.0]], np.float32)
    # the two rows last: the list without them is the same list, bit for bit
    s2, t2 = np.concatenate([s, bad_rows]), np.concatenate([t, [True, False]])
    sd2, td2 = on_device(s2, t2)
    got, cnt = raw_stats(sd2, n + 2, k, td2, theta, TAU, c_tar, c_non, thr)
    assert cnt[2] == 2 and got.tobytes() == clean.tobytes()
    assert np.array_equal(np.delete(cnt, 2), np.delete(clean_cnt, 2))
    # the two rows in the middle (-inf this time): the same sums in another order
    bad_rows[0, 1] = -np.inf
    s3 = np.concatenate([s[:100], bad_rows[:1], s[100:200], bad_rows[1:], s[200:]])
    t3 = np.concatenate([t[:100], [False], t[100:200], [True], t[200:]])
    sd3, td3 = on_device(s3, t3)
    got, cnt = raw_stats(sd3, n + 2, k, td3, theta, TAU, c_tar, c_non, thr)
    want = R.stats(s, t, theta, TAU, c_tar, c_non, thr)
    assert_close(got, want, k, "middle")
    assert_counts(cnt, dict(want, bad=2), 8, "middle")
    assert R.stats(s3, t3, theta, TAU, c_tar, c_non, thr)["bad"] == 2
    # the host raises
    from tf_kaldi_speaker_amd import calibration
    for call in (lambda: calibration.fit(s3, t3, prior=PRIOR), lambda: calibration.cllr(s3[:, 1], t3),
                 lambda: calibration.act_dcf(s3[:, 0], t3, 0.01)):
        with pytest.raises(ValueError):
            call()


def test_stats_are_a_pure_function_of_their_inputs():
    import torch
    k, n = 8, 2 * CHUNK + 77
    s, t = R.fixture(k, n, 31)
    theta = thetas(k)[1]
    c_tar, c_non = R.class_weights(t, PRIOR)
    thr = thresholds(s, theta)
    sd, td = on_device(s, t)
    first = raw_stats(sd, n, k, td, theta, TAU, c_tar, c_non, thr)
    for extra in (0, 0, 1 << 20, 1 << 20, 0):
        again = raw_stats(sd, n, k, td, theta, TAU, c_tar, c_non, thr, extra_ws=extra)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    # what lies behind row n does not matter: more rows, NaN rows, rows of the other class
    rs = np.random.RandomState(1)
    tail = (rs.standard_normal((CHUNK + 5, k)) * 50.0).astype(np.float32)
    tail[::7] = np.nan
    sd2, td2 = on_device(np.concatenate([s, tail]), np.concatenate([t, rs.rand(len(tail)) < 0.5]))
    again = raw_stats(sd2, n, k, td2, theta, TAU, c_tar, c_non, thr)
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ fusion
@pytest.mark.parametrize("k", [1, 3, 8])
def test_fuse_is_bit_identical_to_the_oracle(k):
    from tf_kaldi_speaker_amd import calibration
    for n in (1, 65, 70000):
        s, t = R.fixture(k, max(n, 2), 50 + k)
        s = s[:n]
        rs = np.random.RandomState(n + k)
        for theta in thetas(k) + [rs.standard_normal(k + 1) * 3.0]:
            m = calibration.Model(theta[:k], theta[k])
            want = R.fuse(s, theta)
            assert want.shape == (n,)
            for pad in (0, 3):
                sd, _ = on_device(s, np.zeros(n), pad)
                got = calibration.apply(m, sd)
                assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (k, n, pad)
            assert calibration.apply(m, s if k > 1 else s[:, 0]).tobytes() == want.tobytes()
            assert calibration.apply(m, sd, as_tensor=True).is_cuda


# ------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("k,prior", R.FIT_CASES)
def test_fit_matches_the_oracle_fit(k, prior):
    from tf_kaldi_speaker_amd import calibration
    tol = 1e-14
    s, t, theta_ref, _, lam = R.fit_case(k, prior, calibration.newton)
    assert lam >= 1e-4
    model, report = calibration.fit(s, t, prior=prior, tol=tol)
    theta = model.theta
    dec, H = R.decrement(s, t, prior, theta)
    dist = float(np.linalg.norm(theta - theta_ref))
    print("k %d prior %g: %d steps, oracle decrement %.3g, |theta - oracle| %.3g (bound %.3g)"
          % (k, prior, report.iterations, dec, dist, 2.0 * math.sqrt(4.0 * tol / lam)))
    assert model.prior == prior and 1 <= report.iterations <= 50 and np.isfinite(report.F)
    assert dec <= 4.0 * tol
    assert dist <= 2.0 * math.sqrt(4.0 * tol / lam)
    again, report2 = calibration.fit(s, t, prior=prior, tol=tol)
    assert again.theta.tobytes() == theta.tobytes() and report2 == report


def test_separable_scores_raise_on_the_gpu():
    from tf_kaldi_speaker_amd import calibration
    rs = np.random.RandomState(0)
    t = rs.rand(400) < 0.3
    s = np.where(t, 1.0 + rs.rand(400), -1.0 - rs.rand(400)).astype(np.float32)
    with pytest.raises(RuntimeError):
        calibration.fit(s, t, prior=0.05)


def test_calibration_does_what_it_is_for():
    from tf_kaldi_speaker_amd import calibration, scoring
    n, m, prior = 20000, 8.0, 0.05
    rs = np.random.RandomState(77)
    t = rs.rand(n) < 0.2
    true_llr = np.where(t, m, -m) + math.sqrt(2.0 * m) * rs.standard_normal(n)       # N(+-m, 2m): a well-calibrated llr
    s = (0.3 * true_llr - 2.0).astype(np.float32)
    # the oracle's own fit first
    theta, _ = calibration.newton(R.objective(s, t, prior), 1)
    cal = R.fuse(s, theta)
    assert R.cllr(cal, t) < R.cllr(s, t)
    assert R.act_dcf(cal, t, prior) <= 1.05 * scoring.min_dcf(cal, t, prior)[0]
    # the GPU
    model, _ = calibration.fit(s, t, prior=prior)
    llr = calibration.apply(model, s)
    raw_cllr, cal_cllr = calibration.cllr(s, t), calibration.cllr(llr, t)
    act, mind = calibration.act_dcf(llr, t, prior), scoring.min_dcf(llr, t, prior)[0]
    print("Cllr %.4f -> %.4f, actDCF %.4f, minDCF %.4f" % (raw_cllr, cal_cllr, act, mind))
    assert cal_cllr < raw_cllr
    assert mind <= act <= 1.05 * mind
    # the metrics are the oracle's
    assert abs(raw_cllr - R.cllr(s, t)) <= 1e-12 and abs(cal_cllr - R.cllr(llr, t)) <= 1e-12
    for p, cm, cf in ((prior, 1.0, 1.0), (0.01, 1.0, 1.0), (0.001, 10.0, 1.0), (0.5, 1.0, 2.0)):
        assert calibration.act_dcf(llr, t, p, cm, cf) == R.act_dcf(llr, t, p, cm, cf)
    both = calibration.evaluate(llr, t, [(prior, 1.0, 1.0), (0.01, 1.0, 1.0)])
    assert both[0] == cal_cllr and both[1] == [act, R.act_dcf(llr, t, 0.01)]
    assert abs(calibration.cllr(np.zeros(12, np.float32), np.array([True] * 4 + [False] * 8)) - 1.0) <= 1e-15


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_train_apply_eval(tmp_path, repo_root):
    from tf_kaldi_speaker_amd import calibration, scoring
    n = 600
    s, t = R.fixture(2, n, 61)
    keys = [("spk%03d" % (i % 37), "utt%04d" % i) for i in range(n)]
    text = [["%g" % v for v in s[:, j]] for j in range(2)]
    s = np.array([[float(v) for v in col] for col in text], dtype=np.float32).T      # the scores as the files hold them
    paths = [str(tmp_path / ("scores%d" % j)) for j in range(2)]
    order = [np.arange(n), np.random.RandomState(3).permutation(n)[:-5]]             # file 2: shuffled, five trials short
    for j in range(2):
        with open(paths[j], "w") as f:
            f.write("".join("%s %s %s\n" % (keys[i][0], keys[i][1], text[j][i]) for i in order[j]))
    trials = str(tmp_path / "trials")
    with open(trials, "w") as f:
        f.write("".join("%s %s %s\n" % (keys[i][0], keys[i][1], "target" if t[i] else "nontarget") for i in range(n)))
        f.write("nobody nothing target\n")
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(*args):
        r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.calibrate"] + list(args), env=env, cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return r
    model_path, out = str(tmp_path / "model"), str(tmp_path / "llr")
    r = run("train", "--prior", "0.05", trials, model_path, paths[0], paths[1])
    assert "skipped 6 of 601 trials" in r.stderr
    kept = np.sort(order[1])
    want_model, _ = calibration.fit(s[kept], t[kept], prior=0.05)
    model = calibration.read_model(model_path)
    assert model.theta.tobytes() == want_model.theta.tobytes() and model.prior == 0.05
    r = run("apply", model_path, out, paths[0], paths[1])
    assert "skipped 5 of 600 trials" in r.stderr
    want = ["%s %s %g" % (keys[i][0], keys[i][1], v) for i, v in zip(kept, calibration.apply(model, s[kept]))]
    assert open(out).read().splitlines() == want
    r = run("eval", "--p-target", "0.05", "--p-target", "0.01,10,1", trials, out)
    line = r.stdout.strip().splitlines()[-1]
    mm = re.fullmatch(r"EER: (\S+)% minDCF\(p=0.05\): (\S+) actDCF\(p=0.05\): (\S+) minDCF\(p=0.01,10,1\): (\S+) "
                      r"actDCF\(p=0.01,10,1\): (\S+) Cllr: (\S+)", line)
    assert mm, line
    llr = np.array([float(w.split()[2]) for w in want], dtype=np.float32)
    tk = t[kept]
    expect = [100.0 * scoring.exact_eer(llr, tk), scoring.min_dcf(llr, tk, 0.05)[0], calibration.act_dcf(llr, tk, 0.05),
              scoring.min_dcf(llr, tk, 0.01, 10.0, 1.0)[0], calibration.act_dcf(llr, tk, 0.01, 10.0, 1.0), calibration.cllr(llr, tk)]
    fmts = ["%.4g", "%.4f", "%.4f", "%.4f", "%.4f", "%.4f"]
    assert [mm.group(i + 1) for i in range(6)] == [f % v for f, v in zip(fmts, expect)]
