"""Cosine scoring on the GPU (csrc/score.hip) through the C ABI via tf_kaldi_speaker_amd.scoring, against the float64
oracle tests/helpers/ref_score.py.

The bar for every score of prepared (unit) rows is delta = (d + 8) * 2^-24 absolute: an fp32 dot product of length d
is off by at most d * 2^-24 * sum|a_i b_i| <= d * 2^-24 (Cauchy-Schwarz), plus a few ulps from the two normalisations.
It is derived, not measured.  With a mean and a transform in front no closed bound is offered (cancellation amplifies the
input rounding): there the bar is the larger of delta and 4 x the error a plain float32 numpy evaluation of the same chain
shows against float64 on the same inputs; the test prints both."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_score  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scoring():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import scoring as s
    return s


def _scaled_rows(rng, n, d, lo, hi):
    """N(0,1) rows, each times a random power of two 2^lo..2^hi."""
    return (rng.standard_normal((n, d)) * np.exp2(rng.integers(lo, hi + 1, (n, 1)))).astype(np.float32)


@pytest.mark.parametrize("n,m,d", [(1, 1, 3), (37, 129, 150), (1000, 257, 200), (300, 300, 512), (64, 65, 2048)])
def test_matrix(scoring, n, m, d):
    rng = np.random.default_rng(1000 + n + m + d)
    a, b = _scaled_rows(rng, n, d, -30, 30), _scaled_rows(rng, m, d, -30, 30)
    zero = n // 2
    a[zero] = 0.0
    pa, pb = scoring.prepare(a, as_tensor=True), scoring.prepare(b, as_tensor=True)
    got = scoring.cosine_matrix(pa, pb)
    want = ref_score.cosine_matrix(ref_score.prepare(a), ref_score.prepare(b))
    assert got.shape == (n, m) and got.dtype == np.float32
    err = np.max(np.abs(got - want))
    print("matrix (%d, %d, %d): max |error| %.3e, delta %.3e" % (n, m, d, err, ref_score.delta(d)))
    assert np.all(np.isfinite(got))
    assert err <= ref_score.delta(d)
    assert np.all(got[zero] == 0.0)


def test_pairs(scoring):
    rng = np.random.default_rng(2)
    n, m, d, k = 5000, 4000, 512, 20000
    a, b = _scaled_rows(rng, n, d, -30, 30), _scaled_rows(rng, m, d, -30, 30)
    ia, ib = rng.integers(0, n, k), rng.integers(0, m, k)
    ia[100:200] = ia[0:100]                      # repeats
    ib[100:200] = ib[0:100]
    ib[200:300] = ia[200:300] % m                # i == j
    ia[200:300] = ib[200:300]
    pa, pb = scoring.prepare(a, as_tensor=True), scoring.prepare(b, as_tensor=True)
    got = scoring.cosine_pairs(pa, pb, ia, ib)
    ra, rb = ref_score.prepare(a), ref_score.prepare(b)
    want = np.sum(ra[ia] * rb[ib], axis=1)
    delta = ref_score.delta(d)
    err = np.max(np.abs(got - want))
    mat = scoring.cosine_matrix(pa, pb)[ia, ib]
    print("pairs: max |error| %.3e, vs matrix %.3e, delta %.3e" % (err, np.max(np.abs(got - mat)), delta))
    assert err <= delta
    assert np.max(np.abs(got - mat)) <= 2 * delta
    assert np.array_equal(got[100:200], got[0:100])
    again = scoring.cosine_pairs(pa, pb, ia, ib)
    assert got.tobytes() == again.tobytes()
    from tf_kaldi_speaker_amd import _lib
    with pytest.raises(_lib.XvError) as e:
        scoring.cosine_pairs(pa, pb, [0, n], [0, 0])
    assert e.value.code == _lib.XV_ERR_INVALID
    with pytest.raises(_lib.XvError):
        scoring.cosine_pairs(pa, pb, [0, 1], [-1, 0])


def _f32_chain(x, mean, transform, normalize, eps):
    """The same chain in plain float32 numpy: the stand-in that sets the bar where no closed bound exists."""
    y = np.asarray(x, np.float32)
    if mean is not None:
        y = y - mean.astype(np.float32)[None, :]
    if transform is not None:
        t = transform.astype(np.float32)
        y = y @ t[:, :y.shape[1]].T + (t[:, -1][None, :] if t.shape[1] == y.shape[1] + 1 else np.float32(0))
    if normalize:
        s = np.sum(y * y, axis=1, dtype=np.float32) + np.float32(eps)
        y = y / np.sqrt(np.where(s == 0, np.float32(1), s))[:, None]
    return y.astype(np.float32)


@pytest.mark.parametrize("case", ["mean", "transform", "affine", "mean_affine_raw", "eps0", "eps1e-12", "raw"])
def test_prepare(scoring, case):
    """Normalised cases: rows N(0,1) x 2^-6..2^6; un-normalised cases: N(0,1) rows (the outputs are then of order one, the
    scale at which delta is stated).  Transforms are N(0,1) / sqrt(512)."""
    rng = np.random.default_rng(31)
    n, d, dout = 333, 512, 200
    normalize = case not in ("mean_affine_raw", "raw")
    x = _scaled_rows(rng, n, d, -6, 6) if normalize else rng.standard_normal((n, d)).astype(np.float32)
    x[5] = 0.0
    mean = (0.5 * rng.standard_normal(d)).astype(np.float32) if case in ("mean", "mean_affine_raw") else None
    transform = None
    if case == "transform":
        transform = (rng.standard_normal((dout, d)) / np.sqrt(512)).astype(np.float32)
    if case in ("affine", "mean_affine_raw"):
        transform = (rng.standard_normal((dout, d + 1)) / np.sqrt(512)).astype(np.float32)
    eps = 1e-12 if case == "eps1e-12" else 0.0
    got = scoring.prepare(x, mean=mean, transform=transform, normalize=normalize, eps=eps)
    want = ref_score.prepare(x, mean=mean, transform=transform, normalize=normalize, eps=eps)
    f32_err = np.max(np.abs(_f32_chain(x, mean, transform, normalize, eps) - want))
    err = np.max(np.abs(got - want))
    bar = max(ref_score.delta(d), 4 * f32_err)
    print("prepare %s: GPU max |error| %.3e, float32 numpy %.3e, bar %.3e" % (case, err, f32_err, bar))
    assert got.shape == want.shape and got.dtype == np.float32
    assert err <= bar
    if case in ("eps0", "eps1e-12", "raw"):
        assert np.all(got[5] == 0.0)
    if case == "raw":
        assert np.array_equal(got, x)


def test_prepare_extreme_rows(scoring):
    """Rows at the ends of the fp32 range neither overflow nor flush: the sum of squares is taken of the scaled row."""
    rng = np.random.default_rng(32)
    x = rng.standard_normal((6, 512)).astype(np.float32)
    x[0] *= np.float32(2.0 ** 100)
    x[1] *= np.float32(2.0 ** -100)
    x[3] *= np.float32(2.0 ** 120)
    got = scoring.prepare(x, eps=0.0)
    want = ref_score.prepare(x, eps=0.0)
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got - want)) <= ref_score.delta(512)


def _speaker_data(seed=4, speakers=200, per=10, d=512):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((speakers, d))
    x = np.repeat(cent, per, axis=0) + 4.0 * rng.standard_normal((speakers * per, d))
    x = (x * np.exp2(rng.integers(-6, 7, (speakers * per, 1)))).astype(np.float32)
    labels = np.repeat(np.arange(speakers), per)
    perm = rng.permutation(speakers * per)       # same-label pairs all over the matrix, not only beside the diagonal
    return x[perm], labels[perm]


def _check_bracket(h, oracle_sorted, nbins, delta, what):
    """For every bin edge e_k: #{oracle < e_k - delta} <= C(k) <= #{oracle < e_k + delta}, C = cumulative GPU count."""
    edges = -1.0 + 2.0 * np.arange(nbins + 1) / nbins
    c = np.concatenate([[0], np.cumsum(h.astype(np.int64))])
    lo = np.searchsorted(oracle_sorted, edges - delta, side="left")
    hi = np.searchsorted(oracle_sorted, edges + delta, side="left")
    exact = np.searchsorted(oracle_sorted, edges, side="left")
    print("%s, %d bins: %d scores in a neighbouring bin at the worst edge" % (what, nbins, np.max(np.abs(c - exact))))
    assert np.all(lo <= c) and np.all(c <= hi), what


@pytest.mark.parametrize("nbins", [65536, 256])
def test_histogram_counts_self(scoring, nbins):
    x, labels = _speaker_data()
    d = x.shape[1]
    px = scoring.prepare(x, eps=1e-12, as_tensor=True)
    hs, hd = scoring.score_histograms(px, labels, nbins=nbins)
    assert hs.dtype == np.uint64 and hd.dtype == np.uint64 and hs.shape == (nbins,) and hd.shape == (nbins,)
    assert int(hs.sum()) == 9000 and int(hd.sum()) == 1990000
    r = ref_score.prepare(x, eps=1e-12)
    same, diff = ref_score.self_pairs(ref_score.cosine_matrix(r, r), labels)
    assert same.size == 9000 and diff.size == 1990000
    _check_bracket(hs, np.sort(same), nbins, ref_score.delta(d), "same-label")
    _check_bracket(hd, np.sort(diff), nbins, ref_score.delta(d), "different-label")
    hs2, hd2 = scoring.score_histograms(px, labels, nbins=nbins)
    assert np.array_equal(hs, hs2) and np.array_equal(hd, hd2)


@pytest.mark.parametrize("nbins", [65536, 4096])
def test_histogram_counts_two_sets(scoring, nbins):
    rng = np.random.default_rng(6)
    n, m, d = 700, 1300, 512
    a, b = _scaled_rows(rng, n, d, -6, 6), _scaled_rows(rng, m, d, -6, 6)
    la, lb = rng.integers(0, 50, n), rng.integers(0, 50, m)
    pa, pb = scoring.prepare(a, as_tensor=True), scoring.prepare(b, as_tensor=True)
    hs, hd = scoring.score_histograms(pa, la, pb, lb, nbins=nbins)
    eq = la[:, None] == lb[None, :]
    assert int(hs.sum()) == int(eq.sum()) and int(hd.sum()) == n * m - int(eq.sum())
    s = ref_score.cosine_matrix(ref_score.prepare(a), ref_score.prepare(b))
    _check_bracket(hs, np.sort(s[eq]), nbins, ref_score.delta(d), "same-label")
    _check_bracket(hd, np.sort(s[~eq]), nbins, ref_score.delta(d), "different-label")
    # string labels go through the same path
    hs3, hd3 = scoring.score_histograms(pa, ["s%d" % v for v in la], pb, ["s%d" % v for v in lb], nbins=nbins)
    assert np.array_equal(hs, hs3) and np.array_equal(hd, hd3)


def _check_eer(eer, thr, rates, nbins, delta):
    """min(FRR(thr - w - delta), FAR(thr + w + delta)) <= eer <= max(FRR(thr + w + delta), FAR(thr - w - delta)) with the
    oracle's exact step functions: follows from the count bracket and monotonicity."""
    w = 2.0 / nbins
    lo = min(rates.frr(thr - w - delta), rates.far(thr + w + delta))
    hi = max(rates.frr(thr + w + delta), rates.far(thr - w - delta))
    assert lo <= eer <= hi, (lo, eer, hi)


def test_pairwise_eer(scoring, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    x, labels = _speaker_data()
    d = x.shape[1]
    delta = ref_score.delta(d)
    r = ref_score.prepare(x, eps=1e-12)
    same, diff = ref_score.self_pairs(ref_score.cosine_matrix(r, r), labels)
    exact = ref_score.exact_eer(same, diff)
    print("oracle exact EER %.6f" % exact)
    assert 0.02 <= exact <= 0.4                      # not a degenerate case
    before = x.copy()
    for nbins in (65536, 1024):
        eer, thr = scoring.pairwise_eer(x, labels, nbins=nbins)
        print("pairwise_eer, %d bins: %.6f at %.5f, |eer - exact| %.2e" % (nbins, eer, thr, abs(eer - exact)))
        _check_eer(eer, thr, ref_score.StepRates(same, diff), nbins, delta)
    assert np.array_equal(x, before)                 # the caller's array is not normalised in place
    assert not os.path.exists("test.txt")            # and no stray file in the working directory

    # max_num_embeddings: the reference's stride selection range(0, n, n // max), same condition on that subset
    keep = np.arange(0, x.shape[0], x.shape[0] // 500)
    rs = ref_score.prepare(x[keep], eps=1e-12)
    same_s, diff_s = ref_score.self_pairs(ref_score.cosine_matrix(rs, rs), labels[keep])
    eer, thr = scoring.pairwise_eer(x, labels, max_num_embeddings=500)
    _check_eer(eer, thr, ref_score.StepRates(same_s, diff_s), 65536, delta)
    hs, hd = scoring.score_histograms(scoring.prepare(x[keep], eps=1e-12), labels[keep])
    assert (eer, thr) == scoring.eer_from_histograms(hs, hd)
    assert int(hs.sum()) == same_s.size and int(hd.sum()) == diff_s.size
    assert np.array_equal(x, before)


def test_command_line(scoring, repo_root, tmp_path):
    from tf_kaldi_speaker_amd import kaldi_io, native_ark
    rng = np.random.default_rng(8)
    n, d, dout = 300, 512, 200
    keys = ["utt%04d" % i for i in range(n)]
    x1, x2 = _scaled_rows(rng, n, d, -6, 6), _scaled_rows(rng, n, d, -6, 6)
    # table 2 leans towards the same utterance of table 1, so that target trials score higher
    x2 += x1 * (np.float32(0.08) * np.linalg.norm(x2, axis=1) / np.linalg.norm(x1, axis=1))[:, None].astype(np.float32)
    for name, x in (("a", x1), ("b", x2)):
        w = native_ark.VectorWriter("ark,scp:%s,%s" % (tmp_path / (name + ".ark"), tmp_path / (name + ".scp")))
        w.write(keys, x)
        w.close()
    # 2000 trials, a quarter of them targets (the same utterance on both sides), 7 lines naming a missing key
    t1, t2 = rng.integers(0, n, 2000), rng.integers(0, n, 2000)
    t2[::4] = t1[::4]
    lines = [[keys[i], keys[j], "target" if i == j else "nontarget"] for i, j in zip(t1, t2)]
    missing = (3, 500, 777, 1200, 10, 1500, 1999)
    for pos in missing[:4]:
        lines[pos][0] = "missing%d" % pos
    for pos in missing[4:]:
        lines[pos][1] = "nobody%d" % pos
    (tmp_path / "trials").write_text("".join(" ".join(p) + "\n" for p in lines))
    mean = (np.float32(2.0 ** -8) * rng.standard_normal(d)).astype(np.float32)
    transform = (rng.standard_normal((dout, d + 1)) / np.sqrt(512)).astype(np.float32)
    transform[:, -1] *= np.float32(2.0 ** -8)
    kaldi_io.write_vec_flt(str(tmp_path / "mean.vec"), mean)
    kaldi_io.write_mat(str(tmp_path / "transform.mat"), transform)
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "tf_kaldi_speaker_amd.score_cos", "--gpu", "0"]
    kept = [p for k, p in enumerate(lines) if k not in missing]
    row = {k: i for i, k in enumerate(keys)}
    ia, ib = [row[p[0]] for p in kept], [row[p[1]] for p in kept]
    delta = ref_score.delta(d)

    def run(extra, out):
        r = subprocess.run(base + extra + ["trials", "scp:a.scp", "ark:b.ark", out], env=env, cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [ln.split() for ln in (tmp_path / out).read_text().splitlines()]
        assert len(got) == 1993
        assert [g[:2] for g in got] == [p[:2] for p in kept]              # trial order
        assert "skipped 7 of 2000" in r.stderr
        return np.array([float(g[2]) for g in got]), r

    # plain cosine
    got, _ = run([], "plain.cos")
    want = np.sum(ref_score.prepare(x1)[ia] * ref_score.prepare(x2)[ib], axis=1)
    print("plain: max |error| %.3e" % np.max(np.abs(got - want)))
    assert np.max(np.abs(got - want)) <= delta + 5e-7                     # + the %g rounding
    # mean + affine transform + length norm, with the EER
    got, r = run(["--mean", "mean.vec", "--transform", "transform.mat", "--normalize", "true", "--eer"], "lda.cos")
    o1, o2 = ref_score.prepare(x1, mean, transform), ref_score.prepare(x2, mean, transform)
    want = np.sum(o1[ia] * o2[ib], axis=1)
    f1, f2 = _f32_chain(x1, mean, transform, True, 0.0), _f32_chain(x2, mean, transform, True, 0.0)
    f32_err = np.max(np.abs(np.sum(f1[ia].astype(np.float64) * f2[ib], axis=1) - want))
    print("mean + transform: max |error| %.3e, float32 numpy %.3e" % (np.max(np.abs(got - want)), f32_err))
    assert np.max(np.abs(got - want)) <= max(delta, 4 * f32_err) + 5e-7
    tgt = np.array([p[2] == "target" for p in kept])
    exact = ref_score.exact_eer(got[tgt], got[~tgt])
    print("EER of the printed scores %.6f; the tool printed %r" % (exact, r.stdout.strip()))
    assert r.stdout.strip() == "EER: %.4g%%" % (100.0 * exact)

    # nothing matches: non-zero exit status
    (tmp_path / "none").write_text("x y target\nz w nontarget\n")
    r = subprocess.run(base + ["none", "scp:a.scp", "scp:a.scp", "none.cos"], env=env, cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0
