"""Back-end training statistics on the GPU (csrc/backend.hip) through the C ABI, and the three commands end to end.

The bar of one entry of G = sum_r w_r (x_r - c)(x_r - c)^T.  With y = x - c evaluated in float64 from the same fp32 rows the
oracle is G_ref = (y w)^T y in float64, and

    |G - G_ref|_ij <= (n + 16) 2^-53 sum_r |w_r y_ri y_rj|

 * the kernel's y is the same float64 subtraction (one rounding, shared with the oracle);
 * y w is one rounding, the product with the other operand and the add are one fused rounding per term: a chain of n double
   adds in a fixed order (per slice, then over the slices), at most n 2^-53 sum|.| to first order;
 * the 16 covers the weighting, and the oracle's own (blocked, pairwise) summation, which is no worse than the chain's.
Derived, not measured; every test prints the measured maximum beside it."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_backend  # noqa: E402
import ref_plda  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# End to end (test_commands_end_to_end): the largest |score - oracle score| / max |oracle score| over the 6400 trials.  The
# difference comes from the float32 files (mean.vec, transform.mat), the float32 front of the commands and the %g of the score
# file; it was measured with exactly those steps in float32 and the rest in float64 on the host, on the inputs of the test:
# 1.07e-6 (scores -496..14, EER 1.25 % on both sides).  The fp32 scoring kernels add at most their own bar on top
# ((K + 8) 2^-24 sum |a b| + 4 * 2^-24 (|rho| + |tau| + |s|), tests/test_gpu_plda.py: below 3e-6 of the largest score here).
# The bar is 100 x the measured value (profiles/backend.md); the test prints what the device gives.
E2E_MEASURED = 1.1e-6
E2E_BAR = 100.0 * E2E_MEASURED


class Dev(object):
    def __init__(self):
        import __graft_entry__ as g
        g.build()
        import torch
        from tf_kaldi_speaker_amd import _lib, backend
        self.torch, self._lib, self.backend, self.lib = torch, _lib, backend, _lib.load()

    def put(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def gram(self, x, d, c=None, w=None, ws_bytes=None, rows64=False):
        """x [n, ld] (float32, or float64 with rows64) -> (return code, G [d, d] float64)."""
        import ctypes as C
        n, ld = x.shape
        xd, cd, wd = self.put(x), self.put(c), self.put(w)
        need = self.lib.xv_gram_f64_workspace(n, d)
        have = need if ws_bytes is None else ws_bytes
        ws = self.torch.empty((max(have, 8) // 8 + 1,), dtype=self.torch.float64, device="cuda:0")
        g = self.torch.full((max(d, 1), max(d, 1)), np.nan, dtype=self.torch.float64, device="cuda:0")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
        fn = self.lib.xv_gram_f64_rows64 if rows64 else self.lib.xv_gram_f64
        rc = fn(0, p(xd), ld, n, d, p(cd), p(wd), p(g), p(ws), have, None)
        self.torch.cuda.synchronize()
        return rc, g.cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    return Dev()


def _oracle(x, d, c, w):
    y = x[:, :d].astype(np.float64) - (0.0 if c is None else c[None, :])
    yw = y if w is None else y * w[:, None]
    n = x.shape[0]
    return yw.T @ y, (n + 16) * U * (np.abs(yw).T @ np.abs(y))


@pytest.mark.parametrize("n", [0, 1, 5, 1000, 20011])
@pytest.mark.parametrize("d", [1, 3, 17, 150, 512])
def test_gram(dev, d, n):
    """Plain, centred + weighted, and centred + weighted with a leading dimension d + 5, each against the bar of the module
    docstring; G == G^T bitwise; a second call is bit-identical; n = 0 writes zeros."""
    rng = np.random.default_rng(100 * d + n % 97)
    ld = d + 5
    x = (rng.standard_normal((n, ld)) * np.exp2(rng.integers(-3, 4, (1, ld))) + 0.5).astype(np.float32)
    c = rng.standard_normal(d) * 0.3 + 0.5
    w = rng.uniform(0.5, 3.0, n)
    for name, xs, cc, ww in [("plain", np.ascontiguousarray(x[:, :d]), None, None),
                             ("c+w", np.ascontiguousarray(x[:, :d]), c, w), ("c+w ld", x, c, w),
                             ("c", np.ascontiguousarray(x[:, :d]), c, None), ("w", np.ascontiguousarray(x[:, :d]), None, w)]:
        rc, g = dev.gram(xs, d, cc, ww)
        assert rc == 0
        want, bar = _oracle(xs, d, cc, ww)
        err = np.abs(g - want)
        ratio = float(np.max(err / np.where(bar > 0, bar, 1.0))) if n else 0.0
        print("gram d %d n %d %s: max |error| %.3e, max error / bar %.3f" % (d, n, name, err.max(), ratio))
        assert np.all(np.isfinite(g)) and np.all(err <= bar)
        assert np.array_equal(g, g.T)
        if n == 0:
            assert np.all(g == 0.0)
        rc2, g2 = dev.gram(xs, d, cc, ww)
        assert rc2 == 0 and g2.tobytes() == g.tobytes()


def test_gram_layout_probe(dev):
    """Rows with one or two non-zero integer entries at known positions and distinct integer weights: every product and sum
    is an integer below 2^53, so G must equal the expected integer matrix exactly.  The positions of a two-entry row lie in
    different 64-column blocks at different offsets, so a transposed or permuted MFMA lane mapping, a wrong tile or a wrong
    mirror puts a value where another belongs."""
    rng = np.random.default_rng(7)
    d, n = 150, 1500
    x = np.zeros((n, d), np.float32)
    a = rng.integers(0, d, n)
    b = (a + rng.integers(1, d, n)) % d                     # b != a
    va, vb = rng.integers(1, 8, n), rng.integers(1, 8, n)
    two = rng.random(n) < 0.8
    x[np.arange(n), a] = va
    x[np.arange(n)[two], b[two]] = vb[two]
    w = np.arange(1, n + 1, dtype=np.float64)
    want = np.zeros((d, d), np.int64)
    for r in range(n):
        want[a[r], a[r]] += (r + 1) * va[r] * va[r]
        if two[r]:
            want[b[r], b[r]] += (r + 1) * vb[r] * vb[r]
            want[a[r], b[r]] += (r + 1) * va[r] * vb[r]
            want[b[r], a[r]] += (r + 1) * va[r] * vb[r]
    rc, g = dev.gram(x, d, None, w)
    assert rc == 0
    wrong = np.argwhere(g != want.astype(np.float64))
    print("layout probe: %d of %d entries differ%s" % (len(wrong), d * d, "" if not len(wrong) else ", first at %s" % (wrong[0],)))
    assert len(wrong) == 0
    # the same with an integer centre: (x - c) stays an integer
    c = rng.integers(-3, 4, d).astype(np.float64)
    rc, g = dev.gram(x, d, c, w)
    y = x.astype(np.float64) - c[None, :]
    assert rc == 0 and np.array_equal(g, (y * w[:, None]).T @ y)


@pytest.mark.parametrize("e", [40, -40, 60, -60])
def test_gram_magnitude(dev, e):
    """Rows scaled by 2^e: the squares reach 2^+-120, outside what an fp32 product or sum holds; the double path keeps the bar
    (which scales with the data) and stays finite and non-zero."""
    rng = np.random.default_rng(100 + e)
    n, d = 777, 70
    x = np.ldexp(rng.standard_normal((n, d)), e).astype(np.float32)
    w = rng.uniform(0.5, 2.0, n)
    rc, g = dev.gram(x, d, None, w)
    want, bar = _oracle(x, d, None, w)
    err = np.abs(g - want)
    print("gram 2^%d: diagonal %.3e..%.3e, max error / bar %.3f" % (e, np.diag(g).min(), np.diag(g).max(), np.max(err / bar)))
    assert rc == 0 and np.all(np.isfinite(g)) and np.all(np.diag(g) > 0.0) and np.all(err <= bar)


def test_gram_double_rows(dev):
    """The double-row form (the between-class scatter over class means): same bar, no fp32 rounding of the rows."""
    rng = np.random.default_rng(3)
    n, d = 301, 70
    x = rng.standard_normal((n, d)) + 1.0 / 3.0
    w = rng.integers(1, 10, n).astype(np.float64)
    rc, g = dev.gram(x, d, None, w, rows64=True)
    want = (x * w[:, None]).T @ x
    bar = (n + 16) * U * (np.abs(x * w[:, None]).T @ np.abs(x))
    print("gram of double rows: max error / bar %.3f" % np.max(np.abs(g - want) / bar))
    assert rc == 0 and np.all(np.abs(g - want) <= bar) and np.array_equal(g, g.T)


def test_gram_errors(dev):
    x = np.ones((40, 8), np.float32)
    L = dev._lib
    assert dev.gram(np.ones((40, 1), np.float32), 0)[0] == L.XV_ERR_UNSUPPORTED
    assert dev.gram(np.ones((3, 2049), np.float32), 2049)[0] == L.XV_ERR_UNSUPPORTED
    assert dev.lib.xv_gram_f64_workspace(10, 0) == L.XV_ERR_UNSUPPORTED
    assert dev.lib.xv_gram_f64_workspace(10, 2049) == L.XV_ERR_UNSUPPORTED
    need = dev.lib.xv_gram_f64_workspace(40, 8)
    assert need > 0 and dev.lib.xv_gram_f64_workspace(0, 8) == 0
    rc, g = dev.gram(x, 8, ws_bytes=need - 8)
    assert rc == L.XV_ERR_WORKSPACE and np.all(np.isnan(g))           # refused before anything was written
    rc, g = dev.gram(x, 8)
    assert rc == 0 and np.all(g == 40.0)
    rc, g = dev.gram(np.ones((3, 2048), np.float32), 2048)            # the largest d
    assert rc == 0 and np.all(g == 3.0)


def test_class_mean(dev):
    """Against float64 means at (n_s + 2) 2^-53 sum |x| (with c: one more rounding, 2^-53 (|mean| + |c|) at most): a class
    of one, an empty class in the middle and an empty tail, rows in shuffled order, a leading dimension."""
    import ctypes as C
    rng = np.random.default_rng(9)
    n, d, ld = 300, 17, 20
    x = (rng.standard_normal((n, ld)) * 4.0 + 1.0).astype(np.float32)
    sizes = [1, 7, 0, 33, 64, 150, 2, 0, 0]
    index = rng.permutation(n)[:sum(sizes)].astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    c = rng.standard_normal(d)
    xd, offd, idxd, cd = dev.put(x), dev.put(off), dev.put(index), dev.put(c)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    for cc, ccd in [(None, None), (c, cd)]:
        out = dev.torch.full((len(sizes), d + 3), -7.0, dtype=dev.torch.float64, device="cuda:0")
        rc = dev.lib.xv_class_mean_f64(0, p(xd), ld, n, d, p(offd), p(idxd), len(sizes), p(ccd), p(out), d + 3, None)
        dev.torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert rc == 0 and np.all(got[:, d:] == -7.0)
        worst = 0.0
        for s, k in enumerate(sizes):
            rows = x[index[off[s]:off[s + 1]], :d].astype(np.float64)
            if k == 0:
                assert np.all(got[s, :d] == 0.0)
                continue
            want = rows.sum(axis=0) / k - (0.0 if cc is None else cc)
            bar = (k + 2) * U * np.abs(rows).sum(axis=0)
            if cc is not None:
                bar = bar + U * (np.abs(rows.sum(axis=0) / k) + np.abs(cc))
            worst = max(worst, float(np.max(np.abs(got[s, :d] - want) / bar)))
            assert np.all(np.abs(got[s, :d] - want) <= bar)
            if k == 1 and cc is None:
                assert np.array_equal(got[s, :d], rows[0])
        print("class means (%s): max error / bar %.3f" % ("plain" if cc is None else "minus c", worst))


def _stats_bars(x, labels, st):
    """(bar of total, bar of between) for scatter_stats of float64 rows x with class ids `labels`; see test_scatter_stats."""
    n, s = x.shape[0], st.num_classes
    ids = np.unique(labels)
    y = np.abs(x - st.center)
    m = np.abs(np.stack([x[labels == k].mean(axis=0) for k in ids]) - st.center)
    delta = (st.counts[:, None] + 3) * U * np.stack([np.abs(x[labels == k]).mean(axis=0) for k in ids])
    mw = m * st.counts[:, None]
    return (n + 16) * U * (y.T @ y), (s + 16) * U * (mw.T @ m) + (delta * st.counts[:, None]).T @ m + mw.T @ delta


def test_scatter_stats(dev):
    """backend.scatter_stats against numpy float64 (tests/helpers/ref_backend.numpy_stats about the same centre): the total
    scatter at the bar of the module docstring; the between-class scatter at that bar over the class means plus what the
    error of a class mean, delta <= (n_s + 3) 2^-53 mean|x| (the bar of test_class_mean and the host's subtraction of the
    centre), moves it by: n_s (delta_i |m_j - c_j| + |m_i - c_i| delta_j)."""
    rng = np.random.default_rng(21)
    d = 24
    mean, transform, psi = ref_plda.random_model(rng, d)
    x, labels = ref_plda.draw(rng, mean, transform, psi, 50, 5)
    keep = rng.permutation(x.shape[0])[:211]
    x, labels = x[keep].astype(np.float32), labels[keep]
    x64 = x.astype(np.float64)
    cases = [("about the mean", x64, labels, labels, None), ("about 0", x64, labels, labels, np.zeros(d))]
    # (offsets, index): rows outside every class do not count, a row listed twice counts twice
    off, idx = np.array([0, 3, 3, 8]), np.array([5, 1, 9, 2, 2, 7, 30, 4])
    cases.append(("offsets + index", x64[idx], np.array([0, 0, 0, 1, 1, 1, 1, 1]), (off, idx), None))
    for name, rows, ids, class_index, centre in cases:
        st = dev.backend.scatter_stats(x, class_index, center=centre)
        ref = ref_backend.numpy_stats(rows, ids, st.center)
        assert st.n == rows.shape[0] and np.array_equal(st.counts, ref["counts"])
        sums = np.stack([np.abs(rows[ids == k]).sum(axis=0) for k in np.unique(ids)])
        assert np.all(np.abs(st.means - ref["means"]) <= (st.counts[:, None] + 2) * U * sums)
        assert np.all(np.abs(st.mean - ref["mean"]) <= (st.n + 2) * U * np.abs(rows).sum(axis=0) / st.n + 2 * U * np.abs(ref["mean"]))
        bar_t, bar_b = _stats_bars(rows, ids, st)
        et, eb = np.abs(st.total - ref["total"]), np.abs(st.between - ref["between"])
        print("scatter_stats (%s): total error / bar %.3f, between error / bar %.3f" % (name, np.max(et / bar_t), np.max(eb / bar_b)))
        assert np.all(et <= bar_t) and np.all(eb <= bar_b)


def _write_ark(path, keys, x):
    from tf_kaldi_speaker_amd import kaldi_io
    with open(path, "wb") as f:
        for k, v in zip(keys, x):
            kaldi_io.write_vec_flt(f, np.ascontiguousarray(v, dtype=np.float32), key=k)


def _run(module, *args):
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd." + module] + list(args), cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert r.returncode == 0, "%s failed:\n%s" % (module, r.stderr[-2000:])
    return r


def test_commands_end_to_end(dev, tmp_path):
    """compute_mean -> compute_lda --dim 16 -> compute_plda as child processes on ark files, scored with score_plda, against
    the same chain in float64 (ref_backend + ref_plda).  Scores within E2E_BAR of the oracle relative to the largest score;
    the EER over the held-out trials identical; the files readable by plda.read_plda and score_cos --mean --transform.
    How the bar was measured: see E2E_MEASURED."""
    from tf_kaldi_speaker_amd import kaldi_io, plda, scoring
    rng = np.random.default_rng(2024)
    d, dim = 24, 16
    model = ref_plda.random_model(rng, d)
    xtr, ltr = ref_plda.draw(rng, *model, 200, 6)
    # enrolment (40 x 3) and test (40 x 4) share their held-out speakers: one draw of 40 x 7, split
    xho, _ = ref_plda.draw(rng, *model, 40, 7)
    ho = xho.reshape(40, 7, d)
    xen, xte, lte = ho[:, :3].astype(np.float32), ho[:, 3:].reshape(160, d).astype(np.float32), np.repeat(np.arange(40), 4)
    xtr = xtr.astype(np.float32)
    spk_en = xen.astype(np.float64).mean(axis=1).astype(np.float32)            # speaker means of three utterances

    t = str(tmp_path)
    ktr = ["s%03d-u%d" % (s, i) for s in range(200) for i in range(6)]
    _write_ark(t + "/train.ark", ktr, xtr)
    _write_ark(t + "/enroll.ark", ["e%02d" % s for s in range(40)], spk_en)
    _write_ark(t + "/test.ark", ["t%02d-%d" % (s, i) for s in range(40) for i in range(4)], xte)
    with open(t + "/utt2spk", "w") as f:
        f.write("".join("%s s%03d\n" % (k, int(k[1:4])) for k in ktr))
    with open(t + "/spk2utt", "w") as f:
        for s in range(200):
            extra = " s%03d-absent" % s if s == 5 else ""                        # an utterance without a vector: skipped
            f.write("s%03d %s%s\n" % (s, " ".join("s%03d-u%d" % (s, i) for i in range(6)), extra))
        f.write("s999 s999-u0 s999-u1\n")                                        # a speaker without any: left out
    with open(t + "/num_utts.ark", "w") as f:
        f.write("".join("e%02d 3\n" % s for s in range(40)))
    targets = []
    with open(t + "/trials", "w") as f:
        for s in range(40):
            for j in range(160):
                targets.append(lte[j] == s)
                f.write("e%02d t%02d-%d %s\n" % (s, lte[j], j % 4, "target" if lte[j] == s else "nontarget"))
    targets = np.array(targets)

    _run("compute_mean", "ark:" + t + "/train.ark", t + "/mean.vec")
    _run("compute_lda", "--dim", str(dim), "--mean", t + "/mean.vec", "ark:" + t + "/train.ark", "ark:" + t + "/utt2spk", t + "/transform.mat")
    r = _run("compute_plda", "--mean", t + "/mean.vec", "--transform", t + "/transform.mat", "--normalize-length",
             "ark:" + t + "/spk2utt", "ark:" + t + "/train.ark", t + "/plda")
    assert "skipped 3 of 1203" in r.stderr
    _run("score_plda", "--mean", t + "/mean.vec", "--transform", t + "/transform.mat", "--num-utts", "ark:" + t + "/num_utts.ark",
         t + "/plda", "ark:" + t + "/enroll.ark", "ark:" + t + "/test.ark", t + "/trials", t + "/scores")
    got = np.array([float(line.split()[2]) for line in open(t + "/scores")])
    assert got.shape == (6400,)

    # the files
    mean_f = kaldi_io.read_vec_flt(t + "/mean.vec")
    lda_f = kaldi_io.read_mat(t + "/transform.mat")
    plda_f = plda.read_plda(t + "/plda")
    assert mean_f.shape == (d,) and lda_f.shape == (dim, d + 1) and lda_f.dtype == np.float32 and plda_f.dim == dim
    assert scoring.check_transform(d, lda_f.shape) == (dim, d + 1)
    assert np.all(plda_f.psi >= 0.0) and np.all(np.diff(plda_f.psi) <= 0.0)

    # the oracle: the same chain in float64 from the same float32 x-vectors
    x64 = xtr.astype(np.float64)
    mean = x64.mean(axis=0)
    lda = ref_backend.lda(x64 - mean, ltr, dim)

    def front(x, scale):
        y = (x.astype(np.float64) - mean) @ lda[:, :d].T + lda[:, d]
        return y / np.linalg.norm(y, axis=1, keepdims=True) * scale
    pm = ref_backend.plda(front(xtr, np.sqrt(dim)), ltr, 10)
    e = ref_plda.transform_ivector(pm["mean"], pm["transform"], pm["psi"], front(spk_en, 1.0), n=3)
    tt = ref_plda.transform_ivector(pm["mean"], pm["transform"], pm["psi"], front(xte, 1.0), n=1)
    want = ref_plda.llr(pm["psi"], e, 3, tt).reshape(-1)

    diff = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    eer_got, eer_want = scoring.exact_eer(got, targets), scoring.exact_eer(want, targets)
    print("end to end: scores %.2f..%.2f, max |difference| / max |score| %.3e (bar %.1e); EER %.4f%% vs %.4f%%; psi rel %.3e"
          % (want.min(), want.max(), diff, E2E_BAR, 100 * eer_got, 100 * eer_want,
             np.max(np.abs(plda_f.psi - pm["psi"])) / pm["psi"].max()))
    assert diff <= E2E_BAR
    assert eer_got == eer_want and 0.0 < eer_want < 0.5

    # the same files through score_cos --mean --transform
    _run("score_cos", "--mean", t + "/mean.vec", "--transform", t + "/transform.mat", t + "/trials", "ark:" + t + "/enroll.ark",
         "ark:" + t + "/test.ark", t + "/scores.cos")
    cos = np.array([float(line.split()[2]) for line in open(t + "/scores.cos")])
    a, b = front(spk_en, 1.0), front(xte, 1.0)
    assert cos.shape == (6400,) and np.max(np.abs(cos - (a @ b.T).reshape(-1))) <= 1e-4
