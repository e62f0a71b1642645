"""GPU: cohort score normalisation (xv_cohort_stats, snorm.py, the --cohort options of score_cos / score_plda).

Two kinds of reference.  (a) The library's own score matrix (xv_score_matrix / xv_plda_matrix): selection then runs on
identical fp32 values and only the rounding of a double result to fp32 separates the two: 2^-22 relative (four fp32 ulps) on
mean and std, absolute 2^-22 * max|s| of the row where |mean| < 2^-10 * max|s|.  So that the relative bound on std means
something the test asserts, on the oracle, std >= 2^-10 * max|s| wherever K_eff >= 2; where K_eff = 1 the definition makes the
std exactly 0 and that is what is asserted instead.  (b) The float64 oracle from float64 scores of unit rows (tests/helpers/
ref_snorm.py): order statistics and the population std of K values are 1-Lipschitz in the sup norm, so the per-score bound
(k + 8) * 2^-24 of csrc/score.hip carries over; a factor 2 covers the final rounding."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi_layouts as L  # noqa: E402
import ref_plda  # noqa: E402
import ref_score  # noqa: E402
import ref_snorm  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 2.0 ** -22
SHAPES = [(1, 1, 3), (130, 257, 37), (5, 5000, 150), (300, 129, 512)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    return _lib.load()


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t)


def raw_stats(lib, a, lda, n, rb, b, ldb, m, cb, k, top_k, la=None, lb=None, ws_bytes=None):
    """xv_cohort_stats on device operands (tensors or raw pointers) -> (mean, std, count) as host arrays."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    need = lib.xv_cohort_stats_workspace(n, m, top_k)
    ws_bytes = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    mean = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    std = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    cnt = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.xv_cohort_stats(0, _ptr(a), lda, n, _ptr(rb), _ptr(la), _ptr(b), ldb, m, _ptr(cb), _ptr(lb), k, top_k,
                                   _ptr(mean), _ptr(std), _ptr(cnt), _ptr(ws), ws_bytes, None))
    torch.cuda.synchronize()
    return mean.cpu().numpy(), std.cpu().numpy(), cnt.cpu().numpy()


def lib_matrix(lib, a, rb, b, cb):
    """The library's own scores of the same operands, as float32 host array."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    (n, k), m = a.shape, b.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=DEV)
    if rb is None and cb is None:
        _lib.check(lib.xv_score_matrix(0, _ptr(a), k, n, _ptr(b), k, m, k, _ptr(out), m, None))
    else:
        _lib.check(lib.xv_plda_matrix(0, _ptr(a), k, n, _ptr(rb), _ptr(b), k, m, _ptr(cb), k, _ptr(out), m, None))
    return out.cpu().numpy()


def check_against_matrix(got, s, top_k, labels=None, cohort_labels=None, what=""):
    """Rule (a) of the module docstring."""
    mean, std, cnt = got
    rm, rs, rc = ref_snorm.cohort_stats(s, top_k, labels, cohort_labels)
    assert np.array_equal(cnt, rc), what
    big = np.max(np.abs(s.astype(np.float64)), axis=1)
    several = rc >= 2
    assert np.all(rs[several] >= 2.0 ** -10 * big[several]), (what, "the oracle's std is too small for a relative bound")
    assert np.all(std[rc == 1] == 0.0), what
    mean_bar = np.where(np.abs(rm) >= 2.0 ** -10 * big, REL * np.abs(rm), REL * big)
    em, es = np.abs(mean - rm), np.abs(std - rs)
    print("%s: max mean error / bar %.3g, max std error / bar %.3g" % (what, np.max(em / mean_bar), np.max(es[several] / (REL * rs[several])) if several.any() else 0.0))
    assert np.all(em <= mean_bar), what
    assert np.all(es[several] <= REL * rs[several]), what


def anchored(rng, n, m, k):
    """Operands whose two largest scores of every row are well apart (the relative std bound needs it for top_k = 2): every
    row of a carries a common component u, cohort row 0 is 2 u and row 1 is u; everything else is noise."""
    u = rng.standard_normal(k)
    u *= 2.0 / np.linalg.norm(u)
    a = (u[None, :] + 0.5 * rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    b = (0.7 * rng.standard_normal((m, k)) / np.sqrt(k)).astype(np.float32)
    b[0] = 2.0 * u
    if m > 1:
        b[1] = u
    return a, b


@pytest.fixture(scope="module")
def cases(lib):
    """Per shape and kind: device operands and the library's own matrix, made once."""
    out = {}
    for n, m, k in SHAPES:
        for kind in ("cosine", "plda"):
            rng = np.random.default_rng(100 * n + m + (7 if kind == "plda" else 0))
            a, b = anchored(rng, n, m, k)
            rb = cb = None
            if kind == "plda":
                rb = _dev((0.25 * rng.standard_normal(n)).astype(np.float32))
                cb = _dev((0.25 * rng.standard_normal(m)).astype(np.float32))
            ad, bd = _dev(a), _dev(b)
            out[(n, m, k, kind)] = (ad, bd, rb, cb, lib_matrix(lib, ad, rb, bd, cb))
    return out


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("kind", ["cosine", "plda"])
@pytest.mark.parametrize("n,m,k", SHAPES)
def test_against_the_library_matrix(lib, cases, n, m, k, kind):
    ad, bd, rb, cb, s = cases[(n, m, k, kind)]
    for top_k in sorted(set(t for t in (0, 1, 2, 7, m - 1, m) if 0 <= t <= m)):
        got = raw_stats(lib, ad, k, n, rb, bd, k, m, cb, k, top_k)
        check_against_matrix(got, s, top_k, what="%s n=%d m=%d k=%d top_k=%d" % (kind, n, m, k, top_k))


def test_rows_longer_than_the_lds_stage(lib):
    """m above 12288: the sweeps read the panel in global memory; with and without exclusion labels."""
    rng = np.random.default_rng(77)
    n, m, k = 3, 12301, 16
    a, b = anchored(rng, n, m, k)
    ad, bd = _dev(a), _dev(b)
    s = lib_matrix(lib, ad, None, bd, None)
    la, lb = np.array([0, 1, 2], np.int32), rng.integers(0, 40, m).astype(np.int32)
    lb[:2] = 99
    for top_k in (0, 7, m - 1):
        check_against_matrix(raw_stats(lib, ad, k, n, None, bd, k, m, None, k, top_k), s, top_k, what="long row top_k=%d" % top_k)
        got = raw_stats(lib, ad, k, n, None, bd, k, m, None, k, top_k, _dev(la), _dev(lb))
        check_against_matrix(got, s, top_k, la, lb, what="long row, labels, top_k=%d" % top_k)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("n,m,d", [(130, 257, 37), (5, 5000, 150)])
def test_end_to_end_cosine_against_float64(lib, n, m, d):
    from tf_kaldi_speaker_amd import scoring, snorm
    rng = np.random.default_rng(n + m)
    x, c = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    xp, cp = scoring.prepare(x, as_tensor=True), scoring.prepare(c, as_tensor=True)
    s64 = ref_score.cosine_matrix(ref_score.prepare(x), ref_score.prepare(c))
    bar = 2 * ref_score.delta(d)
    for top_k in (0, 7, 100):
        got = snorm.cohort_stats(xp, cp, top_k=top_k)
        rm, rs, rc = ref_snorm.cohort_stats(s64, top_k)
        em, es = np.max(np.abs(got.mean - rm)), np.max(np.abs(got.std - rs))
        print("end to end d=%d top_k=%d: mean error %.3e, std error %.3e, bar %.3e" % (d, top_k, em, es, bar))
        assert np.array_equal(got.count, rc) and got.mean.dtype == np.float32 and got.count.dtype == np.int32
        assert em <= bar and es <= bar


# ------------------------------------------------------------------------------------------------ 3
def test_ties(lib):
    """Every cohort row three times, top_k = 100: the boundary falls inside a group of equal scores.  Then 83 times, top_k =
    8299: the same in a row too long for the LDS stage."""
    rng = np.random.default_rng(3)
    n, m1, k = 20, 150, 24
    a, b1 = anchored(rng, n, m1, k)
    b = np.concatenate([b1, b1, b1], axis=0)[rng.permutation(3 * m1)]
    ad, bd = _dev(a), _dev(b)
    s = lib_matrix(lib, ad, None, bd, None)
    check_against_matrix(raw_stats(lib, ad, k, n, None, bd, k, 3 * m1, None, k, 100), s, 100, what="ties")
    check_against_matrix(raw_stats(lib, ad, k, n, None, bd, k, 3 * m1, None, k, 99), s, 99, what="ties, whole groups")
    # the same block 83 times: m = 12450 is above the 12288 scores a workgroup stages in LDS, so the select sweeps the row in
    # global memory.  8299 is no multiple of 83: the boundary falls inside a group of 83 equal scores in every row
    reps = 83
    m = reps * m1
    b = np.tile(b1, (reps, 1))[rng.permutation(m)]
    bd = _dev(b)
    s = lib_matrix(lib, ad, None, bd, None)
    desc = -np.sort(-s, axis=1)
    assert np.array_equal(desc[:, 8298], desc[:, 8299])
    check_against_matrix(raw_stats(lib, ad, k, n, None, bd, k, m, None, k, 8300), s, 8300, what="long ties, whole groups")
    check_against_matrix(raw_stats(lib, ad, k, n, None, bd, k, m, None, k, 8299), s, 8299, what="long ties")


# ------------------------------------------------------------------------------------------------ 4
def test_degenerate_rows(lib):
    rng = np.random.default_rng(4)
    n, m, k = 6, 300, 20
    a = rng.standard_normal((n, k)).astype(np.float32)
    a[2] = 0.0
    b = rng.standard_normal((m, k)).astype(np.float32)
    for top_k in (0, 5):
        mean, std, cnt = raw_stats(lib, _dev(a), k, n, None, _dev(b), k, m, None, k, top_k)
        assert mean[2] == 0.0 and std[2] == 0.0 and np.all(std[[0, 1, 3, 4, 5]] > 0)      # scores +-0: no NaN path
        # a cohort of m copies of one vector: every selected value is the same
        same = np.repeat(b[:1], m, axis=0)
        mean, std, cnt = raw_stats(lib, _dev(a), k, n, None, _dev(same), k, m, None, k, top_k)
        s = lib_matrix(lib, _dev(a), None, _dev(same), None)
        assert np.all(std == 0.0) and np.array_equal(mean, s[:, 0]) and np.all(cnt == (top_k or m))
    # all scores negative: the lower half of the key order.  Row i against -a_j (j != i made positive definite by the shared part)
    u = np.ones(k, np.float32)
    pos = (u[None, :] + 0.1 * rng.standard_normal((40, k))).astype(np.float32)
    ad, bd = _dev(pos), _dev(-pos)
    s = lib_matrix(lib, ad, None, bd, None)
    assert np.all(s < 0)
    for top_k in (0, 3, 39):
        check_against_matrix(raw_stats(lib, ad, k, 40, None, bd, k, 40, None, k, top_k), s, top_k, what="negative top_k=%d" % top_k)


# ------------------------------------------------------------------------------------------------ 5
def test_exclusion(lib):
    from tf_kaldi_speaker_amd import scoring, snorm
    rng = np.random.default_rng(5)
    spk, per, d = 40, 5, 24
    cent = rng.standard_normal((spk, d))
    x = (np.repeat(cent, per, axis=0) + 0.5 * rng.standard_normal((spk * per, d))).astype(np.float32)
    labels = np.repeat(np.array(["spk%02d" % i for i in range(spk)]), per)
    xp = scoring.prepare(x, as_tensor=True)
    m = spk * per
    s = lib_matrix(lib, xp, None, xp, None)
    for top_k in (0, 10, 198):                                     # 198 > the 195 eligible columns: all of them
        got = snorm.cohort_stats(xp, xp, top_k=top_k, labels=labels, cohort_labels=labels)
        assert np.all(got.count == (m - per if top_k in (0, 198) else top_k))
        check_against_matrix(got, s, top_k, labels, labels, what="exclusion top_k=%d" % top_k)
    # without the labels the row itself (cosine 1) leads every top-K list
    assert np.all(snorm.cohort_stats(xp, xp, top_k=10).mean > snorm.cohort_stats(xp, xp, top_k=10, labels=labels, cohort_labels=labels).mean)
    # a label that covers the whole cohort
    got = snorm.cohort_stats(xp[:3], xp[:per], top_k=2, labels=["spk00", "other", "spk00"], cohort_labels=labels[:per])
    assert list(got.count) == [0, 2, 0]
    assert np.isnan(got.mean[0]) and np.isnan(got.std[0]) and np.isnan(got.mean[2]) and np.isfinite(got.mean[1])
    with pytest.raises(ValueError, match="enrolment row 0 "):
        snorm.normalize(np.zeros(1, np.float32), [0], [0], got, got, mode="z")


# ------------------------------------------------------------------------------------------------ 6
def test_panel_loop_and_repeats(lib):
    import torch
    from tf_kaldi_speaker_amd import scoring, snorm
    rng = np.random.default_rng(6)
    n, m, d = 300, 700, 40
    xp = scoring.prepare(rng.standard_normal((n, d)).astype(np.float32), as_tensor=True)
    cp = scoring.prepare(rng.standard_normal((m, d)).astype(np.float32), as_tensor=True)
    least = snorm.workspace_min_bytes(n, m, 50)
    assert least == 128 * 700 * 4
    runs = [snorm.cohort_stats(xp, cp, top_k=50, workspace_bytes=w, as_tensor=True) for w in (least, 64 << 20, least, 64 << 20, None)]
    for r in runs[1:]:
        assert torch.equal(r.mean, runs[0].mean) and torch.equal(r.std, runs[0].std) and torch.equal(r.count, runs[0].count)
    from tf_kaldi_speaker_amd import _lib
    with pytest.raises(_lib.XvError) as e:
        snorm.cohort_stats(xp, cp, top_k=50, workspace_bytes=least - 1)
    assert e.value.code == _lib.XV_ERR_WORKSPACE


# ------------------------------------------------------------------------------------------------ 7
def test_layouts(lib):
    """Padded leading dimensions and base pointers one and three floats past a 16-byte boundary (the loader without vector
    loads): the same bits as the packed call, inputs left as they were."""
    rng = np.random.default_rng(7)
    n, m, k = 131, 70, 37
    a, b = anchored(rng, n, m, k)
    rb, cb = _dev((0.25 * rng.standard_normal(n)).astype(np.float32)), _dev((0.25 * rng.standard_normal(m)).astype(np.float32))
    la, lb = _dev(rng.integers(0, 9, n).astype(np.int32)), _dev(rng.integers(0, 9, m).astype(np.int32))
    for bias in (False, True):
        r, c = (rb, cb) if bias else (None, None)
        want = None
        for pa, pb in L.PAIRS:
            fa, fb = L.place(a, pa, DEV)[0], L.place(b, pb, DEV)[0]
            got = raw_stats(lib, fa.ptr, fa.ld, n, r, fb.ptr, fb.ld, m, c, k, 7, la, lb)
            assert L.intact(fa, a) and L.intact(fb, b), (pa, pb)
            assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])), (pa, pb)       # a NaN: padding reached a score
            if want is None:
                want = got
            for g, w in zip(got, want):
                assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (bias, pa, pb)


# ------------------------------------------------------------------------------------------------ 8
@pytest.fixture(scope="module")
def plda_case(lib):
    from tf_kaldi_speaker_amd import plda
    rng = np.random.default_rng(8)
    d = 24
    pm, ptm, psi = ref_plda.random_model(rng, d)
    model = plda.Plda(0.02 * pm, ptm * np.sqrt(d), psi)
    draw = lambda spk, per: ref_plda.draw(rng, model.mean, model.transform, model.psi, spk, per, 1.0)[0].astype(np.float32)  # noqa: E731
    return model, draw(30, 1), draw(45, 1), draw(20, 7)           # enrolment, test, cohort rows


def test_plda_orientation(lib, plda_case):
    """per="test" against the float64 statistics of the *columns* of llr_matrix(prepare_enroll(cohort), test), transposed on the
    host.  The swapped call adds the biases as (a . b + tau_j) + rho_i, the matrix as (a . b + rho_i) + tau_j: each is within
    2^-24 * (|a . b| + |rho| + |tau|) per rounding of the exact sum, so two entries differ by at most 4 * 2^-24 * M with
    M = max(|a . b| + |rho| + |tau|); statistics are 1-Lipschitz in the sup norm, and 2^-22 * max|s| covers the final rounding.
    per="enroll" takes the matrix's own bits and is held to rule (a)."""
    from tf_kaldi_speaker_amd import plda, snorm
    model, xe, xt, xc = plda_case
    enroll, test = plda.prepare_enroll(model, xe), plda.prepare_test(model, xt)
    ce, ct = plda.prepare_enroll(model, xc), plda.prepare_test(model, xc)
    s_e = plda.llr_matrix(enroll, ct)
    s_t = plda.llr_matrix(ce, test)
    k = ce.k
    dot = np.abs(ce.packed.cpu().numpy()[:, :k].astype(np.float64) @ test.packed.cpu().numpy()[:, :k].astype(np.float64).T)
    big = np.max(dot + np.abs(ce.bias.cpu().numpy().astype(np.float64))[:, None]
                 + np.abs(test.tau(ce.uniform_n).cpu().numpy().astype(np.float64))[None, :])
    bar = 4 * 2.0 ** -24 * big + REL * np.max(np.abs(s_t))
    for top_k in (0, 5, 30):
        ze = snorm.plda_cohort_stats(enroll, ct, per="enroll", top_k=top_k)
        check_against_matrix(ze, s_e, top_k, what="plda per=enroll top_k=%d" % top_k)
        zt = snorm.plda_cohort_stats(ce, test, per="test", top_k=top_k)
        rm, rs, rc = ref_snorm.cohort_stats(s_t.T, top_k)
        assert zt.mean.shape == (len(test),) and np.array_equal(zt.count, rc)
        em, es = np.max(np.abs(zt.mean - rm)), np.max(np.abs(zt.std - rs))
        print("plda per=test top_k=%d: mean error %.3e, std error %.3e, bar %.3e" % (top_k, em, es, bar))
        assert em <= bar and es <= bar
    # the orientation matters: the statistics of the rows of the same matrix are something else
    assert not np.allclose(ref_snorm.cohort_stats(s_t.T, 5)[0][:20], ref_snorm.cohort_stats(s_t, 5)[0][:20])


# ------------------------------------------------------------------------------------------------ 9
def test_command_line(lib, plda_case, repo_root, tmp_path):
    """--cohort --norm s --top-k 5, cosine and PLDA, each one run in a child process: the scores written equal snorm.normalize of
    the unnormalised scores (the calls the tool makes without --cohort), printed as the tool prints them, to 1e-6."""
    from tf_kaldi_speaker_amd import native_ark, plda, scoring, snorm
    model, xe, xt, xc = plda_case
    plda.write_plda(str(tmp_path / "plda"), model)
    tables = {"enroll": (["spk%02d" % i for i in range(len(xe))], xe), "test": (["utt%02d" % i for i in range(len(xt))], xt),
              "cohort": (["coh%03d" % i for i in range(len(xc))], xc)}
    for name, (keys, x) in tables.items():
        w = native_ark.VectorWriter("ark:%s" % (tmp_path / (name + ".ark")))
        w.write(keys, x)
        w.close()
    rng = np.random.default_rng(9)
    ia, ib = rng.integers(0, len(xe), 200), rng.integers(0, len(xt), 200)
    tgt = (ia + ib) % 5 == 0
    (tmp_path / "trials").write_text("".join("%s %s %s\n" % (tables["enroll"][0][i], tables["test"][0][j], "target" if t else "nontarget")
                                             for i, j, t in zip(ia, ib, tgt)))
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(tool, out):
        pos = (["trials", "ark:enroll.ark", "ark:test.ark"] if tool == "score_cos" else ["plda", "ark:enroll.ark", "ark:test.ark", "trials"])
        r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd." + tool, "--gpu", "0", "--eer", "--cohort", "ark:cohort.ark",
                            "--norm", "s", "--top-k", "5"] + pos + [out], env=env, cwd=str(tmp_path), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return np.array([float(ln.split()[2]) for ln in (tmp_path / out).read_text().splitlines()]), r.stdout

    def check(tool, got, stdout, plain, ze, zt):
        want = np.array([float("%g" % v) for v in snorm.normalize(plain, ia, ib, ze, zt, mode="s")])
        print("%s: normalised scores %.3f..%.3f, max difference %.3e" % (tool, want.min(), want.max(), np.max(np.abs(got - want))))
        assert got.shape == want.shape and np.all(np.abs(got - want) <= 1e-6)
        assert np.max(np.abs(want - np.array([float("%g" % v) for v in plain]))) > 0.1        # the run did normalise
        assert stdout.strip() == "EER: %.4g%%" % (100.0 * scoring.exact_eer(got, tgt))

    pe, pt, pc = (scoring.prepare(x, as_tensor=True) for x in (xe, xt, xc))
    got, stdout = run("score_cos", "cos.snorm")
    check("score_cos", got, stdout, scoring.cosine_pairs(pe, pt, ia, ib), snorm.cohort_stats(pe, pc, top_k=5),
          snorm.cohort_stats(pt, pc, top_k=5))
    got, stdout = run("score_plda", "plda.snorm")
    enroll, test = plda.prepare_enroll(model, pe), plda.prepare_test(model, pt)
    check("score_plda", got, stdout, plda.llr_pairs(enroll, test, ia, ib),
          snorm.plda_cohort_stats(enroll, plda.prepare_test(model, pc), per="enroll", top_k=5),
          snorm.plda_cohort_stats(plda.prepare_enroll(model, pc), test, per="test", top_k=5))
