"""GPU: identification (xv_score_topk, scoring.top_k, plda.llr_top_k, the identify tool).

Every comparison is exact, bit for bit.  The expected result is built from what the library had before this call existed: the
matrix xv_score_matrix / xv_plda_matrix writes for the same operands in the same order, copied to the host and pushed through
the numpy statement of the rule (tests/helpers/ref_topk.py).  Output buffers are pre-filled with a canary and given a leading
dimension of top_k + 3, so a store past column top_k - 1 shows up."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi_layouts as L  # noqa: E402
import ref_plda  # noqa: E402
import ref_topk  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_F, CANARY_I = 0x7FC5A5A5, 0x5A5A5A5A
# (n, m, k): both sides of the 128-row and the 128-column tile edge, one and several tiles, one and several K steps
SHAPES = [(1, 1, 1), (129, 5, 7), (300, 127, 200), (129, 128, 512), (128, 129, 7), (1, 129, 200), (129, 1000, 200), (300, 4099, 7)]


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


def top_ks(m):
    return sorted(set(t for t in (1, 2, 64, 1000, 1024, m + 3) if t <= 1024))


def raw_topk(lib, a, lda, n, rb, b, ldb, m, cb, k, top_k, la=None, lb=None, ws_bytes=None, ldo=None, expect=0, count=True, ws_shift=0):
    """xv_score_topk on device operands (tensors or raw pointers) -> (scores [n, ldo] as uint32 bits, index [n, ldo], count)."""
    import torch
    need = max(int(lib.xv_score_topk_workspace(n, m, min(max(top_k, 1), 1024))), 0)
    ws_bytes = need if ws_bytes is None else ws_bytes
    ldo = top_k + 3 if ldo is None else ldo
    ws = torch.empty(max(ws_bytes, 1) + ws_shift, dtype=torch.uint8, device=DEV)[ws_shift:]       # ws_shift: bytes off alignment
    rows = max(n, 1)                                                # n = 0 still gets buffers that could be written
    sc = torch.full((rows, max(ldo, 1)), CANARY_F, dtype=torch.int32, device=DEV)
    ix = torch.full((rows, max(ldo, 1)), CANARY_I, dtype=torch.int32, device=DEV)
    cnt = torch.full((rows,), CANARY_I, dtype=torch.int32, device=DEV)
    rc = lib.xv_score_topk(0, _ptr(a), lda, n, _ptr(rb), _ptr(la), _ptr(b), ldb, m, _ptr(cb), _ptr(lb), k, top_k, _ptr(sc), _ptr(ix),
                           ldo, _ptr(cnt) if count else None, _ptr(ws), ws_bytes, None)
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.xv_last_error(None))
    return sc.cpu().numpy().view(np.uint32), ix.cpu().numpy(), cnt.cpu().numpy()


def untouched(got):
    return bool(np.all(got[0] == CANARY_F) and np.all(got[1] == CANARY_I) and np.all(got[2] == CANARY_I))


def lib_matrix(lib, a, rb, b, cb):
    """The library's own scores of the same operands in the same order, as float32 host array."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    (n, k), m = a.shape, b.shape[0]
    out = torch.empty((n, max(m, 1)), dtype=torch.float32, device=DEV)
    if rb is None and cb is None:
        _lib.check(lib.xv_score_matrix(0, _ptr(a), k, n, _ptr(b), k, m, k, _ptr(out), max(m, 1), None))
    else:
        _lib.check(lib.xv_plda_matrix(0, _ptr(a), k, n, _ptr(rb), _ptr(b), k, m, _ptr(cb), k, _ptr(out), max(m, 1), None))
    return out.cpu().numpy()[:, :m]


def check(got, s, top_k, la=None, lb=None, what="", count=True):
    """Bit for bit against the rule over the host matrix `s`; everything from column top_k on is still the canary."""
    sc, ix, cnt = got
    ws, wi, wc = ref_topk.top_k(s, top_k, la, lb)
    assert np.array_equal(cnt, wc) if count else np.all(cnt == CANARY_I), what
    assert np.array_equal(ix[:, :top_k], wi), what
    assert np.array_equal(sc[:, :top_k], ws.view(np.uint32)), what
    assert np.all(sc[:, top_k:] == CANARY_F) and np.all(ix[:, top_k:] == CANARY_I), (what, "a store past column top_k - 1")
    pad = np.arange(top_k)[None, :] >= wc[:, None]
    assert np.all(ix[:, :top_k][pad] == -1) and np.all(sc[:, :top_k][pad] == 0xFF800000), what


@pytest.fixture(scope="module")
def cases(lib):
    """Per shape and kind: device operands and the library's own matrix, made once."""
    out = {}
    for n, m, k in SHAPES:
        for kind in ("cosine", "plda"):
            rng = np.random.default_rng(100 * n + m + (7 if kind == "plda" else 0))
            a = rng.standard_normal((n, k)).astype(np.float32)
            b = rng.standard_normal((m, k)).astype(np.float32)
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
    for top_k in top_ks(m):
        check(raw_topk(lib, ad, k, n, rb, bd, k, m, cb, k, top_k), s, top_k, what="%s n=%d m=%d k=%d top_k=%d" % (kind, n, m, k, top_k))


def test_one_sided_bias_and_no_count(lib, cases):
    """A row bias alone and a column bias alone (the other NULL: 0) are the PLDA epilogue with a zero vector; count_dev NULL."""
    n, m, k = 129, 1000, 200
    ad, bd, rb, cb, _ = cases[(n, m, k, "plda")]
    zr, zc = _dev(np.zeros(n, np.float32)), _dev(np.zeros(m, np.float32))
    check(raw_topk(lib, ad, k, n, rb, bd, k, m, None, k, 64), lib_matrix(lib, ad, rb, bd, zc), 64, what="row bias only")
    check(raw_topk(lib, ad, k, n, None, bd, k, m, cb, k, 64, count=False), lib_matrix(lib, ad, zr, bd, cb), 64,
          what="column bias only", count=False)


def test_rows_longer_than_the_lds_stage(lib):
    """m above 12288: the sweeps read the panel in global memory; with and without exclusion labels."""
    rng = np.random.default_rng(77)
    n, m, k = 3, 12301, 16
    a, b = rng.standard_normal((n, k)).astype(np.float32), rng.standard_normal((m, k)).astype(np.float32)
    b[5000:5040] = b[100:140]                                   # equal scores far apart
    ad, bd = _dev(a), _dev(b)
    s = lib_matrix(lib, ad, None, bd, None)
    la, lb = np.array([0, 1, 2], np.int32), rng.integers(0, 40, m).astype(np.int32)
    for top_k in (1, 7, 1024):                                   # 1024: the select runs all three digits; 1, 7: it stops after one
        check(raw_topk(lib, ad, k, n, None, bd, k, m, None, k, top_k), s, top_k, what="long row top_k=%d" % top_k)
        check(raw_topk(lib, ad, k, n, None, bd, k, m, None, k, top_k, _dev(la), _dev(lb)), s, top_k, la, lb,
              what="long row, labels, top_k=%d" % top_k)
        # a workspace 4 bytes past a 16-byte boundary: the sweeps without 16-byte loads
        check(raw_topk(lib, ad, k, n, None, bd, k, m, None, k, top_k, ws_shift=4), s, top_k, what="long row, shifted workspace")


# ------------------------------------------------------------------------------------------------ 2
def test_ties(lib):
    """ref_topk.tie_operands: small integers, most scores collide, the gallery in four copies.  The count of rows whose
    boundary falls inside a run of equal scores keeps the test from passing on tie-free data (tests/test_topk_host.py checks
    the construction without a device)."""
    a, b = ref_topk.tie_operands()
    ad, bd = _dev(a), _dev(b)
    s = lib_matrix(lib, ad, None, bd, None)
    assert np.array_equal(s, a @ b.T)
    for top_k in (1, 2, 64, 999):
        inside = ref_topk.boundary_ties(s, top_k)
        print("ties top_k=%d: the boundary falls inside a run of equal scores in %d of %d rows" % (top_k, inside, len(a)))
        assert inside >= 50
        got = raw_topk(lib, ad, 7, 300, None, bd, 7, 1000, None, 7, top_k)
        check(got, s, top_k, what="ties top_k=%d" % top_k)
        # the expected indices are the lowest of each tie: within a row, equal scores come in ascending column order
        sc, ix = got[0][:, :top_k].view(np.float32), got[1][:, :top_k]
        assert np.all((sc[:, 1:] < sc[:, :-1]) | ((sc[:, 1:] == sc[:, :-1]) & (ix[:, 1:] > ix[:, :-1])))


@pytest.mark.parametrize("copies,rows", [(16, 300), (50, 130)])
def test_ties_in_longer_rows(lib, copies, rows):
    """The same block 16 times (m = 4000: a row staged in LDS) and 50 times (m = 12 500: a row swept in global memory): more
    than 1024 scores share the boundary's leading digits, so the select runs all its digits, and the runs of equal scores
    cross the quarters of the row that the four waves compact."""
    a, b = ref_topk.tie_operands()
    a, b = a[:rows], np.tile(b[:250], (copies, 1))
    ad, bd = _dev(a), _dev(b)
    s = lib_matrix(lib, ad, None, bd, None)
    assert np.array_equal(s, a @ b.T)
    for top_k in (2, 64, 1000):
        assert ref_topk.boundary_ties(s, top_k) >= 50
        check(raw_topk(lib, ad, 7, rows, None, bd, 7, len(b), None, 7, top_k), s, top_k, what="ties m=%d top_k=%d" % (len(b), top_k))
    check(raw_topk(lib, ad, 7, rows, None, bd, 7, len(b), None, 7, 64, ws_shift=4), s, 64, what="ties m=%d, shifted workspace" % len(b))


# ------------------------------------------------------------------------------------------------ 3
def test_exclusion(lib):
    rng = np.random.default_rng(3)
    n, k = 300, 200
    a = rng.standard_normal((n, k)).astype(np.float32)
    ad = _dev(a)
    s = lib_matrix(lib, ad, None, ad, None)
    # self-search: no row returns itself, and without the labels every row leads its own list
    ids = np.arange(n, dtype=np.int32)
    got = raw_topk(lib, ad, k, n, None, ad, k, n, None, k, 64, _dev(ids), _dev(ids))
    check(got, s, 64, ids, ids, what="self-search")
    assert not np.any(got[1][:, :64] == ids[:, None])
    assert np.array_equal(raw_topk(lib, ad, k, n, None, ad, k, n, None, k, 1)[1][:, 0], ids)
    # grouped labels: rows of group 0 have 5 eligible columns (partly padded), rows of group 1 have 295, rows of group 2 all 300
    la = (np.arange(n) % 3).astype(np.int32)
    lb = np.where(np.arange(n) < 5, 1, 0).astype(np.int32)
    got = raw_topk(lib, ad, k, n, None, ad, k, n, None, k, 64, _dev(la), _dev(lb))
    check(got, s, 64, la, lb, what="grouped labels")
    assert set(got[2][la == 0]) == {5} and set(got[2][la != 0]) == {64}
    # a gallery that carries one label: the rows of that label have nothing eligible and come back fully padded
    lb = np.full(5, 2, np.int32)
    got = raw_topk(lib, ad, k, n, None, ad[:5], k, 5, None, k, 2, _dev(la), _dev(lb))
    check(got, s[:, :5], 2, la, lb, what="nothing eligible")
    assert np.all(got[2][la == 2] == 0) and np.all(got[1][la == 2][:, :2] == -1) and np.all(got[2][la != 2] == 2)


def test_empty_sides(lib):
    a = _dev(np.ones((3, 4), np.float32))
    got = raw_topk(lib, a, 4, 3, None, a, 4, 0, None, 4, 5)                 # m = 0: the padding is written
    check(got, np.zeros((3, 0), np.float32), 5, what="m = 0")
    assert untouched(raw_topk(lib, a, 4, 0, None, a, 4, 3, None, 4, 5))     # n = 0: nothing is touched


# ------------------------------------------------------------------------------------------------ 4
def test_workspace_sizes_and_repeats(lib, cases):
    n, m, k = 300, 4099, 7
    ad, bd, rb, cb, s = cases[(n, m, k, "plda")]
    least = int(lib.xv_score_topk_workspace(n, m, 64))
    assert least == 128 * 4100 * 4
    first = raw_topk(lib, ad, k, n, rb, bd, k, m, cb, k, 64, ws_bytes=least)
    check(first, s, 64, what="least workspace")
    for ws_bytes in (64 * least, least, least + 1, 2 * least - 1):
        got = raw_topk(lib, ad, k, n, rb, bd, k, m, cb, k, 64, ws_bytes=ws_bytes)
        assert all(np.array_equal(g, f) for g, f in zip(got, first)), ws_bytes
    from tf_kaldi_speaker_amd import _lib
    assert untouched(raw_topk(lib, ad, k, n, rb, bd, k, m, cb, k, 64, ws_bytes=least - 1, expect=_lib.XV_ERR_WORKSPACE))


def test_repeats_on_one_stream(lib):
    import torch
    a, b = ref_topk.tie_operands()
    ad, bd = _dev(a), _dev(b)
    n, m, top_k = 300, 1000, 64
    ws_bytes = int(lib.xv_score_topk_workspace(n, m, top_k))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    outs = [(torch.zeros((n, top_k), dtype=torch.float32, device=DEV), torch.zeros((n, top_k), dtype=torch.int32, device=DEV),
             torch.zeros((n,), dtype=torch.int32, device=DEV)) for _ in range(3)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for sc, ix, cnt in outs:                                    # back to back, one workspace, no wait in between
            assert lib.xv_score_topk(0, _ptr(ad), 7, n, None, None, _ptr(bd), 7, m, None, None, 7, top_k, _ptr(sc), _ptr(ix), top_k,
                                     _ptr(cnt), _ptr(ws), ws_bytes, ctypes.c_void_p(stream.cuda_stream)) == 0
    stream.synchronize()
    for o in outs[1:]:
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(o, outs[0]))
    want = ref_topk.top_k(a @ b.T, top_k)
    assert np.array_equal(outs[0][1].cpu().numpy(), want[1]) and np.array_equal(outs[0][0].cpu().numpy(), want[0])


# ------------------------------------------------------------------------------------------------ 5
def test_layouts(lib):
    """Padded leading dimensions, some of them no multiple of 4, and base pointers one and three floats past a 16-byte boundary
    (the loader without vector loads): the same bits as the packed call, inputs left as they were."""
    rng = np.random.default_rng(7)
    n, m, k = 131, 270, 37
    a, b = rng.standard_normal((n, k)).astype(np.float32), rng.standard_normal((m, k)).astype(np.float32)
    rb, cb = _dev((0.25 * rng.standard_normal(n)).astype(np.float32)), _dev((0.25 * rng.standard_normal(m)).astype(np.float32))
    la, lb = _dev(rng.integers(0, 9, n).astype(np.int32)), _dev(rng.integers(0, 9, m).astype(np.int32))
    for bias in (False, True):
        r, c = (rb, cb) if bias else (None, None)
        s = lib_matrix(lib, _dev(a), r, _dev(b), c)
        for pa, pb in L.PAIRS:
            fa, fb = L.place(a, pa, DEV)[0], L.place(b, pb, DEV)[0]
            got = raw_topk(lib, fa.ptr, fa.ld, n, r, fb.ptr, fb.ld, m, c, k, 10, la, lb)
            assert L.intact(fa, a) and L.intact(fb, b), (pa, pb)
            check(got, s, 10, la.cpu().numpy(), lb.cpu().numpy(), what="layouts %s %s bias=%s" % (pa, pb, bias))


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("mixed", [False, True])
def test_plda_both_directions(lib, mixed):
    """A synthetic model (d = 16).  per="enroll" is llr_matrix's operand order; per="test" is xv_plda_matrix called with the
    test side first (tau as the row bias, rho as the column bias; an enrolment set of mixed num_utts has no tau: zeros)."""
    import torch
    from tf_kaldi_speaker_amd import _lib, plda
    rng = np.random.default_rng(8)
    d = 16
    pm, ptm, psi = ref_plda.random_model(rng, d)
    model = plda.Plda(0.02 * pm, ptm * np.sqrt(d), psi)
    xe = ref_plda.draw(rng, model.mean, model.transform, model.psi, 70, 2, 1.0)[0].astype(np.float32)       # 140 enrolment rows
    xt = ref_plda.draw(rng, model.mean, model.transform, model.psi, 45, 1, 1.0)[0].astype(np.float32)
    num_utts = rng.integers(1, 4, len(xe)) if mixed else np.full(len(xe), 3)
    enroll, test = plda.prepare_enroll(model, xe, num_utts=num_utts), plda.prepare_test(model, xt)
    assert (enroll.uniform_n is None) == mixed
    n, m = len(enroll), len(test)
    le, lt = np.arange(n) // 2, np.arange(m) + 10                  # test row j may not find enrolment rows 2 j + 20, 2 j + 21
    s = plda.llr_matrix(enroll, test)
    for top_k in (1, 10, 64):
        got = plda.llr_top_k(enroll, test, top_k, per="enroll", labels_enroll=le, labels_test=lt)
        ws, wi, wc = ref_topk.top_k(s, top_k, le, lt)
        assert got.scores.dtype == np.float32 and got.indices.dtype == np.int32 and got.count.dtype == np.int32
        assert np.array_equal(got.indices, wi) and np.array_equal(got.count, wc)
        assert np.array_equal(got.scores.view(np.uint32), ws.view(np.uint32))
    k = enroll.k
    tau = test.tau(enroll.uniform_n) if not mixed else torch.zeros(m, dtype=torch.float32, device=DEV)
    swapped = torch.empty((m, n), dtype=torch.float32, device=DEV)
    _lib.check(lib.xv_plda_matrix(0, _lib.ptr(test.packed), test.packed.shape[1], m, _lib.ptr(tau), _lib.ptr(enroll.packed),
                                  enroll.packed.shape[1], n, _lib.ptr(enroll.bias), k, _lib.ptr(swapped), n, None))
    st = swapped.cpu().numpy()
    for top_k in (1, 10, 200):                                     # 200 > the 140 enrolment rows: padded
        got = plda.llr_top_k(enroll, test, top_k, per="test", labels_enroll=le, labels_test=lt)
        ws, wi, wc = ref_topk.top_k(st, top_k, lt, le)
        assert got.scores.shape == (m, top_k)
        assert np.array_equal(got.indices, wi) and np.array_equal(got.count, wc)
        assert np.array_equal(got.scores.view(np.uint32), ws.view(np.uint32))
        assert np.all(got.count == min(top_k, n - 2))


# ------------------------------------------------------------------------------------------------ 7
def test_argument_errors_leave_the_outputs(lib):
    from tf_kaldi_speaker_amd import _lib
    a = _dev(np.ones((4, 8), np.float32))
    ids = _dev(np.arange(4, dtype=np.int32))
    U, I = _lib.XV_ERR_UNSUPPORTED, _lib.XV_ERR_INVALID
    assert untouched(raw_topk(lib, a, 8, 4, None, a, 8, 4, None, 8, 0, ldo=8, expect=U))
    assert untouched(raw_topk(lib, a, 8, 4, None, a, 8, 4, None, 8, 1025, ldo=1030, expect=U))
    assert untouched(raw_topk(lib, a, 8, 4, None, a, 8, 4, None, 0, 3, expect=U))
    assert untouched(raw_topk(lib, a, 2049, 4, None, a, 2049, 4, None, 2049, 3, expect=U))
    assert untouched(raw_topk(lib, a, 8, 4, None, a, 8, 4, None, 8, 3, ldo=2, expect=I))
    assert untouched(raw_topk(lib, a, 8, 4, None, a, 8, 4, None, 8, 3, la=ids, expect=I))
    assert untouched(raw_topk(lib, a, 8, 4, None, a, 8, 4, None, 8, 3, lb=ids, expect=I))
    assert b"xv_score_topk" in lib.xv_last_error(None)


# ------------------------------------------------------------------------------------------------ 8
def test_python_surface(lib):
    import torch
    from tf_kaldi_speaker_amd import scoring
    rng = np.random.default_rng(9)
    x, g = rng.standard_normal((25, 24)).astype(np.float32), rng.standard_normal((40, 24)).astype(np.float32)
    xp, gp = scoring.prepare(x), scoring.prepare(g)
    s = scoring.cosine_matrix(xp, gp)
    labels_q, labels_g = ["s%d" % (i % 7) for i in range(25)], ["s%d" % (i % 9) for i in range(40)]
    for k, la, lb in ((10, None, None), (45, None, None), (10, labels_q, labels_g)):
        ws, wi, wc = ref_topk.top_k(s, k, la, lb)
        got = scoring.top_k(xp, gp, k, labels_a=la, labels_b=lb)
        assert isinstance(got, scoring.TopK) and got.scores.shape == (25, k)
        assert np.array_equal(got.scores.view(np.uint32), ws.view(np.uint32)) and np.array_equal(got.indices, wi)
        assert np.array_equal(got.count, wc)
        t = scoring.top_k(torch.from_numpy(xp).to(DEV), torch.from_numpy(gp).to(DEV), k, labels_a=la, labels_b=lb, as_tensor=True)
        assert t.scores.is_cuda and t.indices.dtype == torch.int32 and np.array_equal(t.indices.cpu().numpy(), wi)
    with pytest.raises(ValueError):
        scoring.top_k(xp, gp, 0)
    with pytest.raises(ValueError):
        scoring.top_k(xp, gp, 1025)
    empty = scoring.top_k(xp[:0], gp, 3)
    assert empty.scores.shape == (0, 3) and empty.count.shape == (0,)


def test_command_line(lib, repo_root, tmp_path):
    """40 gallery and 25 query vectors as ark, the tool in a child process: the file against the rule over
    scoring.cosine_matrix, the rank line against rates counted by hand."""
    from tf_kaldi_speaker_amd import native_ark, scoring
    rng = np.random.default_rng(10)
    cent = rng.standard_normal((11, 24))
    gspk, qspk = [i % 10 for i in range(40)], [i % 11 for i in range(25)]         # speaker 10 is not in the gallery
    g = (cent[gspk] + 0.8 * rng.standard_normal((40, 24))).astype(np.float32)
    q = (cent[qspk] + 0.8 * rng.standard_normal((25, 24))).astype(np.float32)
    gkeys, qkeys = ["gal%02d" % i for i in range(40)], ["qry%02d" % i for i in range(25)]
    for name, keys, x in (("gallery", gkeys, g), ("query", qkeys, q)):
        w = native_ark.VectorWriter("ark:%s" % (tmp_path / (name + ".ark")))
        w.write(keys, x)
        w.close()
    (tmp_path / "g2s").write_text("".join("%s spk%d\n" % kv for kv in zip(gkeys, gspk)))
    (tmp_path / "q2s").write_text("".join("%s spk%d\n" % kv for kv in zip(qkeys, qspk)))
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.identify", "--gpu", "0", "--top-k", "10", "--gallery-utt2spk", "g2s",
                        "--query-utt2spk", "q2s", "ark:gallery.ark", "ark:query.ark", "hits"], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    s = scoring.cosine_matrix(scoring.prepare(q), scoring.prepare(g))
    ws, wi, wc = ref_topk.top_k(s, 10)
    want = "".join("%s %s %g\n" % (qkeys[i], gkeys[wi[i, j]], ws[i, j]) for i in range(25) for j in range(wc[i]))
    assert (tmp_path / "hits").read_text() == want and len(want.splitlines()) == 250
    rates = []
    for rank in (1, 5, 10):
        rates.append(sum(any(gspk[j] == qspk[i] for j in wi[i, :rank]) for i in range(25)) / 25.0)
    absent = sum(1 for v in qspk if v not in gspk)
    assert absent == 2 and 0.0 < rates[0] <= rates[1] <= rates[2] <= 23 / 25.0
    assert r.stdout.strip() == "rank-1 %.4f rank-5 %.4f rank-10 %.4f (25 queries, %d without a gallery entry)" % (tuple(rates) + (absent,))
    mine, _ = scoring.identification_rate(wi, ["spk%d" % v for v in qspk], ["spk%d" % v for v in gspk])
    assert list(mine.values()) == rates
