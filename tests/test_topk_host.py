"""CPU: identification without a device: the numpy rule (tests/helpers/ref_topk.py) on cases worked out by hand,
scoring.identification_rate, the argument checks of xv_score_topk through the built library (they come before the first HIP
call), the workspace size, and the argument parsing and output formatting of the identify tool with the search stood in for by
the numpy rule."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_topk  # noqa: E402

INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the rule
S = np.array([[1.0, 5.0, 3.0, 5.0, 2.0],
              [2.0, 2.0, 2.0, 2.0, 2.0],
              [-1.0, 0.0, -0.0, -7.0, 0.0]], np.float32)


def test_rule_by_hand():
    s, i, c = ref_topk.top_k(S, 3)
    assert s.dtype == np.float32 and i.dtype == np.int32 and c.dtype == np.int32
    assert i.tolist() == [[1, 3, 2], [0, 1, 2], [1, 2, 4]]          # equal scores: lowest column first; -0.0 ties with 0.0
    assert s.tolist() == [[5.0, 5.0, 3.0], [2.0, 2.0, 2.0], [0.0, -0.0, 0.0]]
    assert np.signbit(s[2]).tolist() == [False, True, False]         # the bits of the matrix, not of the key
    assert c.tolist() == [3, 3, 3]
    s, i, c = ref_topk.top_k(S, 1)
    assert i.tolist() == [[1], [0], [1]]


def test_rule_pads_past_the_columns():
    s, i, c = ref_topk.top_k(S, 7)
    assert c.tolist() == [5, 5, 5]
    assert i[0].tolist() == [1, 3, 2, 4, 0, -1, -1] and s[0].tolist() == [5.0, 5.0, 3.0, 2.0, 1.0, -INF, -INF]
    s, i, c = ref_topk.top_k(np.zeros((2, 0), np.float32), 2)
    assert c.tolist() == [0, 0] and np.all(i == -1) and np.all(s == -INF)


def test_rule_with_exclusion():
    la, lb = ["a", "b", "c"], ["x", "a", "x", "b", "b"]
    s, i, c = ref_topk.top_k(S, 3, la, lb)
    assert i.tolist() == [[3, 2, 4], [0, 1, 2], [1, 2, 4]]           # row 0 loses column 1, row 1 columns 3 and 4
    assert c.tolist() == [3, 3, 3]
    s, i, c = ref_topk.top_k(S, 4, la, lb)
    assert c.tolist() == [4, 3, 4] and i[1].tolist() == [0, 1, 2, -1] and s[1, 3] == -INF
    s, i, c = ref_topk.top_k(S, 2, ["a", "b", "c"], ["b"] * 5)
    assert c.tolist() == [2, 0, 2] and i[1].tolist() == [-1, -1] and np.all(s[1] == -INF)
    assert ref_topk.boundary_ties(S, 1) == 3 and ref_topk.boundary_ties(S, 2) == 2 and ref_topk.boundary_ties(S, 5) == 0
    assert ref_topk.boundary_ties(S, 1, la, lb) == 2                 # row 0 has lost one of its two fives


def test_tie_construction():
    """What tests/test_gpu_topk.py::test_ties relies on: with these operands the selection boundary falls inside a run of
    equal scores in at least 50 rows, for every top_k it uses, and the rule then takes the lowest columns of the run."""
    a, b = ref_topk.tie_operands()
    s = a @ b.T
    assert np.array_equal(s, np.round(s)) and np.array_equal(b[:250], b[750:])
    for top_k in (1, 2, 64, 999):
        assert ref_topk.boundary_ties(s, top_k) >= 50, top_k
    sc, ix, _ = ref_topk.top_k(s, 64)
    assert np.all((sc[:, 1:] < sc[:, :-1]) | ((sc[:, 1:] == sc[:, :-1]) & (ix[:, 1:] > ix[:, :-1])))
    last = sc[:, -1:]                                                # every column left out with the boundary score is higher
    for i in range(0, 300, 37):
        left_out = np.setdiff1d(np.flatnonzero(s[i] == last[i]), ix[i])
        assert left_out.size == 0 or left_out.min() > ix[i][sc[i] == last[i]].max()


# ------------------------------------------------------------------------------------------------ identification_rate
def test_identification_rate_by_hand():
    from tf_kaldi_speaker_amd import scoring
    gallery = np.array(["A", "B", "C", "A", "D"])
    queries = np.array(["A", "B", "Z", "D", "C"])
    idx = np.array([[0, 1, 2],        # A at rank 1
                    [2, 0, 1],        # B at rank 3
                    [4, 3, 2],        # Z is not in the gallery
                    [1, 4, -1],       # D at rank 2, one padded position
                    [-1, -1, -1]])    # nothing eligible
    rates, absent = scoring.identification_rate(idx, queries, gallery, ranks=(1, 2, 3))
    assert list(rates.items()) == [(1, 1 / 5), (2, 2 / 5), (3, 3 / 5)] and absent == 1
    rates, absent = scoring.identification_rate(idx[:, :1], queries, gallery, ranks=(1,))
    assert rates[1] == 1 / 5 and absent == 1
    with pytest.raises(ValueError):
        scoring.identification_rate(idx, queries, gallery, ranks=(1, 4))         # a rank beyond the hits
    with pytest.raises(ValueError):
        scoring.identification_rate(idx, queries[:4], gallery)
    with pytest.raises(ValueError):
        scoring.identification_rate(np.array([[5]]), ["A"], gallery, ranks=(1,))
    rates, absent = scoring.identification_rate(np.zeros((0, 10), np.int32), [], gallery)
    assert list(rates.values()) == [0.0, 0.0, 0.0] and absent == 0
    # the second A of the gallery counts as well as the first
    rates, _ = scoring.identification_rate(np.array([[1, 3]]), ["A"], gallery, ranks=(1, 2))
    assert rates[1] == 0.0 and rates[2] == 1.0


# ------------------------------------------------------------------------------------------------ C ABI
def test_library_refuses_bad_arguments_before_the_first_hip_call(lib):
    from tf_kaldi_speaker_amd import _lib
    buf = (ctypes.c_float * 4096)()
    ibuf = (ctypes.c_int32 * 4096)()
    p, ip = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ibuf, ctypes.c_void_p)
    n, m, k = 2, 5, 4
    need = lib.xv_score_topk_workspace(n, m, 3)
    assert need >= 128 * m * 4

    def call(n=n, m=m, k=k, top_k=3, la=None, lb=None, ws=p, ws_bytes=need, scores=p, index=ip, a=p, lda=None, ldo=None):
        return lib.xv_score_topk(0, a, max(k, 1) if lda is None else lda, n, None, la, p, max(k, 1), m, None, lb, k, top_k, scores,
                                 index, top_k if ldo is None else ldo, None, ws, ws_bytes, None)
    assert call(top_k=0) == _lib.XV_ERR_UNSUPPORTED
    assert call(top_k=1025) == _lib.XV_ERR_UNSUPPORTED
    assert call(top_k=-1) == _lib.XV_ERR_UNSUPPORTED
    assert call(k=0) == _lib.XV_ERR_UNSUPPORTED
    assert call(k=2049) == _lib.XV_ERR_UNSUPPORTED
    assert call(ldo=2) == _lib.XV_ERR_INVALID
    assert call(la=ip) == _lib.XV_ERR_INVALID
    assert call(lb=ip) == _lib.XV_ERR_INVALID
    assert call(ws_bytes=need - 1) == _lib.XV_ERR_WORKSPACE
    assert call(ws=None) == _lib.XV_ERR_WORKSPACE
    assert call(scores=None) == _lib.XV_ERR_INVALID
    assert call(index=None) == _lib.XV_ERR_INVALID
    assert call(a=None) == _lib.XV_ERR_INVALID
    assert call(lda=k - 1) == _lib.XV_ERR_INVALID
    assert call(m=2 ** 31) == _lib.XV_ERR_INVALID
    assert call(n=2 ** 31) == _lib.XV_ERR_INVALID
    assert call(n=0, ws=None, ws_bytes=0, scores=None, index=None) == _lib.XV_OK     # nothing to do, nothing touched
    assert call(n=0, top_k=0) == _lib.XV_ERR_UNSUPPORTED                              # the checks come first all the same
    assert b"xv_score_topk" in lib.xv_last_error(None)
    assert not any(buf) and not any(ibuf)


def test_workspace_is_monotone_and_one_panel(lib):
    last = -1
    for m in (0, 1, 3, 4, 5, 127, 128, 129, 1000, 4099, 12288, 12289, 100000, 2 ** 31 - 1):
        w = lib.xv_score_topk_workspace(1000, m, 10)
        assert w >= 128 * m * 4 and w >= last
        last = w
        sizes = [lib.xv_score_topk_workspace(n, m, 10) for n in (0, 1, 128, 129, 10 ** 6)]
        assert sizes == sorted(sizes) and sizes[0] == sizes[-1] == w            # monotone in n: one panel serves any n
        assert all(lib.xv_score_topk_workspace(1000, m, t) == w for t in (1, 2, 64, 1024))     # and any legal top_k
    assert lib.xv_score_topk_workspace(300, 4099, 10) == 128 * 4100 * 4
    assert lib.xv_score_topk_workspace(-1, 5, 1) < 0
    assert lib.xv_score_topk_workspace(5, 2 ** 31, 1) < 0
    assert lib.xv_score_topk_workspace(5, 5, 0) < 0 and lib.xv_score_topk_workspace(5, 5, 1025) < 0


def test_top_k_without_a_device_raises(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from tf_kaldi_speaker_amd import scoring
    x = np.zeros((2, 4), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.top_k(x, x, 1)
    with pytest.raises(ValueError):
        scoring.top_k(x, np.zeros((2, 5), np.float32), 1)
    with pytest.raises(ValueError):
        scoring.top_k(x, x, 1, labels_a=[0, 1])
    with pytest.raises(ValueError):
        scoring.top_k(x, x, 1, labels_a=[0, 1, 2], labels_b=[0, 1])


# ------------------------------------------------------------------------------------------------ command line
def test_option_parsing():
    from tf_kaldi_speaker_amd import identify
    a = identify.parse_args(["g.ark", "q.ark", "out"])
    assert (a.gpu, a.top_k, a.mean, a.transform, a.normalize, a.plda, a.ranks) == (0, 10, "", "", True, "", [1, 5, 10])
    assert (a.gallery_rspecifier, a.query_rspecifier, a.out) == ("g.ark", "q.ark", "out")
    assert (a.smoothing, a.normalize_length, a.simple_length_normalization, a.num_utts) == (0.0, True, False, None)
    a = identify.parse_args(["--gpu", "3", "--top-k", "7", "--plda", "plda", "--num-utts", "ark:n.ark", "--smoothing", "0.5",
                             "--exclude-utt2spk", "u2s", "--gallery-utt2spk", "g2s", "--query-utt2spk", "q2s", "g", "q", "-"])
    assert (a.gpu, a.top_k, a.plda, a.num_utts, a.smoothing, a.exclude_utt2spk) == (3, 7, "plda", "ark:n.ark", 0.5, "u2s")
    assert a.ranks == [1, 5]                                          # the default ranks as far as --top-k allows
    a = identify.parse_args(["--top-k", "20", "--gallery-utt2spk", "g2s", "--query-utt2spk", "q2s", "--ranks", "1,20", "g", "q", "o"])
    assert a.ranks == [1, 20]
    for argv in (["--top-k", "0"], ["--top-k", "1025"], ["--num-utts", "ark:n.ark"], ["--smoothing", "0.1"],
                 ["--plda", "p", "--smoothing", "2"], ["--gallery-utt2spk", "g2s"], ["--query-utt2spk", "q2s"], ["--ranks", "1"],
                 ["--gallery-utt2spk", "g2s", "--query-utt2spk", "q2s", "--ranks", "1,11"],
                 ["--gallery-utt2spk", "g2s", "--query-utt2spk", "q2s", "--ranks", "0"]):
        with pytest.raises(SystemExit):
            identify.parse_args(argv + ["g", "q", "o"])
    with pytest.raises(SystemExit):
        identify.parse_args(["g", "q"])


def test_formatting():
    from tf_kaldi_speaker_amd import identify, scoring
    hits = scoring.TopK(np.array([[0.5, 0.25], [1e-7, -INF]], np.float32), np.array([[2, 0], [1, -1]], np.int32),
                        np.array([2, 1], np.int32))
    assert identify.format_hits(["q0", "q1"], ["g0", "g1", "g2"], hits) == "q0 g2 0.5\nq0 g0 0.25\nq1 g1 1e-07\n"
    import collections
    line = identify.format_rates(collections.OrderedDict([(1, 0.97314), (5, 0.9912), (10, 0.995)]), 1200, 3)
    assert line == "rank-1 0.9731 rank-5 0.9912 rank-10 0.9950 (1200 queries, 3 without a gallery entry)"


def test_run_with_the_search_stood_in_for(lib, tmp_path, monkeypatch, capsys):
    """identify on small tables: scoring.prepare and scoring.top_k are stood in for by numpy (no GPU here); the file and the
    rank line are what the rule gives for the same scores."""
    from tf_kaldi_speaker_amd import identify, native_ark, scoring
    rng = np.random.default_rng(11)
    spk = ["s%d" % (i % 6) for i in range(14)]
    gkeys, qkeys = ["gal%02d" % i for i in range(14)], ["qry%02d" % i for i in range(9)]
    cent = rng.standard_normal((7, 12))
    g = (cent[[i % 6 for i in range(14)]] + 0.3 * rng.standard_normal((14, 12))).astype(np.float32)
    qspk = [0, 1, 2, 3, 4, 5, 6, 0, 1]                               # speaker 6 is not in the gallery
    q = (cent[qspk] + 0.3 * rng.standard_normal((9, 12))).astype(np.float32)
    for name, keys, x in (("g", gkeys, g), ("q", qkeys, q)):
        w = native_ark.VectorWriter("ark:%s" % (tmp_path / (name + ".ark")))
        w.write(keys, x)
        w.close()
    (tmp_path / "g2s").write_text("".join("%s %s\n" % kv for kv in zip(gkeys, spk)))
    (tmp_path / "q2s").write_text("".join("%s s%d\n" % kv for kv in zip(qkeys, qspk)))
    (tmp_path / "excl").write_text("qry00 X\ngal00 X\ngal06 X\n")     # query 0 may not find gallery entries 0 and 6

    def prepare(v, mean=None, transform=None, normalize=True, eps=0.0, device=0, as_tensor=False):
        v = np.asarray(v, np.float32)
        return v / np.sqrt(np.sum(v * v, axis=1, keepdims=True))

    seen = {}

    def top_k(a, b, k, labels_a=None, labels_b=None, device=0, as_tensor=False):
        seen["labels"] = (labels_a, labels_b)
        return scoring.TopK(*ref_topk.top_k((a @ b.T).astype(np.float32), k, labels_a, labels_b))
    monkeypatch.setattr(scoring, "prepare", prepare)
    monkeypatch.setattr(scoring, "top_k", top_k)
    rc = identify.main(["--top-k", "5", "--exclude-utt2spk", str(tmp_path / "excl"), "--gallery-utt2spk", str(tmp_path / "g2s"),
                        "--query-utt2spk", str(tmp_path / "q2s"), "--ranks", "1,3", "ark:%s" % (tmp_path / "g.ark"),
                        "ark:%s" % (tmp_path / "q.ark"), str(tmp_path / "out")])
    assert rc == 0
    la, lb = seen["labels"]
    assert la[0] == lb[0] == lb[6] and len(set(la) | set(lb)) == 9 + 14 - 2
    s, idx, cnt = ref_topk.top_k((prepare(q) @ prepare(g).T).astype(np.float32), 5, la, lb)
    want = "".join("%s %s %g\n" % (qkeys[i], gkeys[idx[i, r]], s[i, r]) for i in range(9) for r in range(cnt[i]))
    assert (tmp_path / "out").read_text() == want
    assert not any(ln.startswith("qry00 gal00 ") or ln.startswith("qry00 gal06 ") for ln in want.splitlines())
    hit1 = sum(spk[idx[i, 0]] == "s%d" % qspk[i] for i in range(9))
    hit3 = sum(any(spk[j] == "s%d" % qspk[i] for j in idx[i, :3]) for i in range(9))
    assert capsys.readouterr().out.strip() == "rank-1 %.4f rank-3 %.4f (9 queries, 1 without a gallery entry)" % (hit1 / 9, hit3 / 9)
    # an utt2spk that lacks a key is reported, not guessed
    (tmp_path / "short").write_text("gal00 s0\n")
    rc = identify.main(["--gallery-utt2spk", str(tmp_path / "short"), "--query-utt2spk", str(tmp_path / "q2s"),
                        "ark:%s" % (tmp_path / "g.ark"), "ark:%s" % (tmp_path / "q.ark"), str(tmp_path / "out2")])
    assert rc == 1


def test_wrapper_script_names_the_tool(repo_root):
    text = open(os.path.join(repo_root, "bin", "identify.sh")).read()
    assert "tf_kaldi_speaker_amd.identify" in text and os.access(os.path.join(repo_root, "bin", "identify.sh"), os.X_OK)
