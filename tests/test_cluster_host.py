"""No GPU: the numpy statement of the clustering rule (tests/helpers/ref_cluster.py) against an independent exact clustering, the
tie construction the GPU tests rely on, the stop and numbering rules, and the host plumbing of the two commands (RTTM, window
planning, table parsing, argument errors)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_cluster  # noqa: E402


def _log(res):
    _, count, ma, mb, mh = res
    m = len(ma) - count if len(ma) else 0
    return list(zip(ma[:m].tolist(), mb[:m].tolist())), mh[:m]


# ------------------------------------------------------------------------------------------------ oracle
def test_oracle_against_exact_clustering():
    """Random float32 rows, n = 60, d = 16, seed 4: in the exact float64 run the best linkage of every step leads the second best
    by more than 2 n 2^-24 max|s| (twice the bound on the error of a float32 linkage), so no rounding can change a choice: the
    merge pairs are equal and the heights agree to n 2^-24 max|s|."""
    n = 60
    x = np.random.default_rng(4).standard_normal((n, 16)).astype(np.float32)
    s = (x @ x.T).astype(np.float32)
    smax = float(np.abs(np.triu(s, 1)).max())
    exact = ref_cluster.ahc_exact(s)
    assert len(exact) == n - 1
    assert min(gap for _, _, _, gap in exact[:-1]) > 2 * n * 2.0 ** -24 * smax
    pairs, heights = _log(ref_cluster.ahc(s))
    assert pairs == [(a, b) for a, b, _, _ in exact]
    assert np.max(np.abs(heights - np.array([L for _, _, L, _ in exact]))) <= n * 2.0 ** -24 * smax
    assert ref_cluster.shared_maximum_steps(s) == 0


def test_only_the_upper_triangle_is_read():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((23, 8)).astype(np.float32)
    s = (x @ x.T).astype(np.float32)
    t = np.full((23, 28), np.nan, np.float32)                         # padding columns, diagonal, lower triangle: NaN
    iu = np.triu_indices(23, 1)
    t[iu] = s[iu]
    a, b = ref_cluster.ahc(s), ref_cluster.ahc(t)
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def test_tie_construction():
    """The tie matrices really have ties: most steps see several live pairs at the maximum (46 and 242 when written)."""
    s65, s300 = ref_cluster.tie_scores(65), ref_cluster.tie_scores(300)
    assert s65.shape == (65, 65) and s65.dtype == np.float32 and np.array_equal(s65, np.round(s65))
    assert ref_cluster.shared_maximum_steps(s65) >= 40
    assert ref_cluster.shared_maximum_steps(s300) >= 200


def test_tie_rule_by_hand():
    """Four rows, s(0, 2) = s(1, 3) = 3: two pairs at the maximum, the lowest row wins, then (1, 3) at the same height; the
    last merge has S = (s01 + s12) + (s03 + s23) = 1 + 1 over 2 x 2 pairs."""
    s = np.array([[9, 1, 3, 0], [9, 9, 0, 3], [9, 9, 9, 1], [9, 9, 9, 9]], np.float32)
    labels, count, ma, mb, mh = ref_cluster.ahc(s)
    assert ma.tolist() == [0, 1, 0, -1] and mb.tolist() == [2, 3, 1, -1]
    assert mh[:3].tolist() == [3.0, 3.0, 0.5] and np.isnan(mh[3])
    assert count == 1 and labels.tolist() == [0, 0, 0, 0]
    assert ref_cluster.shared_maximum_steps(s) == 1
    # equal heights come in (a, b) order
    pairs, heights = _log(ref_cluster.ahc(ref_cluster.tie_scores(65)))
    for i in range(len(pairs) - 1):
        assert heights[i] != heights[i + 1] or pairs[i] < pairs[i + 1]
    assert mh.dtype == np.float64 and ma.dtype == np.int32 and labels.dtype == np.int32


def test_stop_and_numbering_rules():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((30, 6)).astype(np.float32)
    s = (x @ x.T).astype(np.float32)
    full_pairs, full_h = _log(ref_cluster.ahc(s))
    assert len(full_pairs) == 29
    # average linkage has no inversions beyond rounding: stopping at a threshold = cutting the finished log
    assert np.all(np.diff(full_h) <= 30 * 2.0 ** -24 * np.abs(s).max())
    thr = float(full_h[12])
    cut = int(np.count_nonzero(full_h >= thr))
    by_thr = ref_cluster.ahc(s, threshold=thr)
    assert by_thr[1] == 30 - cut and _log(by_thr)[0] == full_pairs[:cut]
    by_target = ref_cluster.ahc(s, target=8)
    assert by_target[1] == 8 and _log(by_target)[0] == full_pairs[:22]
    # whichever comes first
    assert ref_cluster.ahc(s, threshold=thr, target=30 - cut + 5)[1] == 30 - cut + 5
    assert ref_cluster.ahc(s, threshold=thr, target=2)[1] == 30 - cut
    assert ref_cluster.ahc(s, target=30)[1] == 30 and ref_cluster.ahc(s, target=31)[1] == 30
    assert ref_cluster.ahc(s, threshold=np.inf)[1] == 30
    # numbering by lowest row, and labels_from_merges agrees
    for res in (by_thr, by_target):
        labels, count, ma, mb, _ = res
        assert labels[0] == 0 and sorted(set(labels.tolist())) == list(range(count))
        first = [int(np.flatnonzero(labels == c)[0]) for c in range(count)]
        assert first == sorted(first)
        assert np.array_equal(labels, ref_cluster.labels_from_merges(30, ma, mb))
    # the unused slots
    labels, count, ma, mb, mh = by_target
    assert np.all(ma[22:] == -1) and np.all(mb[22:] == -1) and np.all(np.isnan(mh[22:])) and len(ma) == 30
    # degenerate sizes
    assert ref_cluster.ahc(np.zeros((0, 0), np.float32))[1] == 0
    one = ref_cluster.ahc(np.zeros((1, 1), np.float32))
    assert one[0].tolist() == [0] and one[1] == 1 and one[2].tolist() == [-1] and np.isnan(one[4][0])
    # an all-NaN triangle has no pair to merge; a NaN pair is skipped
    assert ref_cluster.ahc(np.full((3, 3), np.nan, np.float32))[1] == 3
    s3 = np.array([[0, np.nan, 1], [0, 0, 2], [0, 0, 0]], np.float32)
    assert _log(ref_cluster.ahc(s3))[0] == [(1, 2)]                  # then S(0, 1) = NaN + 1: nothing left to merge


# ------------------------------------------------------------------------------------------------ host plumbing
def test_rttm():
    from tf_kaldi_speaker_amd import cluster
    segs = [("b2", "recB", 1.0, 2.0), ("a1", "recA", 0.0, 1.5), ("a3", "recA", 2.0, 3.0), ("a2", "recA", 0.75, 2.0),
            ("a4", "recA", 2.5, 4.0), ("a5", "recA", 5.0, 6.0), ("b1", "recB", 0.0, 1.0), ("a6", "recA", 6.0, 6.5), ("zz", "recA", 9.0, 9.5)]
    labels = {"a1": 1, "a2": 1, "a3": 2, "a4": 1, "a5": 1, "a6": 1, "b1": 2, "b2": 2}
    text = cluster.rttm_lines(segs, labels)
    # recA: a1 + a2 merge (same label, overlap) -> [0, 2]; a3 touches it with another label: no cut; a3 / a4 overlap on
    # [2.5, 3] -> cut at 2.75; a5 + a6 touch and merge; zz has no label.  recB: b1 + b2 touch and merge.
    assert text == ("SPEAKER recA 1 0.000 2.000 <NA> <NA> 1 <NA> <NA>\n"
                    "SPEAKER recA 1 2.000 0.750 <NA> <NA> 2 <NA> <NA>\n"
                    "SPEAKER recA 1 2.750 1.250 <NA> <NA> 1 <NA> <NA>\n"
                    "SPEAKER recA 1 5.000 1.500 <NA> <NA> 1 <NA> <NA>\n"
                    "SPEAKER recB 1 0.000 2.000 <NA> <NA> 2 <NA> <NA>\n")
    assert cluster.rttm_lines([], {}) == ""


def test_tables_and_argument_errors(tmp_path):
    from tf_kaldi_speaker_amd import cluster
    (tmp_path / "n").write_text("recA 2\n\nrecB 10\n")
    assert cluster.read_reco2num_spk(str(tmp_path / "n")) == {"recA": 2, "recB": 10}
    for bad in ("recA 0\n", "recA two\n", "recA 2 3\n", "recA -1\n"):
        (tmp_path / "bad").write_text(bad)
        with pytest.raises(ValueError):
            cluster.read_reco2num_spk(str(tmp_path / "bad"))
    (tmp_path / "seg").write_text("k1 recA 0.5 1.25\nk2 recA 1 2\n")
    assert cluster.read_segments(str(tmp_path / "seg")) == [("k1", "recA", 0.5, 1.25), ("k2", "recA", 1.0, 2.0)]
    for bad in ("k1 recA 0.5\n", "k1 recA x 1\n", "k1 recA 2 1\n"):
        (tmp_path / "bad").write_text(bad)
        with pytest.raises(ValueError):
            cluster.read_segments(str(tmp_path / "bad"))
    assert cluster.format_labels(["a", "b"], [0, 2]) == "a 1\nb 3\n"
    assert cluster.matrix_ld(1) == 4 and cluster.matrix_ld(4) == 4 and cluster.matrix_ld(5) == 8 and cluster.matrix_ld(8192) == 8192
    ok = cluster.parse_args(["u2r", "ark:x", "out"])
    assert ok.threshold == 0.0 and not ok.reco2num_spk and ok.normalize is True
    assert cluster.parse_args(["--reco2num-spk", "n", "u2r", "ark:x", "out"]).threshold is None
    assert cluster.parse_args(["--threshold", "-0.5", "u2r", "ark:x", "out"]).threshold == -0.5
    for bad in (["--threshold", "0.1", "--reco2num-spk", "n", "u2r", "ark:x", "out"],
                ["--threshold", "nan", "u2r", "ark:x", "out"],
                ["--smoothing", "0.1", "u2r", "ark:x", "out"],
                ["--plda", "p", "--smoothing", "1.5", "u2r", "ark:x", "out"],
                ["--segments", "s", "u2r", "ark:x", "out"],
                ["--rttm-out", "r", "u2r", "ark:x", "out"],
                ["u2r", "ark:x"]):
        with pytest.raises(SystemExit):
            cluster.parse_args(bad)
    # the checks of the Python layer that need no device
    assert cluster._targets(None, 3) is None and cluster._targets(2, 3).tolist() == [2, 2, 2]
    assert cluster._targets({"a": 1, "b": 4}, 2, ["a", "b"]).tolist() == [1, 4]
    for bad in (0, [1, 2], [1, 0, 1]):
        with pytest.raises(ValueError):
            cluster._targets(bad, 3)
    with pytest.raises(ValueError):
        cluster._threshold(float("nan"))
    assert cluster._threshold(None) == -np.inf
    # chunks: largest first, within the byte budget, and no group under half the rows of the largest of its chunk
    assert cluster._chunks([3, 0, 5, 2], 1 << 20) == [[2, 0], [3], [1]] and cluster._chunks([9, 9], 1) == [[0], [1]]
    assert cluster._chunks([6, 5, 8, 4], 4 * (8 * 8 + 6 * 8)) == [[2, 0], [1, 3]] and cluster._chunks([], 1) == []
    assert cluster._chunks([8192, 300, 4096, 299], 1 << 30) == [[0, 2], [1, 3]]


def test_utt2reco_and_a_key_without_a_recording(tmp_path, capsys):
    """utt2reco is an utt2spk-shaped table; the command refuses an x-vector key without a recording before it needs a device."""
    from tf_kaldi_speaker_amd import cluster, kaldi_io
    from tf_kaldi_speaker_amd.score_cos import read_utt2spk
    (tmp_path / "u2r").write_text("seg1 recA\n\nseg2 recB\nseg3 recA\n")
    assert read_utt2spk(str(tmp_path / "u2r")) == {"seg1": "recA", "seg2": "recB", "seg3": "recA"}
    for bad in ("seg1\n", "seg1 recA extra\n"):
        (tmp_path / "bad").write_text(bad)
        with pytest.raises(ValueError):
            read_utt2spk(str(tmp_path / "bad"))
    with open(str(tmp_path / "x.ark"), "wb") as f:
        for key in ("seg1", "seg2", "seg4"):
            kaldi_io.write_vec_flt(f, np.arange(4, dtype=np.float32), key=key)
    rc = cluster.main([str(tmp_path / "u2r"), "ark:%s" % (tmp_path / "x.ark"), str(tmp_path / "labels")])
    assert rc == 1 and "seg4" in capsys.readouterr().err and not (tmp_path / "labels").exists()
    (tmp_path / "empty.ark").write_bytes(b"")
    assert cluster.main([str(tmp_path / "u2r"), "ark:%s" % (tmp_path / "empty.ark"), str(tmp_path / "labels")]) == 1


def test_window_planning():
    from tf_kaldi_speaker_amd import extract_windows as ew
    W, P, M = 150, 75, 25
    assert ew.plan_windows(24, W, P, M) == []                                    # shorter than min-segment: skipped
    assert ew.plan_windows(25, W, P, M) == [(0, 25)]
    assert ew.plan_windows(150, W, P, M) == [(0, 150)]                           # exactly one window
    assert ew.plan_windows(151, W, P, M) == [(0, 150), (75, 151)]                # one frame more: the last window ends at the end
    assert ew.plan_windows(225, W, P, M) == [(0, 150), (75, 225)]                # exact multiples of the period
    assert ew.plan_windows(300, W, P, M) == [(0, 150), (75, 225), (150, 300)]
    assert ew.plan_windows(301, W, P, M) == [(0, 150), (75, 225), (150, 300), (225, 301)]
    # period = window: the tail is a window of its own and is dropped when it is shorter than min-segment
    assert ew.plan_windows(174, 150, 150, M) == [(0, 150)]
    assert ew.plan_windows(175, 150, 150, M) == [(0, 150), (150, 175)]
    for t in (25, 149, 150, 151, 226, 1000):
        plan = ew.plan_windows(t, W, P, M)
        assert plan[-1][1] == t and all(e - s <= W and e - s >= M for s, e in plan) and [s for s, _ in plan] == [P * i for i in range(len(plan))]
    with pytest.raises(ValueError):
        ew.plan_windows(100, 0, 75, 25)
    assert ew.window_key("utt", 75, 225) == "utt-0000075-0000225"
    assert ew.segment_line("utt", 75, 225, 0.01) == "utt-0000075-0000225 utt 0.750 2.250\n"
    args = ew.parse_args(["exp", "ark:f", "ark:x", "segs"])
    assert (args.window, args.period, args.min_segment, args.frame_shift, args.cmn_window) == (150, 75, 25, 0.01, 0)
    for bad in (["--window", "0", "exp", "ark:f", "ark:x", "segs"], ["--min-segment", "200", "exp", "ark:f", "ark:x", "segs"],
                ["--frame-shift", "0", "exp", "ark:f", "ark:x", "segs"], ["exp", "ark:f", "ark:x"]):
        with pytest.raises(SystemExit):
            ew.parse_args(bad)


# ------------------------------------------------------------------------------------------------ exports
def test_ahc_symbols_are_declared_listed_and_exported(repo_root):
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    assert "cluster.hip" in g.SOURCES and "ahc_kernel" in open(os.path.join(g.CSRC, "cluster.hip")).read()
    # the two host-side helpers need no device
    f = lib.xv_ahc_matrix_floats
    assert [f(n) for n in (0, 1, 3, 4, 5, 8192)] == [0, 4, 12, 16, 40, 8192 * 8192]
    w = lib.xv_ahc_workspace
    rows = np.array([5, 0, 8192], np.int32)
    assert w(3, rows.ctypes.data) == 256 and w(0, None) == 0 and w(9, np.ones(9, np.int32).ctypes.data) == 512
    assert w(3, np.array([5, -1, 2], np.int32).ctypes.data) == _lib.XV_ERR_INVALID
    assert w(1, np.array([8193], np.int32).ctypes.data) == _lib.XV_ERR_UNSUPPORTED                # the codes of xv_ahc
    assert w(2, np.array([8193, -1], np.int32).ctypes.data) == _lib.XV_ERR_UNSUPPORTED
