"""GPU: speaker clustering (xv_ahc, tf_kaldi_speaker_amd.cluster, the cluster and extract_windows tools).

Every comparison of a clustering is exact, bit for bit, against the numpy statement of the rule (tests/helpers/ref_cluster.py)
applied to the library's own score matrix copied to the host before the call.  The oracle runs once per matrix, to the end; by
the rule a run with a threshold or a target is the prefix of that log that the stop conditions allow (tests/test_cluster_host.py
checks this property of the oracle), so the expected result of every variant is cut from the one full log.

Sizes with a path of their own in csrc/cluster.hip, each with a shape on either side:
  64 rows   one ballot chunk of the row recompute (a wave looks at 64 marks at a time): 64 / 65;
  256 rows  the stride of the 256 threads over the cache in the reduction, the merge and the label scan, and one round of
            64-row chunks over the four waves: 255 / 256 / 257, and 513 for the third round.
Output buffers are pre-filled with a canary and over-allocated: nothing past the last slot may be written."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_cluster  # noqa: E402
import ref_plda  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_I, CANARY_D = 0x5A5A5A5A, 0x7FF8A5A5A5A5A5A5
SIZES = [0, 1, 2, 3, 64, 65, 255, 256, 257, 513]
PAD = 5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    return _lib.load()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ld(n):
    return max(4, (n + 3) // 4 * 4)


def offsets(rows):
    return np.concatenate([[0], np.cumsum([n * ld(n) if n else 0 for n in rows])]).astype(np.int64)


def score_matrices(lib, xs):
    """The packed buffer of xv_ahc filled by xv_score_matrix from the rows of every group -> (device buffer, host views [n, ld])."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    rows = [len(x) for x in xs]
    off = offsets(rows)
    s = torch.full((int(off[-1]) + 4,), float("nan"), dtype=torch.float32, device=DEV)
    for g, x in enumerate(xs):
        if len(x):
            xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
            _lib.check(lib.xv_score_matrix(0, _ptr(xd), x.shape[1], len(x), _ptr(xd), x.shape[1], len(x), x.shape[1],
                                           ctypes.c_void_p(s.data_ptr() + 4 * int(off[g])), ld(len(x)), None))
    torch.cuda.synchronize()
    host = s.cpu().numpy()
    return s, [host[off[g]:off[g + 1]].reshape(n, ld(n)) if n else np.zeros((0, 4), np.float32) for g, n in enumerate(rows)]


def upload(mats):
    """Host matrices [n, >= n] -> the packed device buffer (padding columns NaN)."""
    import torch
    rows = [len(m) for m in mats]
    off = offsets(rows)
    flat = np.full(int(off[-1]) + 4, np.nan, np.float32)
    for g, m in enumerate(mats):
        n = rows[g]
        if n:
            flat[off[g]:off[g + 1]].reshape(n, ld(n))[:, :n] = np.asarray(m)[:, :n]
    return torch.from_numpy(flat).to(DEV)


def raw_ahc(lib, s, rows, targets=None, threshold=-np.inf, ws_bytes=None, expect=0, stream=None, out=None, ws=None):
    """xv_ahc on a packed device buffer (destroyed) -> dict of host arrays, PAD canary slots behind the last group."""
    import torch
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    tg = None if targets is None else np.ascontiguousarray(targets, dtype=np.int32)
    total = int(np.maximum(rows, 0).clip(max=8192).sum())
    need = max(int(lib.xv_ahc_workspace(len(rows), rows.ctypes.data_as(ctypes.c_void_p))), 0) or 256 * ((len(rows) * 32 + 255) // 256)
    ws_bytes = need if ws_bytes is None else ws_bytes
    if ws is None:
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    if out is None:
        out = dict(labels=torch.full((total + PAD,), CANARY_I, dtype=torch.int32, device=DEV),
                   count=torch.full((len(rows) + PAD,), CANARY_I, dtype=torch.int32, device=DEV),
                   ma=torch.full((total + PAD,), CANARY_I, dtype=torch.int32, device=DEV),
                   mb=torch.full((total + PAD,), CANARY_I, dtype=torch.int32, device=DEV),
                   mh=torch.full((total + PAD,), CANARY_D, dtype=torch.int64, device=DEV))
    rc = lib.xv_ahc(0, _ptr(s), rows.ctypes.data_as(ctypes.c_void_p), None if tg is None else tg.ctypes.data_as(ctypes.c_void_p),
                    len(rows), threshold, _ptr(out["labels"]), _ptr(out["count"]), _ptr(out["ma"]), _ptr(out["mb"]), _ptr(out["mh"]),
                    _ptr(ws), ws_bytes, None if stream is None else ctypes.c_void_p(stream))
    assert rc == expect, (rc, lib.xv_last_error(None))
    if stream is not None:
        return out
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def untouched(got):
    return bool(all(np.all(got[k] == CANARY_I) for k in ("labels", "count", "ma", "mb")) and np.all(got["mh"] == CANARY_D))


def full_log(s):
    """The oracle, run to the end -> (merge_a, merge_b, merge_height, merges)."""
    n = len(s)
    _, count, ma, mb, mh = ref_cluster.ahc(s)
    return ma, mb, mh, n - count


def cut(full, n, threshold=-np.inf, target=1):
    """What the rule gives with a threshold and a target: the prefix of the full log that the stop conditions allow."""
    ma, mb, mh, merges = full
    m = 0
    while m < merges and n - m > target and mh[m] >= threshold:
        m += 1
    ma, mb, mh = ma.copy(), mb.copy(), mh.copy()
    ma[m:], mb[m:], mh[m:] = -1, -1, np.nan
    return ref_cluster.labels_from_merges(n, ma, mb), n - m, ma, mb, mh


def check(got, rows, want, what=""):
    """Bit for bit per group; unused merge slots -1 / -1 / NaN; the PAD slots behind the last group still the canary."""
    off = 0
    for g, n in enumerate(rows):
        labels, count, ma, mb, mh = want[g]
        assert got["count"][g] == count, (what, g, n)
        sl = slice(off, off + n)
        assert np.array_equal(got["ma"][sl], ma) and np.array_equal(got["mb"][sl], mb), (what, g, n)
        m = n - count
        assert np.array_equal(got["mh"][sl][:m], mh[:m].view(np.int64)), (what, g, n)
        assert np.all(np.isnan(got["mh"][sl][m:].view(np.float64))) and np.all(got["mh"][sl][m:] != CANARY_D), (what, g, n)
        assert np.array_equal(got["labels"][sl], labels), (what, g, n)
        off += n
    for k in ("labels", "ma", "mb"):
        assert np.all(got[k][off:] == CANARY_I), (what, "a store past the last slot of", k)
    assert np.all(got["mh"][off:] == CANARY_D) and np.all(got["count"][len(rows):] == CANARY_I), (what, "a store past the last slot")


@pytest.fixture(scope="module")
def sized(lib):
    """Groups of SIZES rows (d = 16): the pristine packed buffer, the host matrices and the oracle's full logs, made once."""
    rng = np.random.default_rng(11)
    xs = [rng.standard_normal((n, 16)).astype(np.float32) for n in SIZES]
    s, host = score_matrices(lib, xs)
    return s, host, [full_log(h) for h in host]


@pytest.fixture(scope="module")
def tied():
    mats = [ref_cluster.tie_scores(65), ref_cluster.tie_scores(300)]
    return mats, [full_log(m) for m in mats]


# ------------------------------------------------------------------------------------------------ sizes
def test_sizes_no_threshold(lib, sized):
    s, host, full = sized
    got = raw_ahc(lib, s.clone(), SIZES)
    check(got, SIZES, [cut(f, n) for f, n in zip(full, SIZES)], "no threshold")
    assert got["count"][:len(SIZES)].tolist() == [min(n, 1) for n in SIZES]


@pytest.mark.parametrize("group", [4, 8, 9])
def test_sizes_threshold(lib, sized, group):
    """The threshold of the run is a height from the middle of the oracle's log of one group; every group is checked."""
    s, host, full = sized
    thr = float(full[group][2][SIZES[group] // 2])
    want = [cut(f, n, threshold=thr) for f, n in zip(full, SIZES)]
    assert 1 < want[group][1] < SIZES[group]
    check(raw_ahc(lib, s.clone(), SIZES, threshold=thr), SIZES, want, "threshold %r" % thr)


@pytest.mark.parametrize("target", ["1", "2", "n"])
def test_sizes_targets(lib, sized, target):
    s, host, full = sized
    tg = [max(n, 1) if target == "n" else int(target) for n in SIZES]
    want = [cut(f, n, target=t) for f, n, t in zip(full, SIZES, tg)]
    got = raw_ahc(lib, s.clone(), SIZES, targets=tg)
    check(got, SIZES, want, "target %s" % target)
    assert got["count"][:len(SIZES)].tolist() == [min(n, t) for n, t in zip(SIZES, tg)]


def test_threshold_and_target_whichever_comes_first(lib, sized):
    s, host, full = sized
    thr = float(full[8][2][100])
    by_thr = [n - cut(f, n, threshold=thr)[1] for f, n in zip(full, SIZES)]            # merges the threshold alone allows
    assert by_thr[9] >= 2 and by_thr[6] >= 2
    tg = [1, 1, 1, 1, 10, 60, 3, 200, 200, SIZES[9] - by_thr[9] // 2]
    want = [cut(f, n, threshold=thr, target=t) for f, n, t in zip(full, SIZES, tg)]
    assert want[9][1] == tg[9] and want[6][1] == SIZES[6] - by_thr[6] > 3      # the target stops one group, the threshold another
    check(raw_ahc(lib, s.clone(), SIZES, targets=tg, threshold=thr), SIZES, want, "both")


# ------------------------------------------------------------------------------------------------ ties
def test_ties(lib, tied):
    mats, full = tied
    assert ref_cluster.shared_maximum_steps(mats[0]) >= 40 and ref_cluster.shared_maximum_steps(mats[1]) >= 200
    rows = [65, 300]
    got = raw_ahc(lib, upload(mats), rows)
    check(got, rows, [cut(f, n) for f, n in zip(full, rows)], "ties")
    off = 0
    for n in rows:                                                   # equal heights come in (a, b) order
        h = got["mh"][off:off + n - 1].view(np.float64)
        pairs = list(zip(got["ma"][off:off + n - 1].tolist(), got["mb"][off:off + n - 1].tolist()))
        same = [i for i in range(n - 2) if h[i] == h[i + 1]]
        assert len(same) >= 20 and all(pairs[i] < pairs[i + 1] for i in same)
        off += n
    for tg in (7, 64):
        check(raw_ahc(lib, upload(mats), rows, targets=[tg, tg]), rows, [cut(f, n, target=tg) for f, n in zip(full, rows)], "ties target")


# ------------------------------------------------------------------------------------------------ only the upper triangle
def test_only_the_upper_triangle_is_read(lib, sized, tied):
    s, host, full = sized
    mats = []
    for h, n in zip(host, SIZES):
        t = np.full((n, ld(n)), np.nan, np.float32)
        iu = np.triu_indices(n, 1)
        t[iu] = h[:, :n][iu]
        mats.append(t)
    plain = raw_ahc(lib, s.clone(), SIZES)
    nan = raw_ahc(lib, upload(mats), SIZES)
    for k in plain:
        assert np.array_equal(plain[k], nan[k]), k
    check(nan, SIZES, [cut(f, n) for f, n in zip(full, SIZES)], "NaN outside the triangle")
    tmats, tfull = tied
    t = tmats[0].copy()
    t[np.tril_indices(65)] = np.nan
    check(raw_ahc(lib, upload([t]), [65]), [65], [cut(tfull[0], 65)], "ties, NaN outside the triangle")


def test_the_lower_triangle_is_not_written(lib, sized):
    import torch
    s, host, full = sized
    work = s.clone()
    raw_ahc(lib, work, SIZES)
    after = work.cpu().numpy()
    off = offsets(SIZES)
    for g, n in enumerate(SIZES):
        if n:
            a, b = after[off[g]:off[g + 1]].reshape(n, ld(n)), host[g]
            keep = ~np.triu(np.ones((n, ld(n)), bool), 1) | (np.arange(ld(n))[None, :] >= n)
            assert np.array_equal(a[keep].view(np.uint32), b[keep].view(np.uint32)), n
    assert torch.isnan(work[int(off[-1]):]).all()


# ------------------------------------------------------------------------------------------------ a larger group
@pytest.mark.parametrize("n,first", [(2048, 20), (4100, 3)])
def test_larger_group(lib, n, first):
    """2048 rows: the larger group.  csrc/cluster.hip has no size threshold above the 256-row stride named at the top of this
    file (one kernel, one path; the dynamic LDS is 16 bytes per row whatever n), so 2048 is the shape whose first 20 merges are
    bit for bit against the oracle.  The time the oracle would need keeps this from being bit-exact throughout: the rest is
    checked for consistency (labels follow from the log, the count from its length, heights never rise beyond rounding).
    4100 rows is an extra case, not a threshold of the code: its cache needs more than the 64 KiB of LDS a launch gets without
    the attribute that launch_ahc requests at the first launch of every size, so it shows that the runtime grants the request.
    20 oracle steps at that size take 9 s, so only 3 are compared there; the consistency checks are the same."""
    rng = np.random.default_rng(n)
    s, host = score_matrices(lib, [rng.standard_normal((n, 16)).astype(np.float32)])
    h = host[0]
    got = raw_ahc(lib, s, [n])
    _, _, ma, mb, mh = ref_cluster.ahc(h, target=n - first)
    assert np.array_equal(got["ma"][:first], ma[:first]) and np.array_equal(got["mb"][:first], mb[:first])
    assert np.array_equal(got["mh"][:first], mh[:first].view(np.int64))
    merges = int(np.count_nonzero(got["ma"][:n] >= 0))
    assert merges == n - 1 and got["count"][0] == n - merges
    assert np.all(got["ma"][:merges] < got["mb"][:merges]) and got["ma"][n - 1] == -1 and got["mb"][n - 1] == -1
    assert len(set(got["mb"][:merges].tolist())) == merges           # every row dies once
    assert np.array_equal(got["labels"][:n], ref_cluster.labels_from_merges(n, got["ma"][:n], got["mb"][:n]))
    heights = got["mh"][:merges].view(np.float64)
    assert not np.isnan(heights).any() and np.isnan(got["mh"][n - 1:n].view(np.float64)).all()
    assert np.all(np.diff(heights) <= n * 2.0 ** -24 * np.abs(np.triu(h[:, :n], 1)).max())
    assert np.all(got["ma"][n:] == CANARY_I) and np.all(got["mh"][n:] == CANARY_D) and np.all(got["labels"][n:] == CANARY_I)


# ------------------------------------------------------------------------------------------------ independence and repeats
def test_independence_of_batch_and_workspace(lib, sized, tied):
    s, host, full = sized
    g = 8                                                            # the 257-row group
    n = SIZES[g]
    alone = raw_ahc(lib, upload([host[g]]), [n])
    check(alone, [n], [cut(full[g], n)], "alone")
    rows = [65, 3, n, 300, 0, 64]
    mats = [tied[0][0], host[3], host[g], tied[0][1], host[0], host[4]]
    least = int(lib.xv_ahc_workspace(len(rows), np.array(rows, np.int32).ctypes.data_as(ctypes.c_void_p)))
    assert least == 256
    off = 65 + 3
    for ws_bytes in (least, 8 * least):
        got = raw_ahc(lib, upload(mats), rows, ws_bytes=ws_bytes)
        for k in ("labels", "ma", "mb", "mh"):
            assert np.array_equal(got[k][off:off + n], alone[k][:n]), (k, ws_bytes)
        assert got["count"][2] == alone["count"][0]
        check(got, rows, [cut(tied[1][0], 65), cut(full[3], 3), cut(full[g], n), cut(tied[1][1], 300), cut(full[0], 0), cut(full[4], 64)],
              "batch ws=%d" % ws_bytes)


def test_repeats_on_one_stream(lib, tied):
    import torch
    mats, full = tied
    rows = np.array([65, 300], np.int32)
    bufs = [upload(mats) for _ in range(3)]
    ws = torch.empty(256, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        outs = [raw_ahc(lib, b, rows, ws=ws, ws_bytes=256, stream=stream.cuda_stream) for b in bufs]     # back to back, no wait
    stream.synchronize()
    for o in outs[1:]:
        assert all(torch.equal(o[k], outs[0][k]) for k in o)
    check({k: v.cpu().numpy() for k, v in outs[2].items()}, rows.tolist(), [cut(f, n) for f, n in zip(full, rows.tolist())], "repeat")


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_leave_the_outputs(lib, tied):
    from tf_kaldi_speaker_amd import _lib
    mats, _ = tied
    U, I, W = _lib.XV_ERR_UNSUPPORTED, _lib.XV_ERR_INVALID, _lib.XV_ERR_WORKSPACE
    s = upload([mats[0]])
    assert untouched(raw_ahc(lib, s, [65, 8193], expect=U))
    assert b"xv_ahc" in lib.xv_last_error(None) and b"8192" in lib.xv_last_error(None)
    assert untouched(raw_ahc(lib, s, [65, -1], expect=I))
    assert untouched(raw_ahc(lib, s, [65], targets=[0], expect=I))
    assert untouched(raw_ahc(lib, s, [65], threshold=float("nan"), expect=I))
    assert untouched(raw_ahc(lib, s, [65], ws_bytes=255, expect=W))
    import torch
    odd = torch.empty(264, dtype=torch.uint8, device=DEV)[4:]          # the group table holds 64-bit offsets
    assert untouched(raw_ahc(lib, s, [65], ws=odd, ws_bytes=256, expect=I)) and b"aligned" in lib.xv_last_error(None)
    rows = np.array([65, 8193], np.int32)
    assert lib.xv_ahc_workspace(2, rows.ctypes.data_as(ctypes.c_void_p)) == U          # the sibling call gives xv_ahc's code
    assert b"xv_ahc" in lib.xv_last_error(None)
    assert untouched(raw_ahc(lib, s, [], expect=0))                  # no groups: nothing is touched
    check(raw_ahc(lib, s, [65]), [65], [cut(full_log(mats[0]), 65)], "after the errors")


# ------------------------------------------------------------------------------------------------ Python surface
def _same(c, want):
    labels, count, ma, mb, mh = want
    assert np.array_equal(c.labels, labels) and c.num_clusters == count and np.array_equal(c.merge_a, ma) and np.array_equal(c.merge_b, mb)
    m = len(ma) - count if len(ma) else 0
    assert np.array_equal(c.merge_height[:m].view(np.int64), mh[:m].view(np.int64)) and np.all(np.isnan(c.merge_height[m:]))
    assert c.labels.dtype == np.int32 and c.merge_a.dtype == np.int32 and c.merge_height.dtype == np.float64


def test_python_ahc(lib, tied):
    import torch
    from tf_kaldi_speaker_amd import cluster
    mats, full = tied
    rng = np.random.default_rng(12)
    x = rng.standard_normal((40, 8)).astype(np.float32)
    m3 = (x @ x.T).astype(np.float32)
    inputs = [mats[0], torch.from_numpy(m3).to(DEV), np.zeros((1, 1), np.float32), mats[1]]
    want_full = [full[0], full_log(m3), full_log(np.zeros((1, 1), np.float32)), full[1]]
    sizes = [65, 40, 1, 300]
    for budget in (None, 1):                                         # one chunk, and a chunk per matrix: the same result
        res = cluster.ahc(inputs, budget=budget)
        assert all(isinstance(r, cluster.Clustering) for r in res)
        for r, f, n in zip(res, want_full, sizes):
            _same(r, cut(f, n))
    thr = float(full[1][2][150])
    for r, f, n, t in zip(cluster.ahc(inputs, threshold=thr, num_clusters=[1, 5, 1, 200]), want_full, sizes, [1, 5, 1, 200]):
        _same(r, cut(f, n, threshold=thr, target=t))
    for r, f, n in zip(cluster.ahc(inputs, num_clusters=3), want_full, sizes):
        _same(r, cut(f, n, target=3))
    assert cluster.ahc([]) == []
    bad = m3.copy()
    bad[30, 2] = np.inf                                              # below the diagonal: never read
    _same(cluster.ahc([bad])[0], cut(want_full[1], 40))
    bad[2, 30] = np.inf
    with pytest.raises(ValueError):
        cluster.ahc([bad])
    bad[2, 30] = np.nan
    with pytest.raises(ValueError):
        cluster.ahc([bad])
    with pytest.raises(ValueError):
        cluster.ahc([np.zeros((3, 4), np.float32)])
    with pytest.raises(ValueError, match="split the recording"):
        cluster._run([8193], None, -np.inf, None, 0)


def test_python_cosine_and_plda(lib):
    from tf_kaldi_speaker_amd import cluster, plda, scoring
    rng = np.random.default_rng(13)
    d = 16
    pm, ptm, psi = ref_plda.random_model(rng, d)
    model = plda.Plda(0.02 * pm, ptm * np.sqrt(d), psi)
    x = ref_plda.draw(rng, model.mean, model.transform, model.psi, 30, 5, 1.0)[0].astype(np.float32)         # 150 rows
    groups = np.array(["rec%d" % (i % 3) for i in range(len(x))])
    groups[7] = "solo"                                               # interleaved ids, one group of a single row
    names = sorted(set(groups.tolist()))
    mean = x.mean(axis=0)
    # cosine
    labels, per = cluster.cosine(x, groups, threshold=0.1, mean=mean)
    assert list(per) == names and labels.shape == (len(x),) and labels.dtype == np.int32
    xp = scoring.prepare(x, mean=mean)
    for name in names:
        idx = np.flatnonzero(groups == name)
        s = scoring.cosine_matrix(xp[idx], xp[idx])
        _same(per[name], ref_cluster.ahc(s, threshold=0.1))
        assert np.array_equal(labels[idx], per[name].labels)
    # PLDA, by target per group
    tg = {"rec0": 4, "rec1": 1, "rec2": 60, "solo": 2}
    labels, per = cluster.plda(model, x, groups, num_clusters=tg, normalize=False)
    for name in names:
        idx = np.flatnonzero(groups == name)
        s = plda.llr_matrix(plda.prepare_enroll(model, x[idx]), plda.prepare_test(model, x[idx]))
        _same(per[name], ref_cluster.ahc(s, target=tg[name]))
        assert np.array_equal(labels[idx], per[name].labels) and per[name].num_clusters == min(tg[name], len(idx))
    with pytest.raises(ValueError):
        cluster.cosine(x, groups[:-1])


def test_planted_clusters(lib):
    """5 centroids x 40 rows, d = 24, noise 0.3, two recordings in one call: the within-speaker and the cross-speaker cosines do
    not overlap, and a threshold between them gives back exactly the planted partition."""
    from tf_kaldi_speaker_amd import cluster, scoring
    rng = np.random.default_rng(14)
    labels_all, xs = [], []
    for _ in range(2):
        cent = rng.standard_normal((5, 24))
        spk = rng.permutation(np.repeat(np.arange(5), 40))
        xs.append((cent[spk] + 0.3 * rng.standard_normal((200, 24))).astype(np.float32))
        labels_all.append(spk)
    x, groups = np.concatenate(xs), np.repeat([0, 1], 200)
    lo_within, hi_cross = 1.0, -1.0
    for g in range(2):
        p = scoring.prepare(xs[g])
        s = scoring.cosine_matrix(p, p)
        same = labels_all[g][:, None] == labels_all[g][None, :]
        iu = np.triu(np.ones((200, 200), bool), 1)
        lo_within, hi_cross = min(lo_within, s[same & iu].min()), max(hi_cross, s[~same & iu].max())
    assert hi_cross < lo_within
    thr = 0.5 * (hi_cross + lo_within)
    labels, per = cluster.cosine(x, groups, threshold=thr)
    for g in range(2):
        got, planted = labels[groups == g], labels_all[g]
        assert per[g].num_clusters == 5
        assert np.array_equal(got[:, None] == got[None, :], planted[:, None] == planted[None, :])


# ------------------------------------------------------------------------------------------------ command line
def test_cluster_command_line(lib, repo_root, tmp_path):
    from tf_kaldi_speaker_amd import cluster, native_ark
    rng = np.random.default_rng(15)
    cent = rng.standard_normal((3, 24))
    spk = [i % 3 for i in range(30)]
    x = (cent[spk] + 0.3 * rng.standard_normal((30, 24))).astype(np.float32)
    keys = ["seg%02d" % i for i in range(30)]
    reco = ["recB" if i % 2 else "recA" for i in range(30)]
    w = native_ark.VectorWriter("ark:%s" % (tmp_path / "xvector.ark"))
    w.write(keys, x)
    w.close()
    (tmp_path / "utt2reco").write_text("".join("%s %s\n" % kv for kv in zip(keys, reco)))
    (tmp_path / "segments").write_text("".join("%s %s %.2f %.2f\n" % (k, r, 0.75 * (i // 2), 0.75 * (i // 2) + 1.5)
                                               for i, (k, r) in enumerate(zip(keys, reco))))
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.cluster", "--gpu", "0", "--threshold", "0.3", "--segments", "segments",
                        "--rttm-out", "rttm", "utt2reco", "ark:xvector.ark", "labels"], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    labels, per = cluster.cosine(x, np.array(reco), threshold=0.3)
    want = "".join("%s %d\n" % (k, l + 1) for k, l in zip(keys, labels))
    assert (tmp_path / "labels").read_text() == want
    assert [per[name].num_clusters for name in ("recA", "recB")] == [3, 3]
    assert r.stdout.strip() == "2 recordings, 30 segments, 6 clusters"
    segs = cluster.read_segments(str(tmp_path / "segments"))
    rttm = (tmp_path / "rttm").read_text()
    assert rttm == cluster.rttm_lines(segs, {k: int(l) + 1 for k, l in zip(keys, labels)}) and rttm.count("SPEAKER recA 1 ") >= 3
    # --reco2num-spk; a recording with fewer rows than speakers gets one cluster per row and a warning
    (tmp_path / "num").write_text("recA 2\nrecB 40\n")
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.cluster", "--reco2num-spk", "num", "utt2reco", "ark:xvector.ark", "-"],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "2 recordings, 30 segments, 17 clusters" and "recB" in r.stderr and "warning" in r.stderr
    got = dict(l.split() for l in lines[:-1])
    assert sorted(int(got[k]) for k, rc in zip(keys, reco) if rc == "recB") == list(range(1, 16))
    assert set(got[k] for k, rc in zip(keys, reco) if rc == "recA") == {"1", "2"}
    # a key without a recording is an error
    (tmp_path / "short").write_text("".join("%s %s\n" % kv for kv in list(zip(keys, reco))[:-1]))
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.cluster", "short", "ark:xvector.ark", "-"], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "seg29" in r.stderr


def test_extract_windows_command_line(lib, repo_root, tmp_path):
    """A synthetic checkpoint, three inputs (one too short): keys and the segments file as planned, and every window's vector is
    what Trainer.predict gives for that slice, plain and behind --cmn-window.
    The two are not the same bits: a window embedded inside a packed batch (Trainer.predict_list) and alone (Trainer.predict) are
    both f32 evaluations of the same network, but the pooling partials and the K-split of the small segment layers depend on
    where the rows lie in the batch, so sums are taken in another order.  Measured on an MI355X: largest relative difference
    1.26e-7 (plain; about one unit in the last place of the largest component).  The bound is 1e-5: the worst case of reordered
    fp32 sums of these lengths (K up to 320 per layer, seven layers: a few 1e-5 with every rounding aligned) is the scale above
    which a difference cannot come from ordering, and a wrong window or a missed CMN differs by order 1."""
    from tf_kaldi_speaker_amd import extract_windows as ew
    from tf_kaldi_speaker_amd import kaldi_io, model_io, synth
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params = dict(synth.TDNN_STAT_PARAMS, num_nodes_pooling_layer=160, num_nodes_last_layer=48)
    weights = synth.synth_weights(params, 30, seed=3, channels=64)
    model_dir = str(tmp_path / "exp")
    model_io.save_model(model_dir, params, 30, weights, step=1)
    lens = [130, 20, 61]
    utts = synth.synth_features(len(lens), lens, 30, seed=9)
    names = ["reco%d" % i for i in range(len(lens))]
    with open(str(tmp_path / "feats.ark"), "wb") as f:
        for name, u in zip(names, utts):
            kaldi_io.write_mat(f, u, key=name)
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.extract_windows", "--gpu", "0", "--window", "60", "--period", "30",
                        "--min-segment", "25", "--precision", "f32", "--node", "tdnn6_dense", "--batch-frames", "200", model_dir,
                        "ark:feats.ark", "ark:xvector.ark", "segments"], env=env, cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plan = [(name, s, e) for name, t in zip(names, lens) for s, e in ew.plan_windows(t, 60, 30, 25)]
    assert [p[1:] for p in plan] == [(0, 60), (30, 90), (60, 120), (90, 130), (0, 60), (30, 61)]
    got = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "xvector.ark")))
    assert [k for k, _ in got] == [ew.window_key(*p) for p in plan]
    assert (tmp_path / "segments").read_text() == "".join(ew.segment_line(n, s, e, 0.01) for n, s, e in plan)
    assert "reco1" in r.stderr and "skip" in r.stderr
    p = Params(**params)
    p.embedding_node = "tdnn6_dense"
    tr = Trainer(p, None, 30, single_cpu=True, device=0, precision="f32")
    tr.build("predict")
    tr.load_weights(weights)
    by_name = dict(zip(names, utts))

    def compare(vectors, feats_of, what):
        worst = 0.0
        for (key, v), (name, s, e) in zip(vectors, plan):
            want = tr.predict(feats_of[name][s:e])
            assert v.shape == want.shape, key
            worst = max(worst, float(np.linalg.norm(v - want) / np.linalg.norm(want)))
        print("extract_windows %s: largest relative difference to Trainer.predict of the slice: %.3e" % (what, worst))
        assert worst <= 1e-5, (what, worst)

    compare(got, by_name, "plain")
    # --cmn-window: the whole input is normalised first (the front-end's sliding CMN), then cut
    import torch
    from tf_kaldi_speaker_amd.frontend import cmn_select_packed
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.extract_windows", "--gpu", "0", "--window", "60", "--period", "30",
                        "--min-segment", "25", "--precision", "f32", "--node", "tdnn6_dense", "--cmn-window", "50", model_dir,
                        "ark:feats.ark", "ark:xvector_cmn.ark", "segments_cmn"], env=env, cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got_cmn = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "xvector_cmn.ark")))
    assert [k for k, _ in got_cmn] == [k for k, _ in got] and (tmp_path / "segments_cmn").read_text() == (tmp_path / "segments").read_text()
    normed = {}
    for name, u in by_name.items():
        raw = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(DEV)
        normed[name] = cmn_select_packed(raw, [0, len(u)], None, cmn_window=50, min_frames=0)[0].cpu().numpy()
    assert not np.array_equal(normed["reco0"], by_name["reco0"])
    compare(got_cmn, normed, "cmn-window 50")
    tr.close()
