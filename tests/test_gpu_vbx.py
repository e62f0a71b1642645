"""VB-HMM resegmentation on the GPU (xv_vbx, csrc/vbx.hip) through the raw C ABI and through tf_kaldi_speaker_amd.vbx, against
the float64 oracle tests/helpers/ref_vbx.py.

Shapes (ref_vbx.case: rows of a random PLDA model as speaker mean plus unit noise, speaker runs of 10 rows, a fifth of the
initial labels wrong; D = r + 3 and ldx = D + 5 throughout).  Every value that makes the kernel take another path occurs once:
  T   1 (one frame), 2 (one transition), 65, 257 (past one 256-thread stride), 600; 0 in the batch
  r   1, 7, 33 (off the 4-wide tiles), 128, 256 (with S = 64: alpha fills the 128 KiB of LDS the kernel may ask for)
  S   1, 5, 33 (past half a wave), 64 (a full wave), 12, 8
Fixed-iteration cases run epsilon = -inf with max_iters in {1, 2, 10}.  STOP is case(T=200, r=16, S=8, 3 speakers, scale 0.5,
loop_prob 0.9, seed 7): the oracle needs 9 iterations at epsilon = 1e-6, ends with 3 live speakers and min pi = 1.7e-94 (the
other five die).  In the 257- and 600-row cases pi underflows to exactly 0, so -inf runs through both passes.

Bars.  gamma, pi and every ELBO are compared with the float64 oracle within
    16 x |float64 oracle - longdouble oracle| (for that output and case) + (2 T + 2)(r + S + 8) 2^-53 max(1, max |logp|).
The first term is what an independent rounding of the same chain does to the output, with a margin of 16 that is not tuned to
the kernel; the floor is one rounding per term of the longest chain.  Every test prints its largest error / bar.
Labels must equal the oracle's wherever the oracle's two largest gamma of the row differ by more than twice the row's largest
gamma bar; at most 1 % of the rows may be excused.  Iteration counts must be equal: the early-stop epsilon is the geometric
mean of the oracle's last two improvements, asserted to be a factor 2 away from both."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import poison  # noqa: E402
import ref_plda  # noqa: E402
import ref_vbx as rv  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")

# name -> (T, r, S, speakers, scale, loop_prob, max_iters, seed)
SHAPES = collections.OrderedDict([
    ("one_frame", (1, 1, 1, 1, 1.0, 0.99, 1, 0)),
    ("one_transition", (2, 7, 5, 2, 1.0, 0.99, 2, 0)),
    ("half_wave", (65, 33, 33, 3, 1.0, 0.99, 10, 0)),
    ("lds_limit", (257, 256, 64, 4, 1.0, 0.99, 2, 0)),
    ("recording", (600, 128, 12, 4, 1.0, 0.99, 10, 0)),
])
STOP = (200, 16, 8, 3, 0.5, 0.9, 40, 7)

Case = collections.namedtuple("Case", ["x", "a", "psi", "gamma", "pi", "opts", "ref", "bar"])
_CASES = {}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    import torch
    assert torch.cuda.is_available()
    return _lib.load()


def _case(name):
    """The inputs, the float64 oracle and the bars of a case; made once and never changed."""
    if name not in _CASES:
        t_len, r, s, speakers, scale, loop, iters, seed = STOP if name == "stop" else SHAPES[name]
        x, a, psi, init, _ = rv.case(t_len, r, s, speakers, scale=scale, seed=seed)
        gamma, pi = rv.init_gamma(init, s)
        opts = dict(loop_prob=loop, max_iters=iters, epsilon=-INF)
        if name == "stop":
            first = rv.vb_hmm(x, a, psi, gamma, pi, loop_prob=loop, max_iters=iters, epsilon=1e-6)
            n = first.iters
            assert 9 <= n <= 15 and 2 <= int(np.sum(first.pi > 1e-7)) <= 3 and 1e-110 < first.pi.min() < 1e-80
            last, before = first.elbo[n - 1] - first.elbo[n - 2], first.elbo[n - 2] - first.elbo[n - 3]
            opts["epsilon"] = float(np.sqrt(last * before))
            assert 0.0 < 2.0 * last <= opts["epsilon"] and before >= 2.0 * opts["epsilon"], (last, before)
            assert np.all(np.diff(first.elbo[:n - 1]) >= 2.0 * opts["epsilon"])
        ref, bar = rv.bars(x, a, psi, gamma, pi, **opts)
        if name == "stop":
            assert ref.iters == n
        _CASES[name] = Case(x, a, psi, gamma, pi, opts, ref, bar)
    return _CASES[name]


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _padded_rows(recs, d, pad=5):
    """The rows of `recs` back to back in a [N, d + pad] buffer whose padding columns hold NaN -> (tensor, ldx, offsets)."""
    n = sum(len(x) for x in recs)
    buf = np.full((max(n, 1), d + pad), np.nan, np.float32)
    if n:
        buf[:n, :d] = np.concatenate([x for x in recs if len(x)])
    return _dev(buf), d + pad, np.concatenate([[0], np.cumsum([len(x) for x in recs])]).astype(np.int64)


def raw_vbx(lib, recs, a, psi, gammas, pis, opts, ws_bytes=None, fill=None, expect=0, row_shift=0):
    """xv_vbx through ctypes on recordings of one model -> dict of numpy outputs (gamma, pi packed).  `fill` poisons the
    workspace, labels, elbo and iters first; `row_shift` puts that many unused rows in front of the first recording."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    r, d = a.shape[0], a.shape[1] - 1
    if row_shift:
        recs = [np.full((row_shift, d), 1e30, np.float32)] + list(recs)
    xd, ldx, offsets = _padded_rows(recs, d)
    if row_shift:
        offsets = offsets[1:].copy()
    groups = len(offsets) - 1
    spk = np.array([g.shape[1] for g in gammas], np.int32)
    gd = _dev(np.concatenate([g.reshape(-1) for g in gammas] + [np.zeros(1)]), np.float64)
    pd = _dev(np.concatenate([p.reshape(-1) for p in pis] + [np.zeros(1)]), np.float64)
    iters = int(opts["max_iters"])
    need = int(lib.xv_vbx_workspace(groups, offsets.ctypes.data_as(C.c_void_p), spk.ctypes.data_as(C.c_void_p), r))
    size = (need if ws_bytes is None else ws_bytes) if need >= 0 else 0
    ws = torch.empty((max(size, 8),), dtype=torch.uint8, device=DEV)
    labels = torch.empty((int(xd.shape[0]),), dtype=torch.int32, device=DEV)
    elbo = torch.empty((max(groups, 1), iters), dtype=torch.float64, device=DEV)
    count = torch.empty((max(groups, 1),), dtype=torch.int32, device=DEV)
    for t in (ws, labels, elbo, count):
        poison.fill(t, 0xFF if fill is None else fill)
    before = [t.clone() for t in (gd, pd, labels, elbo, count)]
    ad, psid = _dev(a, np.float64), _dev(psi, np.float64)
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.xv_vbx(0, P(xd), ldx, offsets.ctypes.data_as(C.c_void_p), spk.ctypes.data_as(C.c_void_p), groups, d, P(ad), P(psid), r,
                    P(gd), P(pd), 0.3, 17.0, opts["loop_prob"], iters, opts["epsilon"], P(labels), P(elbo), P(count), P(ws), size, None)
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.xv_last_error(None))
    if expect != 0:
        assert all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(before, (gd, pd, labels, elbo, count)))
        return None
    lo, hi = int(offsets[0]), int(offsets[-1])
    return dict(gamma=gd.cpu().numpy()[:-1], pi=pd.cpu().numpy()[:-1], labels=labels.cpu().numpy()[lo:hi], elbo=elbo.cpu().numpy()[:groups],
                iters=count.cpu().numpy()[:groups], ws_need=need)


def _split(out, recs, spk):
    """Per recording: (gamma [T, S], pi, elbo row, iters, labels)."""
    res, go, po, ro = [], 0, 0, 0
    for i, (x, s) in enumerate(zip(recs, spk)):
        t = len(x)
        res.append((out["gamma"][go:go + t * s].reshape(t, s), out["pi"][po:po + s], out["elbo"][i], int(out["iters"][i]), out["labels"][ro:ro + t]))
        go, po, ro = go + t * s, po + s, ro + t
    return res


def _check(name, got, ref, bar):
    """One recording's device outputs against the oracle within the bars -> the largest error / bar of gamma, pi, elbo."""
    gamma, pi, elbo, iters, labels = got
    assert iters == ref.iters, (name, iters, ref.iters)
    assert np.all(np.isnan(elbo[iters:])) and not np.any(np.isnan(elbo[:iters])) and not np.any(np.isnan(gamma)) and not np.any(np.isnan(pi))
    ratio = dict(gamma=float(np.max(np.abs(gamma - ref.gamma) / bar["gamma"])), pi=float(np.max(np.abs(pi - ref.pi) / bar["pi"])),
                 elbo=float(np.max(np.abs(elbo[:iters] - ref.elbo[:iters]) / bar["elbo"])))
    print("%s: error / bar  gamma %.3g  pi %.3g  elbo %.3g  (iterations %d, min pi %.3g, largest gamma bar %.3g)"
          % (name, ratio["gamma"], ratio["pi"], ratio["elbo"], iters, ref.pi.min(), bar["gamma"].max()))
    assert ratio["gamma"] <= 1.0 and ratio["pi"] <= 1.0 and ratio["elbo"] <= 1.0, (name, ratio)
    assert np.array_equal(labels, np.argmax(gamma, axis=1))                                      # the lowest s among the largest
    if gamma.shape[1] > 1:
        top = np.sort(ref.gamma, axis=1)
        decided = top[:, -1] - top[:, -2] > 2.0 * bar["gamma"].max(axis=1)
        assert np.mean(~decided) <= 0.01, (name, np.mean(~decided))
        assert np.array_equal(labels[decided], ref.labels[decided]), name
    else:
        assert np.all(labels == 0)
    return ratio


# ------------------------------------------------------------------------------------------------- accuracy, raw C ABI

@pytest.mark.parametrize("name", list(SHAPES) + ["stop"])
def test_against_the_oracle(lib, name):
    c = _case(name)
    out = raw_vbx(lib, [c.x], c.a, c.psi, [c.gamma], [c.pi], c.opts)
    _check(name, _split(out, [c.x], [c.gamma.shape[1]])[0], c.ref, c.bar)
    if name == "stop":
        assert 9 <= out["iters"][0] <= 15 and out["iters"][0] < c.opts["max_iters"]


def test_tied_start_gives_label_zero(lib):
    c = _case("half_wave")
    s = 6
    gamma, pi = np.full((65, s), 1.0 / s), np.full(s, 1.0 / s)
    out = raw_vbx(lib, [c.x], c.a, c.psi, [gamma], [pi], dict(loop_prob=0.99, max_iters=1, epsilon=-INF))
    g = out["gamma"].reshape(65, s)
    assert np.all(g == g[:, :1]) and np.all(out["labels"] == 0) and np.all(out["pi"] == out["pi"][0]) and out["iters"][0] == 1


def test_dead_speakers_and_extreme_loop_probabilities(lib):
    """pi = 0 at the start: exactly 0 in gamma and pi afterwards, no NaN; loop_prob 0 and 1 are legal."""
    c = _case("one_transition")
    x, a, psi, init, _ = rv.case(65, 7, 5, 3)
    gamma, _ = rv.init_gamma(init, 5)
    pi = np.array([0.5, 0.0, 0.25, 0.0, 0.25])
    for loop in (0.99, 0.0, 1.0):
        opts = dict(loop_prob=loop, max_iters=5, epsilon=-INF)
        ref, bar = rv.bars(x, a, psi, gamma, pi, **opts)
        out = raw_vbx(lib, [x], a, psi, [gamma], [pi], opts)
        got = _split(out, [x], [5])[0]
        _check("dead speakers, loop_prob %g" % loop, got, ref, bar)
        assert np.all(got[0][:, [1, 3]] == 0.0) and np.all(got[1][[1, 3]] == 0.0)
    assert c.ref.iters == 2


# ------------------------------------------------------------------------------------------------- a batch, and purity

def _batch():
    """Five recordings of one model (r = 7, D = 10): T = 65 / S = 5, T = 0, T = 1 / S = 1, T = 257 / S = 64, T = 2 / S = 33."""
    if "batch" not in _CASES:
        rng = np.random.default_rng(77)
        a, psi = rv.draw_model(rng, 7)
        recs, gammas, pis = [], [], []
        for t_len, s, speakers in ((65, 5, 3), (0, 3, 1), (1, 1, 1), (257, 64, 4), (2, 33, 2)):
            x, init, _ = rv.draw_rows(rng, a, psi, t_len, s, speakers) if t_len else (np.zeros((0, 10), np.float32), np.zeros(0, np.int64), None)
            g, p = rv.init_gamma(init, s)
            recs.append(x), gammas.append(g), pis.append(p)
        opts = dict(loop_prob=0.95, max_iters=10, epsilon=1e-3)
        oracle = [rv.bars(x, a, psi, g, p, **opts) if len(x) else None for x, g, p in zip(recs, gammas, pis)]
        _CASES["batch"] = (a, psi, recs, gammas, pis, opts, oracle)
    return _CASES["batch"]


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_parts(u, v):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(u, v))


def _same(u, v):
    return _same_parts([u[k] for k in ("gamma", "pi", "labels", "elbo", "iters")], [v[k] for k in ("gamma", "pi", "labels", "elbo", "iters")])


def test_batch_against_the_oracle(lib):
    a, psi, recs, gammas, pis, opts, oracle = _batch()
    out = raw_vbx(lib, recs, a, psi, gammas, pis, opts)
    assert out["iters"][1] == 0 and np.all(out["elbo"][1].view(np.int64) == -1)                # T = 0 writes only iters = 0
    counts = set()
    for i, (got, o) in enumerate(zip(_split(out, recs, [g.shape[1] for g in gammas]), oracle)):
        if o is not None:
            _check("batch[%d] T %d S %d" % (i, len(recs[i]), gammas[i].shape[1]), got, o[0], o[1])
            counts.add(got[3])
    assert len(counts) > 1                                                                     # the recordings stop on their own


def test_purity(lib):
    """Bit-identical: a repeat; every recording alone against itself in the batch; the batch reversed; the least workspace
    against a larger one; three fills of the workspace and the outputs; unused rows in front of the first recording."""
    a, psi, recs, gammas, pis, opts, _ = _batch()
    spk = [g.shape[1] for g in gammas]
    base = raw_vbx(lib, recs, a, psi, gammas, pis, opts)
    assert _same(base, raw_vbx(lib, recs, a, psi, gammas, pis, opts))
    whole = _split(base, recs, spk)
    for i in range(len(recs)):
        alone = _split(raw_vbx(lib, [recs[i]], a, psi, [gammas[i]], [pis[i]], opts), [recs[i]], [spk[i]])[0]
        if len(recs[i]):
            assert _same_parts(alone, whole[i]), i
    rev = raw_vbx(lib, recs[::-1], a, psi, gammas[::-1], pis[::-1], opts)
    for u, v in zip(_split(rev, recs[::-1], spk[::-1])[::-1], whole):
        if len(u[4]):
            assert _same_parts(u, v)
    assert _same(base, raw_vbx(lib, recs, a, psi, gammas, pis, opts, ws_bytes=3 * base["ws_need"] + 8))
    for fill in poison.FILLS:
        got = raw_vbx(lib, recs, a, psi, gammas, pis, opts, fill=fill)
        got["elbo"][1] = base["elbo"][1]                       # the row of the 0-row group is not written: it keeps the fill
        assert _same(base, got), fill
    assert _same(base, raw_vbx(lib, recs, a, psi, gammas, pis, opts, row_shift=3))


def test_refusals_leave_the_outputs(lib):
    from tf_kaldi_speaker_amd import _lib
    c = _case("one_transition")
    args = ([c.x], c.a, c.psi, [c.gamma], [c.pi])
    need = raw_vbx(lib, *args, c.opts)["ws_need"]
    assert need == 256 + 8 * (2 * 9 + 3 * 10)
    raw_vbx(lib, *args, c.opts, ws_bytes=need - 1, expect=_lib.XV_ERR_WORKSPACE)
    raw_vbx(lib, *args, dict(c.opts, loop_prob=1.5), expect=_lib.XV_ERR_INVALID)
    raw_vbx(lib, *args, dict(c.opts, epsilon=float("nan")), expect=_lib.XV_ERR_INVALID)
    raw_vbx(lib, [c.x], c.a, c.psi, [np.ones((2, 65)) / 65.0], [np.ones(65) / 65.0], c.opts, expect=_lib.XV_ERR_UNSUPPORTED)
    out = raw_vbx(lib, *args, c.opts)
    _check("after the refusals", _split(out, [c.x], [5])[0], c.ref, c.bar)


# ------------------------------------------------------------------------------------------------- Python surface

def _plda_data(seed=21, d=12, recordings=(("recA", 60, 3), ("recB", 45, 2)), scale=1.0):
    """A Plda model and the rows of its recordings back to back, in time order, speaker runs of 5 rows -> (Plda args, x,
    recording ids, truth)."""
    rng = np.random.default_rng(seed)
    mean, transform, psi = ref_plda.random_model(rng, d)
    xs, ids, truth = [], [], []
    for name, t_len, speakers in recordings:
        y = scale * rng.standard_normal((speakers, d)) * np.sqrt(psi)[None, :]
        who = np.repeat(rng.permutation(np.arange((t_len + 4) // 5) % speakers), 5)[:t_len]
        u = y[who] + rng.standard_normal((t_len, d))
        xs.append((np.linalg.solve(transform, u.T).T + mean[None, :]).astype(np.float32))
        ids += [name] * t_len
        truth.append(who)
    return (mean, transform, psi), np.concatenate(xs), np.array(ids), np.concatenate(truth)


def test_python_vb_hmm_equals_the_raw_call(lib):
    from tf_kaldi_speaker_amd import plda, vbx
    (mean, transform, psi), x, ids, truth = _plda_data()
    model = plda.Plda(mean, transform, psi)
    a, p = rv.model_affine(mean, transform, psi, lda_dim=9)
    xa, xb = x[ids == "recA"], x[ids == "recB"]
    ga, pa = rv.init_gamma(truth[ids == "recA"], 4)
    gb, pb = rv.init_gamma(truth[ids == "recB"], 3)
    opts = dict(loop_prob=0.9, max_iters=6, epsilon=-INF)
    want = raw_vbx(lib, [xa, xb], a, p, [ga, gb], [pa, pb], opts)
    got = vbx.vb_hmm(model, np.concatenate([xa, xb]), [0, 60, 105], [ga, gb], [pa, pb], lda_dim=9, **opts)
    assert _same(want, dict(zip(got._fields, got)))
    packed = vbx.vb_hmm(model, np.concatenate([xa, xb]), [0, 60, 105], np.concatenate([ga.ravel(), gb.ravel()]), np.concatenate([pa, pb]),
                        num_spk=[4, 3], lda_dim=9, as_tensor=True, **opts)
    assert packed.gamma.is_cuda and _same(want, {k: v.cpu().numpy() for k, v in zip(packed._fields, packed)})
    ref, bar = rv.bars(xb, a, p, gb, pb, **opts)
    _check("vb_hmm recB", _split(want, [xa, xb], [4, 3])[1], ref, bar)
    with pytest.raises(ValueError, match="rows of dimension"):
        vbx.vb_hmm(model, np.zeros((3, 11), np.float32), [0, 3], [np.ones((3, 2))], [np.ones(2)])


def test_python_resegment(lib):
    """Initial labels are any integers; the start is softmax(5 onehot); final labels number the survivors by lowest row; a
    small budget (one recording per call) gives the same bits."""
    from tf_kaldi_speaker_amd import plda, vbx
    (mean, transform, psi), x, ids, truth = _plda_data()
    model = plda.Plda(mean, transform, psi)
    rng = np.random.default_rng(3)
    init = truth.copy()
    flip = rng.random(len(init)) < 0.2
    init[flip] = rng.integers(0, 5, int(flip.sum()))
    names = 100 - 7 * init                                            # any integers
    when = np.concatenate([np.arange(c) / float(c) for c in (60, 45)])
    shuffled = np.argsort(when, kind="stable")                        # the recordings interleaved; time order inside each is kept
    x, ids, names, truth = x[shuffled], ids[shuffled], names[shuffled], truth[shuffled]
    labels, per = vbx.resegment(model, x, ids, names, loop_prob=0.9, normalize=False)
    again, per1 = vbx.resegment(model, x, ids, names, loop_prob=0.9, normalize=False, budget=1)
    assert np.array_equal(labels, again) and list(per) == ["recA", "recB"]
    a, p = rv.model_affine(mean, transform, psi)
    for name in per:
        rows = np.where(ids == name)[0]
        lab, s = vbx.map_labels(names[rows])
        g0, pi0 = rv.init_gamma(lab, s)
        ref, bar = rv.bars(x[rows], a, p, g0, pi0, loop_prob=0.9)
        res = per[name]
        assert res.gamma.shape == (len(rows), s) and res.iterations == ref.iters and res.elbo.shape == (ref.iters,)
        _check("resegment " + name, (res.gamma, res.pi, np.concatenate([res.elbo, np.full(40 - ref.iters, np.nan)]), res.iterations,
                                     np.argmax(res.gamma, axis=1)), ref, bar)
        want, kept = vbx.map_labels(ref.labels)
        assert np.array_equal(res.labels, want) and res.num_speakers == kept and np.array_equal(labels[rows], want)
        assert res.labels[0] == 0 and np.array_equal(per1[name].gamma.view(np.int64), res.gamma.view(np.int64))
        # the planted speakers are found
        assert kept == len(set(truth[rows].tolist()))
        assert len(set(zip(res.labels.tolist(), truth[rows].tolist()))) == kept


def test_adapted_model_route(lib):
    from tf_kaldi_speaker_amd import plda, vbx
    (mean, transform, psi), x, ids, truth = _plda_data(recordings=(("recA", 60, 3),))
    model = plda.Plda(mean, transform, psi)
    adapted = plda.adapt_groups(model, x, ids, 0.7)
    ad = adapted["recA"]
    assert ad is not None and ad.dim < 12
    init = np.where(np.arange(60) % 7 == 0, 3, truth)
    labels, per = vbx.resegment(adapted, x, ids, init, loop_prob=0.9, normalize=False)
    lab, s = vbx.map_labels(init)
    g0, pi0 = rv.init_gamma(lab, s)
    ref, bar = rv.bars(x, ad.affine, ad.psi, g0, pi0, loop_prob=0.9)
    res = per["recA"]
    _check("adapted", (res.gamma, res.pi, np.concatenate([res.elbo, np.full(40 - ref.iters, np.nan)]), res.iterations, np.argmax(res.gamma, axis=1)),
           ref, bar)
    assert np.array_equal(labels, vbx.map_labels(ref.labels)[0])


def test_command_line(lib, repo_root, tmp_path):
    """vb_resegment after cluster reproduces vbx.resegment on cluster's labels, with --segments ordering and --lda-dim."""
    from tf_kaldi_speaker_amd import cluster, native_ark, plda, vbx
    from tf_kaldi_speaker_amd import vb_resegment as cmd
    (mean, transform, psi), x, ids, truth = _plda_data()
    model = plda.Plda(mean, transform, psi)
    plda.write_plda(str(tmp_path / "plda"), model)
    n = len(ids)
    rng = np.random.default_rng(9)
    archive = rng.permutation(n)                                      # the archive is not in time order: --segments restores it
    keys = ["seg%03d" % i for i in range(n)]
    start = np.zeros(n)
    for name in ("recA", "recB"):
        rows = np.where(ids == name)[0]
        start[rows] = 0.75 * np.arange(len(rows))
    w = native_ark.VectorWriter("ark:%s" % (tmp_path / "xvector.ark"))
    w.write([keys[i] for i in archive], x[archive])
    w.close()
    (tmp_path / "utt2reco").write_text("".join("%s %s\n" % (keys[i], ids[i]) for i in archive))
    (tmp_path / "segments").write_text("".join("%s %s %.2f %.2f\n" % (keys[i], ids[i], start[i], start[i] + 1.5) for i in range(n)))
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda args: subprocess.run([sys.executable, "-m"] + args, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    r = run(["tf_kaldi_speaker_amd.cluster", "--plda", "plda", "--normalize", "false", "--threshold", "-5", "utt2reco", "ark:xvector.ark", "init"])
    assert r.returncode == 0, r.stderr[-2000:]
    init = cmd.read_labels(str(tmp_path / "init"))
    for extra, kw in (([], {}), (["--lda-dim", "8", "--epsilon=-inf", "--max-iters", "7"], dict(lda_dim=8, epsilon=-INF, max_iters=7))):
        r = run(["tf_kaldi_speaker_amd.vb_resegment", "--plda", "plda", "--normalize", "false", "--loop-prob", "0.9", "--segments", "segments",
                 "--rttm-out", "rttm"] + extra + ["utt2reco", "ark:xvector.ark", "init", "labels"])
        assert r.returncode == 0, r.stderr[-2000:]
        labels, per = vbx.resegment(model, x, ids, np.array([init[k] for k in keys]), loop_prob=0.9, normalize=False, **kw)
        assert (tmp_path / "labels").read_text() == "".join("%s %d\n" % (keys[i], labels[i] + 1) for i in archive)
        before = sum(len(set(init[keys[i]] for i in np.where(ids == name)[0])) for name in per)
        assert r.stdout.strip() == "2 recordings, %d segments, %d -> %d speakers" % (n, before, sum(v.num_speakers for v in per.values()))
        segs = cluster.read_segments(str(tmp_path / "segments"))
        assert (tmp_path / "rttm").read_text() == cluster.rttm_lines(segs, {k: int(l) + 1 for k, l in zip(keys, labels)})
        assert all(1 <= v.num_speakers <= 64 for v in per.values())
    (tmp_path / "short").write_text("".join("%s %d\n" % (k, v) for k, v in list(init.items())[:-1]))
    r = run(["tf_kaldi_speaker_amd.vb_resegment", "--plda", "plda", "utt2reco", "ark:xvector.ark", "short", "-"])
    assert r.returncode == 1 and "have no entry in short" in r.stderr
