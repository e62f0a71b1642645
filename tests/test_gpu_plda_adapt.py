"""Per-recording PCA adaptation of a PLDA model on the GPU (xv_plda_adapt, csrc/plda_adapt.hip) through
tf_kaldi_speaker_amd.plda / cluster, against the float64 oracle tests/helpers/ref_plda_adapt.py.

Inputs: one batch of recordings per D (ref_plda_adapt.CASES: rows of 3 speakers drawn from a ref_plda.random_model, float32),
every batch at target_energy 0.1, 0.5, 0.9 and 1.0.

What the rule determines.  r follows from comparing cumulative energies with target_energy, and the kept subspace from the gap
between lambda_{r-1} and lambda_r, so two correct computations agree on them only where those are not decided by rounding.
ref_plda_adapt.margins measures both on the oracle's spectrum:
 * energy margin >= 1e-6 (every cumulative energy fraction is that far from target_energy): dim must equal the oracle's r;
 * also gap margin >= 1e-5 (lambda_{r-1} - lambda_r >= 1e-5 lambda_0, or r = D): the subspace is determined to ~1e-11 and the
   scores are compared against the direct-Gaussian oracle on the ORACLE's own P.
The rule keeps one direction more than the energy needs, so a recording of fewer rows than dimensions can be asked for more
directions than its covariance has (r > rank = min(n - 1, D)): the extra directions are any basis of the null space, which
Kaldi leaves to its eigensolver as this code does, and with target_energy = 1 even r is decided by the rounding of zeros.
There the checks that hold for any valid choice remain: the eigen-residuals, the model identities and the bitwise ones, and the
scores are compared against the direct-Gaussian oracle on the DEVICE's P.  tests/test_plda_adapt_host.py
(test_inputs_are_well_conditioned) asserts that both margins hold for every (recording, target_energy) with r <= rank, so that a bad seed fails loudly instead of hiding a check.

Bars.  Eigen-residuals and model identities: 8 x max(the same residual of numpy's LAPACK on the same matrix, a floor of
D 2^-53 for the eigenproblem and r cond_2(W') 2^-53 for the identities); the 8 is not derived: both methods are backward stable with constants of the same order, and a
logic error lands ten orders higher.  Every test prints max residual / bar.  Scores: the rule of
tests/test_gpu_plda.py::test_end_to_end, max(derived bar of the device's packed operands + 4 u |s|, 4 x the error of the same
chain in float32 numpy), the float32 chain run from the ORACLE's affine and psi' (steps 5-8 in numpy from P), never from
the device's, so that a wrong affine or psi' cannot widen its own bar; and the rows of the affine's linear part must lie in
the row space of P."""
import collections
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_cluster  # noqa: E402
import ref_plda  # noqa: E402
import ref_plda_adapt as ra  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EPS = 2.0 ** -53
DIMS = list(ra.CASES)

Batch = collections.namedtuple("Batch", ["d", "model", "recs", "xs", "offsets", "oracle", "device"])


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import cluster, plda
    return plda, cluster


def _device_rows(recs, d):
    import torch
    x = np.concatenate(recs) if recs else np.zeros((0, d), np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return torch.from_numpy(np.ascontiguousarray(x.reshape(-1, d))).to("cuda:0"), offsets


_BATCHES = {}


def _batch(mods, d):
    """The batch of dimension d, the oracle of every (recording, target_energy) and the device's five outputs; made once."""
    if d not in _BATCHES:
        plda, _ = mods
        mean, transform, psi, recs = ra.case(d)
        model = plda.Plda(mean, transform, psi)
        xs, offsets = _device_rows(recs, d)
        oracle = {te: [ra.adapt(mean, transform, psi, x, te) for x in recs] for te in ra.TARGET_ENERGIES}
        device = {te: plda._adapt_raw(model, xs, offsets, te) for te in ra.TARGET_ENERGIES}
        _BATCHES[d] = Batch(d, model, recs, xs, offsets, oracle, device)
    return _BATCHES[d]


def _well_determined(ad, te):
    r, energy, gap = ra.margins(ad.eigenvalues, te)
    assert r == ad.dim
    return energy >= 1e-6, energy >= 1e-6 and gap >= 1e-5


def _outputs(dev, g):
    """The specified part of the five outputs of group g."""
    dim, eigval, pca, affine, psi, _ = dev
    r = int(dim[g])
    return r, eigval[g], pca[g, :r], affine[g, :r], psi[g, :r]


@pytest.mark.parametrize("d", DIMS)
def test_dim_and_eigen_residuals(mods, d):
    b = _batch(mods, d)
    worst = dict(resid=0.0, orth=0.0, eig=0.0)
    sweeps = 0
    for te in ra.TARGET_ENERGIES:
        for g, x in enumerate(b.recs):
            r, eigval, pca, _, _ = _outputs(b.device[te], g)
            ad = b.oracle[te][g]
            if x.shape[0] < 2:
                assert r == 0
                continue
            if _well_determined(ad, te)[0]:
                assert r == ad.dim, (d, x.shape[0], te, r, ad.dim)
            assert 1 <= r <= d
            sweeps = max(sweeps, int(b.device[te][5][g, 0]))
            c = ad.cov
            cn = np.linalg.norm(c)
            lam, vrows = ra.sorted_eigh(c)
            assert np.all(np.diff(eigval) <= 0.0)

            def resid(values, rows):
                return np.linalg.norm(c @ rows.T - rows.T * values[None, :]) / cn

            def orth(rows):
                return np.max(np.abs(rows @ rows.T - np.eye(rows.shape[0])))

            floor = d * EPS
            ratios = dict(resid=resid(eigval[:r], pca) / (8 * max(resid(lam[:r], vrows[:r]), floor)),
                          orth=orth(pca) / (8 * max(orth(vrows[:r]), floor)),
                          eig=np.max(np.abs(eigval - lam)) / cn / (8 * floor))
            for k, v in ratios.items():
                worst[k] = max(worst[k], v)
                assert v <= 1.0, (d, x.shape[0], te, k, v)
            # the sign rule
            j = np.argmax(np.abs(pca), axis=1)
            assert np.all(pca[np.arange(r), j] > 0.0)
    print("D %d: max residual / bar: eigen-residual %.3f, orthogonality %.3f, eigenvalues %.3f; at most %d sweeps"
          % (d, worst["resid"], worst["orth"], worst["eig"], sweeps))


@pytest.mark.parametrize("d", DIMS)
def test_model_identities(mods, d):
    b = _batch(mods, d)
    ainv = np.linalg.inv(b.model.transform)
    worst = dict(within=0.0, between=0.0, offset=0.0)
    sweeps = 0
    for te in ra.TARGET_ENERGIES:
        for g, x in enumerate(b.recs):
            r, _, pca, affine, psi2 = _outputs(b.device[te], g)
            if r == 0:
                continue
            sweeps = max(sweeps, int(b.device[te][5][g, 1]))
            ad = b.oracle[te][g]

            def identities(p, aff, ps):
                # A' W' A'^T = (A' P) A^-1 A^-T (A' P)^T with A' P the linear part of the affine: no A' has to be recovered
                # through P^T, which would add the orthogonality error of P (checked on its own above) to the identity
                m = p @ ainv
                t = aff[:, :-1] @ ainv
                return (np.max(np.abs(t @ t.T - np.eye(len(ps)))), np.max(np.abs((t * b.model.psi[None, :]) @ t.T - np.diag(ps))) / ps[0],
                        np.linalg.cond(m @ m.T))

            within, between, cond = identities(pca, affine, psi2)
            o_within, o_between, _ = identities(ad.pca, ad.affine, ad.psi)
            floor = r * cond * EPS
            ratios = dict(within=within / (8 * max(o_within, floor)), between=between / (8 * max(o_between, floor)))
            assert np.all(np.diff(psi2) <= 0.0) and np.all(psi2 >= 0.0)
            ap = np.abs(affine[:, :-1])
            off_bar = (d + r + 4) * EPS * (ap @ np.abs(b.model.mean))
            off_err = np.abs(affine[:, -1] + affine[:, :-1] @ b.model.mean)
            ratios["offset"] = float(np.max(off_err / off_bar))
            for k, v in ratios.items():
                worst[k] = max(worst[k], v)
                assert v <= 1.0, (d, x.shape[0], te, k, v)
            j = np.argmax(np.abs(affine), axis=1)
            assert np.all(affine[np.arange(r), j] > 0.0)
    print("D %d: max residual / bar: A' W' A'^T - I %.3f, A' B' A'^T - diag(psi') %.3f, offset column %.3f; at most %d sweeps"
          % (d, worst["within"], worst["between"], worst["offset"], sweeps))


def test_fallbacks(mods):
    """No rows, one row, identical rows: dim 0; eigval is written for the identical rows (zeros); the Python layer returns None
    and warns once with the count."""
    plda, _ = mods
    b = _batch(mods, 7)
    for te in ra.TARGET_ENERGIES:
        assert list(b.device[te][0][:2]) == [0, 0] and np.all(b.device[te][0][2:] > 0)
    same = np.tile((np.arange(7, dtype=np.float32) - 3) / 3, (6, 1))
    recs = [b.recs[5], same, b.recs[1], b.recs[4]]
    xs, offsets = _device_rows(recs, 7)
    dim, eigval, _, _, _, _ = plda._adapt_raw(b.model, xs, offsets, 0.5)
    assert dim[1] == 0 and dim[2] == 0 and dim[0] == b.device[0.5][0][5] and dim[3] == b.device[0.5][0][4]
    assert np.all(eigval[1] == 0.0)
    groups = np.repeat(["a", "b", "c", "d"], [len(r) for r in recs])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = plda.adapt_groups(b.model, np.concatenate(recs), groups, 0.5)
    mine = [str(w.message) for w in seen if "could not be adapted" in str(w.message)]
    assert len(mine) == 1 and "2 of 4 groups" in mine[0]
    assert list(got) == ["a", "b", "c", "d"] and got["b"] is None and got["c"] is None
    ad = got["a"]
    r, eig, pca, affine, psi2 = _outputs(b.device[0.5], 5)
    assert ad.dim == r and ad.in_dim == 7 and ad.pca.tobytes() == pca.tobytes() and ad.affine.tobytes() == affine.tobytes()
    assert ad.psi.tobytes() == psi2.tobytes() and ad.eigenvalues.tobytes() == eig.tobytes()
    with pytest.raises(ValueError):
        plda.adapt_groups(b.model, np.concatenate(recs), groups, 0.0)
    with pytest.raises(ValueError):
        plda.adapt_groups(b.model, np.concatenate(recs), groups[:-1], 0.5)


@pytest.mark.parametrize("d", [7, 33, 150])
def test_same_bits_alone_in_any_batch_and_workspace(mods, d):
    """All five outputs of a group: alone, in the batch, in the reversed batch, at the least and at twice the least workspace,
    on a repeat.  d = 150 keeps its matrices in the workspace, 7 and 33 in LDS."""
    plda, _ = mods
    from tf_kaldi_speaker_amd import _lib
    b = _batch(mods, d)
    te = 0.5
    base = b.device[te]
    least = int(_lib.load().xv_plda_adapt_workspace(len(b.recs), d))

    def same(dev, g, h):
        for p, q in zip(_outputs(dev, h), _outputs(base, g)):
            assert np.asarray(p).tobytes() == np.asarray(q).tobytes(), (d, g)

    for variant in (dict(), dict(ws_bytes=least), dict(ws_bytes=2 * least)):
        dev = plda._adapt_raw(b.model, b.xs, b.offsets, te, **variant)
        for g in range(len(b.recs)):
            same(dev, g, g)
    xs, offsets = _device_rows(b.recs[::-1], d)
    dev = plda._adapt_raw(b.model, xs, offsets, te)
    for g in range(len(b.recs)):
        same(dev, g, len(b.recs) - 1 - g)
    for g in range(len(b.recs)):
        xs, offsets = _device_rows([b.recs[g]], d)
        same(plda._adapt_raw(b.model, xs, offsets, te), g, 0)
    with pytest.raises(_lib.XvError) as ex:
        plda._adapt_raw(b.model, b.xs, b.offsets, te, ws_bytes=least - 8)
    assert ex.value.code == _lib.XV_ERR_WORKSPACE


def test_argument_errors_leave_the_outputs(mods):
    import ctypes as C
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    b = _batch(mods, 7)
    g, d = len(b.recs), 7
    p = lambda t: C.c_void_p(t.data_ptr())             # noqa: E731
    dbl = lambda *s: torch.full(s, -7.5, dtype=torch.float64, device="cuda:0")             # noqa: E731
    dim = torch.full((g,), -7, dtype=torch.int32, device="cuda:0")
    eig, pca, aff, psi = dbl(g, d), dbl(g, d, d), dbl(g, d, d + 1), dbl(g, d)
    vec, mat = dbl(d), dbl(d, d)
    need = int(lib.xv_plda_adapt_workspace(g, d))
    ws = torch.zeros((need + 8,), dtype=torch.uint8, device="cuda:0")

    def call(off=b.offsets, te=0.5, wsp=p(ws), size=need, dd=d):
        off = np.ascontiguousarray(off, np.int64)
        return lib.xv_plda_adapt(0, p(b.xs), d, off.ctypes.data_as(C.c_void_p), g, dd, p(vec), p(mat), p(vec), te, p(dim), p(eig),
                                 p(pca), p(aff), p(psi), wsp, size, None)

    bad = b.offsets.copy()
    bad[2] = bad[1] - 1
    assert call(off=bad) == _lib.XV_ERR_INVALID and call(te=float("nan")) == _lib.XV_ERR_INVALID and call(te=1.5) == _lib.XV_ERR_INVALID
    assert call(size=need - 1) == _lib.XV_ERR_WORKSPACE and call(wsp=C.c_void_p(ws.data_ptr() + 4)) == _lib.XV_ERR_INVALID
    assert call(dd=257) == _lib.XV_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((dim == -7).all()) and all(bool((t == -7.5).all()) for t in (eig, pca, aff, psi))


def _f32_scores(ad_affine, ad_psi, x):
    """The chain of prepare_enroll / prepare_test in plain float32 numpy (the affine rounded once, applied to [x; 1], the
    length normalisation of TransformIvector with one utterance), scored by the float64 oracle from those rows."""
    t = ad_affine.astype(np.float32)
    u = x.astype(np.float32) @ t[:, :-1].T + t[:, -1][None, :]
    inv = (1.0 / (ad_psi + 1.0)).astype(np.float32)
    ss = np.sum(u * u * inv[None, :], axis=1, dtype=np.float32)
    y = u * np.where(ss > 0, np.sqrt(np.float32(u.shape[1]) / np.where(ss > 0, ss, np.float32(1))), np.float32(0))[:, None]
    return ref_plda.llr(ad_psi, y, 1, y)


@pytest.mark.parametrize("d", DIMS)
def test_scores_end_to_end(mods, d):
    """cluster.plda_matrices(target_energy) against the direct-Gaussian oracle in float64; a recording's matrix is bit for bit
    plda.llr_matrix of its rows prepared with its adapted model, a fallback recording's is the global model's; the labels are
    ref_cluster's AHC of the device's own matrices."""
    plda, cluster = mods
    b = _batch(mods, d)
    recs = [x for x in b.recs if x.shape[0] > 0]
    idx = [g for g, x in enumerate(b.recs) if x.shape[0] > 0]
    names = ["rec%02d" % g for g in idx]
    x = np.concatenate(recs)
    groups = np.repeat(names, [len(r) for r in recs])
    # shuffle the rows of different recordings among each other without changing the order inside a recording
    slots = np.random.default_rng(7).permutation(len(x))
    mixed = np.empty(len(x), np.int64)
    for n in names:
        mine = np.flatnonzero(groups == n)
        mixed[np.sort(slots[mine])] = mine
    xm, gm = x[mixed], groups[mixed]
    front = dict(normalize=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = cluster.plda_matrices(b.model, xm, gm, **front)
    worst, worst_leak = 0.0, 0.0
    for te in ra.TARGET_ENERGIES:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            mats = cluster.plda_matrices(b.model, xm, gm, target_energy=te, **front)
            labels, per = cluster.plda(b.model, xm, gm, threshold=0.0, target_energy=te, **front)
        assert list(mats) == names
        for g, name, xg in zip(idx, names, recs):
            got = mats[name]
            assert got.shape == (len(xg), len(xg)) and got.dtype == np.float32 and np.all(np.isfinite(got))
            r, _, pca, affine, psi2 = _outputs(b.device[te], g)
            want_labels = ref_cluster.ahc(got, threshold=0.0)
            assert np.array_equal(per[name].labels, want_labels[0]) and per[name].num_clusters == want_labels[1]
            assert np.array_equal(labels[gm == name], per[name].labels)
            if r == 0:
                assert got.tobytes() == plain[name].tobytes()
                continue
            model_g = plda.AdaptedPlda(pca, affine, psi2, None)
            e, t = plda.prepare_enroll(model_g, xg, device=0), plda.prepare_test(model_g, xg, device=0)
            assert plda.llr_matrix(e, t).tobytes() == got.tobytes()
            ad = b.oracle[te][g]
            # the kept subspace ties the affine to P: the rows of A' P lie in the row space of P.  ||T (I - P^T P)||_F <=
            # ||A'||_F ||I - P P^T||_2 with ||I - P P^T||_2 <= r max|P P^T - I| <= r 8 D 2^-53 (the orthogonality bar of
            # test_dim_and_eigen_residuals), plus the rounding of the product A' P, (r + D) 2^-53 ||A'||_F; ||A'||_F = ||T||_F (1 + small)
            lin = affine[:, :-1]
            leak = np.linalg.norm(lin - (lin @ pca.T) @ pca) / ((8 * r * d + r + d) * 1.01 * EPS * np.linalg.norm(lin))
            worst_leak = max(worst_leak, float(leak))
            assert leak <= 1.0, (d, len(xg), te, r, float(leak))
            # the oracle and the float32 chain never see the device's affine or psi': both start from P (the oracle's own
            # where the rule determines the subspace, the device's elsewhere) and run steps 5-9 in numpy
            p_ref = ad.pca if _well_determined(ad, te)[1] else pca
            ref_affine, ref_psi, _, _ = ra.model_from_p(b.model.mean, b.model.transform, b.model.psi, p_ref)
            want = ra.llr_direct(b.model.mean, b.model.transform, b.model.psi, p_ref, xg)
            f32_err = np.max(np.abs(_f32_scores(ref_affine, ref_psi, xg) - want))
            _, dot_bar, bias_bar = ref_plda.score_bar(e.packed.cpu().numpy()[:, :e.k], t.packed.cpu().numpy()[:, :e.k],
                                                      e.bias.cpu().numpy(), t.tau(1).cpu().numpy())
            bar = np.maximum(dot_bar + bias_bar + 4 * U * np.abs(want), 4 * f32_err)
            err = np.abs(got - want)
            worst = max(worst, float(np.max(err / bar)))
            assert np.all(err <= bar), (d, len(xg), te, r, float(np.max(err / bar)), float(err.max()), f32_err)
    print("D %d: scores against the direct-Gaussian oracle, max error / bar %.3f; affine outside the row space of P / bar %.3f"
          % (d, worst, worst_leak))
    # without the option nothing changes: today's matrix, from the global model
    name, xg = names[-1], recs[-1]
    e, t = plda.prepare_enroll(b.model, xg), plda.prepare_test(b.model, xg)
    assert plda.llr_matrix(e, t).tobytes() == plain[name].tobytes()


def test_command_line(mods, repo_root, tmp_path):
    plda, cluster = mods
    from tf_kaldi_speaker_amd import native_ark
    b = _batch(mods, 33)
    recs = b.recs
    x = np.concatenate(recs)
    keys = ["seg%03d" % i for i in range(len(x))]
    reco = np.repeat(["rec%d" % g for g in range(len(recs))], [len(r) for r in recs])
    w = native_ark.VectorWriter("ark:%s" % (tmp_path / "xvector.ark"))
    w.write(keys, x)
    w.close()
    (tmp_path / "utt2reco").write_text("".join("%s %s\n" % kv for kv in zip(keys, reco)))
    plda.write_plda(str(tmp_path / "plda"), b.model)
    env = dict(os.environ, PYTHONPATH=repo_root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.cluster", "--gpu", "0", "--plda", "plda", "--normalize", "false",
                        "--target-energy", "0.5", "utt2reco", "ark:xvector.ark", "labels"], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    labels, per = cluster.plda(b.model, x, reco, threshold=0.0, normalize=False, target_energy=0.5)
    assert (tmp_path / "labels").read_text() == cluster.format_labels(keys, labels)
    plain, _ = cluster.plda(b.model, x, reco, threshold=0.0, normalize=False)
    print("labels that differ from the global model's: %d of %d" % (int(np.sum(plain != labels)), len(labels)))
    assert r.stdout.strip() == "%d recordings, %d segments, %d clusters" % (len(recs), len(x), sum(c.num_clusters for c in per.values()))
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.cluster", "--target-energy", "0.5", "utt2reco", "ark:xvector.ark", "-"],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "needs --plda" in r.stderr
