"""Host side of back-end training (tf_kaldi_speaker_amd.backend: lda_from_stats, plda_from_stats, global_mean, the argument
checks of the commands), without a GPU: the statistics are built in numpy (tests/helpers/ref_backend.numpy_stats) and the
results compared with tests/helpers/ref_backend.py, a float64 transcription of the Kaldi loops that accumulates speaker by
speaker and runs the EM class by class.

The bar.  Both sides are float64 over the same numbers in a different order, so they differ by rounding amplified through two
eigendecompositions; the amplification depends on the eigen-gaps and has no closed form.  It was measured on the inputs of
this file (d = 12, 60 speakers of 1..9 utterances): the largest relative difference of any compared quantity, oracle or
invariant, is 3.3e-14 (MEASURED below; profiles/backend.md).  The bar is 100 x that and no looser than 1e-8: BAR = 3.3e-12.
Every test prints what it measures."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_backend  # noqa: E402
import ref_plda  # noqa: E402

from tf_kaldi_speaker_amd import backend, kaldi_io, plda, scoring  # noqa: E402

MEASURED = 3.3e-14
BAR = min(100.0 * MEASURED, 1e-8)
D, SPEAKERS, LDA_DIM = 12, 60, 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    """Largest difference of two arrays relative to the largest magnitude of the second."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _draw(seed, per=None):
    """ref_plda.draw with 1..9 utterances per speaker (speakers 0..5 have exactly one), or `per` for all."""
    rng = np.random.default_rng(seed)
    mean, transform, psi = ref_plda.random_model(rng, D)
    x, labels = ref_plda.draw(rng, mean, transform, psi, SPEAKERS, 9 if per is None else per)
    if per is None:
        keep_n = rng.integers(1, 10, SPEAKERS)
        keep_n[:6] = 1
        keep = np.concatenate([np.flatnonzero(labels == s)[:keep_n[s]] for s in range(SPEAKERS)])
        keep = keep[rng.permutation(keep.shape[0])]            # rows of one speaker are not adjacent
        x, labels = x[keep], labels[keep]
    return x, labels


def _stats(x, labels, center=None):
    return backend.Stats(**ref_backend.numpy_stats(x, labels, center))


@pytest.fixture(scope="module")
def data():
    x, labels = _draw(11)
    assert np.sum(np.bincount(labels) == 1) >= 6 and np.bincount(labels).max() <= 9
    return x, labels, _stats(x, labels)


@pytest.fixture(scope="module")
def oracle(data):
    x, labels, _ = data
    return ref_backend.lda(x, labels, LDA_DIM), ref_backend.plda(x, labels, 10)


@pytest.mark.parametrize("centre", ["mean", "zero", "far"])
def test_lda_against_the_oracle(data, oracle, centre):
    """A^T A and ||A mu + offset|| (sign-invariant) against ivector-compute-lda.cc as loops; the same from statistics taken
    about another centre (Stats.about_mean recentres them).  Measured: 1.7e-14 (mean), 3.2e-14 (zero), 3.3e-14 (far)."""
    x, labels, stats = data
    if centre != "mean":
        stats = _stats(x, labels, np.zeros(D) if centre == "zero" else x.mean(axis=0) + 3.0)
    got = backend.lda_from_stats(stats, dim=LDA_DIM).astype(np.float64)
    want = oracle[0]
    assert got.shape == (LDA_DIM, D + 1)
    a, w = got[:, :D], want[:, :D]
    a64 = backend.lda_float64(stats, dim=LDA_DIM)            # the file is float32: the oracle bar is for the float64 matrix
    e1 = rel(a64[:, :D].T @ a64[:, :D], w.T @ w)
    mu = x.mean(axis=0)
    e2 = float(np.linalg.norm(a64[:, :D] @ mu + a64[:, D])) / float(np.linalg.norm(w @ mu))
    e3 = rel(a.T @ a, w.T @ w)
    print("lda (%s): A^T A rel %.3e, offset residue rel %.3e, float32 file rel %.3e; bar %.1e" % (centre, e1, e2, e3, BAR))
    assert e1 <= BAR and e2 <= BAR
    assert e3 <= 4 * 2.0 ** -24            # the cast: two float32 roundings per product, relative to the largest entry


def test_lda_invariants(data):
    """A within A^T = I and A between A^T diagonal and descending (f = 0), from the rows themselves.  Measured: 3.1e-15."""
    x, labels, stats = data
    a = backend.lda_float64(stats, dim=LDA_DIM)[:, :D]
    y = x - x.mean(axis=0)
    counts = np.bincount(labels)
    means = np.stack([y[labels == s].mean(axis=0) for s in range(SPEAKERS)])
    between = (means * counts[:, None]).T @ means / y.shape[0]
    within = y.T @ y / y.shape[0] - between
    wi = a @ within @ a.T
    bi = a @ between @ a.T
    e1 = float(np.max(np.abs(wi - np.eye(LDA_DIM))))
    off = bi - np.diag(np.diag(bi))
    e2 = float(np.max(np.abs(off))) / float(np.max(np.abs(bi)))
    print("lda invariants: |A W A^T - I| %.3e, off-diagonal of A B A^T rel %.3e; bar %.1e" % (e1, e2, BAR))
    assert e1 <= BAR and e2 <= BAR
    assert np.all(np.diff(np.diag(bi)) <= BAR * np.max(np.diag(bi)))


def test_plda_against_the_oracle(data, oracle):
    """psi, mean and transform^T diag(.) transform against plda.cc as loops (class by class).  Measured: 1.1e-14."""
    _, _, stats = data
    got, want = backend.plda_from_stats(stats, 10), oracle[1]
    t, tw = got.transform, want["transform"]
    errs = dict(psi=rel(got.psi, want["psi"]), mean=rel(got.mean, want["mean"]),
                tt=rel(t.T @ t, tw.T @ tw), tpt=rel(t.T @ (got.psi[:, None] * t), tw.T @ (want["psi"][:, None] * tw)),
                w=rel(got.within_var, want["within_var"]), b=rel(got.between_var, want["between_var"]))
    print("plda: " + ", ".join("%s rel %.3e" % kv for kv in sorted(errs.items())) + "; bar %.1e" % BAR)
    assert max(errs.values()) <= BAR


def test_plda_invariants(data):
    """transform W transform^T = I, transform B transform^T = diag(psi) for the last W, B of the EM; psi >= 0, descending.
    Measured: 1.0e-15."""
    _, _, stats = data
    m = backend.plda_from_stats(stats, 10)
    e1 = float(np.max(np.abs(m.transform @ m.within_var @ m.transform.T - np.eye(D))))
    e2 = float(np.max(np.abs(m.transform @ m.between_var @ m.transform.T - np.diag(m.psi)))) / float(m.psi.max())
    print("plda invariants: |T W T^T - I| %.3e, |T B T^T - diag(psi)| rel %.3e; bar %.1e" % (e1, e2, BAR))
    assert e1 <= BAR and e2 <= BAR
    assert np.all(m.psi >= 0.0) and np.all(np.diff(m.psi) <= 0.0)


def test_plda_offset_scatter_does_not_depend_on_the_centre(data):
    x, labels, stats = data
    far = _stats(x, labels, x.mean(axis=0) + 3.0)
    a, b = backend.plda_from_stats(stats, 10), backend.plda_from_stats(far, 10)
    e = max(rel(a.psi, b.psi), rel(a.within_var, b.within_var))
    print("plda about a centre 3 away: rel %.3e; bar %.1e" % (e, BAR))
    assert e <= BAR


def test_em_fixed_point():
    """All n_s equal (n = 4), 50 iterations: one more iteration moves W and B by less than the bar, and the point reached is
    the closed form of equal n: W = offset_scatter / (N - S), B = (1 / S) sum_s m m^T - W / n.

    The EM contracts a direction of between-class variance psi (within-class 1) by about 1 / (1 + n psi) per iteration, the
    share of the class mean that the data leave undetermined.  Fifty iterations reach a double-precision fixed point only
    where n psi is not small, so this draw sets psi log-spaced in 2..50 (n psi >= 8: a factor of at most 1/9 per iteration);
    the psi of ref_plda.random_model go down to 1e-3, where the factor is 0.996 and iteration 51 still moves W by 6e-5.
    Measured here: iteration 51 moves W, B by 2.8e-16; closed form within 4.3e-16."""
    rng = np.random.default_rng(12)
    mean, transform, _ = ref_plda.random_model(rng, D)
    psi = np.exp(np.linspace(np.log(50.0), np.log(2.0), D))
    per = 4
    x, labels = ref_plda.draw(rng, mean, transform, psi, SPEAKERS, per)
    stats = _stats(x, labels)
    a, b = backend.plda_from_stats(stats, 50), backend.plda_from_stats(stats, 51)
    e = max(rel(b.within_var, a.within_var), rel(b.between_var, a.between_var))
    centred = stats.means - stats.means.mean(axis=0)
    w_closed = (stats.total - stats.between) / float(stats.n - SPEAKERS)
    b_closed = centred.T @ centred / SPEAKERS - w_closed / per
    assert np.linalg.eigvalsh(b_closed).min() > 0.0            # otherwise the EM's fixed point is on the boundary, not this one
    e2 = max(rel(a.within_var, w_closed), rel(a.between_var, b_closed))
    print("EM fixed point: iteration 51 moves W, B by rel %.3e, closed form rel %.3e; bar %.1e" % (e, e2, BAR))
    assert e <= BAR and e2 <= BAR
    want = ref_backend.plda(x, labels, 50)
    assert max(rel(a.within_var, want["within_var"]), rel(a.between_var, want["between_var"])) <= BAR


def test_round_trip(tmp_path, data):
    _, _, stats = data
    m = backend.plda_from_stats(stats, 3)
    for binary in (True, False):
        path = str(tmp_path / ("plda_%d" % binary))
        plda.write_plda(path, m, binary=binary)
        back = plda.read_plda(path)
        assert np.array_equal(back.mean, m.mean) and np.array_equal(back.transform, m.transform) and np.array_equal(back.psi, m.psi)
    lda = backend.lda_from_stats(stats, dim=LDA_DIM)
    path = str(tmp_path / "transform.mat")
    kaldi_io.write_mat(path, lda)
    back = kaldi_io.read_mat(path)
    assert back.dtype == np.float32 and np.array_equal(back, lda)
    assert scoring.check_transform(D, back.shape) == (LDA_DIM, D + 1)
    mean = backend.global_mean(data[0].astype(np.float32))
    path = str(tmp_path / "mean.vec")
    kaldi_io.write_vec_flt(path, mean)
    assert mean.dtype == np.float32 and np.array_equal(kaldi_io.read_vec_flt(path), mean)
    assert np.array_equal(mean, (data[0].astype(np.float32).astype(np.float64).sum(axis=0) / data[0].shape[0]).astype(np.float32))


def test_arguments(data):
    x, labels, stats = data
    with pytest.raises(ValueError):
        backend.lda_from_stats(stats, dim=D + 1)
    with pytest.raises(ValueError):
        backend.lda_from_stats(stats, dim=0)
    with pytest.raises(ValueError):
        backend.lda_from_stats(stats, dim=3, total_covariance_factor=1.5)
    with pytest.raises(ValueError):
        backend.plda_from_stats(stats, -1)
    with pytest.raises(ValueError):
        backend.global_mean(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError):                       # an empty class list
        backend.class_lists((np.array([0]), np.array([], np.int64)), 5)
    with pytest.raises(ValueError):
        backend.class_lists((np.array([0, 0, 0]), np.array([], np.int64)), 5)
    with pytest.raises(ValueError):                       # mismatched lengths
        backend.class_lists(np.arange(4), 5)
    with pytest.raises(ValueError):
        backend.class_lists((np.array([0, 2]), np.array([0, 1, 2])), 5)
    with pytest.raises(ValueError):                       # a row number out of range
        backend.class_lists((np.array([0, 2]), np.array([0, 5])), 5)
    with pytest.raises(ValueError):
        backend.scatter_stats(np.zeros((5, 3), np.float32), np.arange(4))
    with pytest.raises(ValueError):
        backend.scatter_stats(np.zeros((5, 3), np.float32), np.arange(5), center=np.zeros(4))
    with pytest.raises(ValueError):
        backend.Stats(np.array([2.0]), np.zeros((2, 3)), np.zeros(3), np.zeros(3), np.zeros((3, 3)), np.zeros((3, 3)))
    off, idx = backend.class_lists(np.array([7, 3, 7, 3, 9]), 5)
    assert off.tolist() == [0, 2, 4, 5] and idx.tolist() == [1, 3, 0, 2, 4]
    off, idx = backend.class_lists((np.array([0, 2, 2, 3]), np.array([4, 0, 2])), 5)      # the empty class is dropped
    assert off.tolist() == [0, 2, 3] and idx.tolist() == [4, 0, 2]


@pytest.mark.parametrize("module,argv", [("compute_mean", ["a"]), ("compute_mean", ["a", "b", "c"]),
                                         ("compute_lda", ["a", "b"]), ("compute_lda", ["a", "b", "c", "d"]),
                                         ("compute_plda", ["a", "b"]), ("compute_plda", ["--num-em-iters", "-1", "a", "b", "c"])])
def test_cli_argument_counts(module, argv):
    """A wrong number of positional arguments (or a bad option) ends the command with a non-zero status before it reads
    anything."""
    import importlib
    mod = importlib.import_module("tf_kaldi_speaker_amd." + module)
    with pytest.raises(SystemExit) as ex:
        mod.main(argv)
    assert ex.value.code not in (0, None)


def test_cli_as_a_process(tmp_path):
    """compute_mean end to end on the host, as a child process: table in, Kaldi vector out; no argument -> non-zero exit."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((9, 5)).astype(np.float32)
    ark = str(tmp_path / "x.ark")
    with open(ark, "wb") as f:
        for i in range(9):
            kaldi_io.write_vec_flt(f, x[i], key="utt%d" % i)
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = str(tmp_path / "mean.vec")
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.compute_mean", "ark:" + ark, out], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(kaldi_io.read_vec_flt(out), backend.global_mean(x))
    r = subprocess.run([sys.executable, "-m", "tf_kaldi_speaker_amd.compute_mean"], env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0
