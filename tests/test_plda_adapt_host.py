"""Host side of the per-recording PLDA adaptation (xv_plda_adapt, csrc/plda_adapt.hip): the oracle against itself, the energy
rule, the declarations, the argument checks of the C entry point (which come before any HIP call, so they answer on a machine
without a GPU) and the command line."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_plda  # noqa: E402
import ref_plda_adapt as ra  # noqa: E402


@pytest.mark.parametrize("d", list(ra.CASES))
def test_the_two_oracle_forms_agree(d):
    """Chain 1-9 with eigh / cholesky against the log likelihood ratio of the projected Gaussian model without any
    diagonalisation, on the inputs of tests/test_gpu_plda_adapt.py: within 1e-9 (1 + |s|)."""
    mean, transform, psi, recs = ra.case(d)
    worst = 0.0
    for x in recs:
        for te in ra.TARGET_ENERGIES:
            ad = ra.adapt(mean, transform, psi, x, te)
            if x.shape[0] < 2:
                assert ad is None
                continue
            a = ra.llr_adapted(ad, x)
            b = ra.llr_direct(mean, transform, psi, ad.pca, x)
            rel = np.max(np.abs(a - b) / (1.0 + np.abs(b)))
            worst = max(worst, rel)
            assert rel <= 1e-9, (d, x.shape[0], te, rel)
            # the adapted model is a model: within-class covariance I, between-class diag(psi')
            a2 = ad.affine[:, :-1] @ ad.pca.T
            assert np.max(np.abs(a2 @ ad.w_proj @ a2.T - np.eye(ad.dim))) <= 1e-10
    print("D %d: the two forms agree to %.2e (1 + |s|)" % (d, worst))


@pytest.mark.parametrize("d", list(ra.CASES))
def test_inputs_are_well_conditioned(d):
    mean, transform, psi, recs = ra.case(d)
    low_e, low_g = np.inf, np.inf
    for x in recs:
        if x.shape[0] < 2:
            continue
        rank = min(x.shape[0] - 1, d)
        for te in ra.TARGET_ENERGIES:
            ad = ra.adapt(mean, transform, psi, x, te)
            r, energy, gap = ra.margins(ad.eigenvalues, te)
            if r <= rank:
                low_e, low_g = min(low_e, energy), min(low_g, gap)
                assert energy >= 1e-6 and gap >= 1e-5, (d, x.shape[0], te, r, energy, gap)
    print("D %d: smallest energy margin %.2e, smallest gap margin %.2e over the recordings with r <= rank" % (d, low_e, low_g))
    assert np.isfinite(low_e)


def test_energy_rule():
    lam = np.array([4.0, 3.0, 2.0, 1.0])                     # fractions 0.4, 0.7, 0.9, 1.0
    assert ra.energy_dim(lam, 0.1) == 2                      # k = 1, plus one
    assert ra.energy_dim(lam, 0.4) == 3                      # 0.4 is not > 0.4: k = 2
    assert ra.energy_dim(lam, 0.5) == 3
    assert ra.energy_dim(lam, 0.75) == 4                     # k = 3, plus one
    assert ra.energy_dim(lam, 0.95) == 4                     # k = 4: the cap at D
    assert ra.energy_dim(lam, 1.0) == 4                      # no k: D
    assert ra.energy_dim(np.array([2.5]), 0.1) == 1 and ra.energy_dim(np.array([2.5]), 1.0) == 1       # D = 1
    assert ra.energy_dim(np.array([1.0, 0.0, 0.0]), 0.9) == 2
    assert ra.margins(lam, 0.5) == (3, pytest.approx(0.1), pytest.approx(0.25))
    assert ra.margins(lam, 1.0)[1] == pytest.approx(0.1)     # the last fraction does not count against target_energy = 1
    rows = ra.fix_signs([[1.0, -2.0, 2.0], [0.5, 0.25, -0.125], [-3.0, 3.0, 0.0]])
    assert np.array_equal(rows, [[-1.0, 2.0, -2.0], [0.5, 0.25, -0.125], [3.0, -3.0, 0.0]])


def test_fallback_groups_of_the_oracle():
    mean, transform, psi, _ = ra.case(7)
    x = np.tile(np.arange(7, dtype=np.float32), (5, 1))
    assert ra.adapt(mean, transform, psi, x, 0.5) is None            # identical rows: no variance
    assert ra.adapt(mean, transform, psi, x[:1], 0.5) is None and ra.adapt(mean, transform, psi, x[:0], 0.5) is None


def test_symbols_declared_listed_and_built(repo_root):
    import __graft_entry__ as g
    assert "plda_adapt.hip" in g.SOURCES and os.path.isfile(os.path.join(g.CSRC, "plda_adapt.hip"))
    header = open(os.path.join(repo_root, "include", "xvec_hip.h")).read()
    assert "parity unpinned" in header[header.index("csrc/plda_adapt.hip"):header.index("int64_t xv_plda_adapt_workspace")]


def test_argument_refusals_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x10000)                               # never followed: every check comes before the first HIP call
    big = 1 << 40

    def call(d=7, offsets=(0, 2, 5), te=0.5, ws=fake, ws_bytes=big, groups=None, ldx=None):
        off = (C.c_int64 * len(offsets))(*offsets)
        return lib.xv_plda_adapt(0, fake, d if ldx is None else ldx, off, len(offsets) - 1 if groups is None else groups, d, fake,
                                 fake, fake, te, fake, fake, fake, fake, fake, ws, ws_bytes, None)

    assert call(d=257) == _lib.XV_ERR_UNSUPPORTED and call(d=0) == _lib.XV_ERR_UNSUPPORTED
    assert lib.xv_plda_adapt_workspace(3, 257) == _lib.XV_ERR_UNSUPPORTED and lib.xv_plda_adapt_workspace(3, 0) == _lib.XV_ERR_UNSUPPORTED
    assert call(offsets=(0, 4, 3)) == _lib.XV_ERR_INVALID and call(offsets=(-1, 4, 5)) == _lib.XV_ERR_INVALID
    for te in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        assert call(te=te) == _lib.XV_ERR_INVALID, te
    assert call(ws=C.c_void_p(0x10004)) == _lib.XV_ERR_INVALID
    assert call(ldx=6) == _lib.XV_ERR_INVALID and call(groups=-1) == _lib.XV_ERR_INVALID
    need = lib.xv_plda_adapt_workspace(2, 7)
    assert need == 256 + 32 * 8 * 8                         # the group table and one slot of four 8 x 8 matrices
    assert lib.xv_plda_adapt_slot_bytes(7) == 32 * 8 * 8 and lib.xv_plda_adapt_slot_bytes(257) == _lib.XV_ERR_UNSUPPORTED
    assert lib.xv_plda_adapt_workspace(2, 256) == 256 + 32 * 256 * 256 and lib.xv_plda_adapt_workspace(100, 1) == 1792 + 128
    assert call(ws_bytes=need - 1) == _lib.XV_ERR_WORKSPACE and call(ws=None) == _lib.XV_ERR_WORKSPACE
    assert b"workspace" in lib.xv_last_error(None)
    assert call(groups=0) == _lib.XV_OK                      # nothing to do: returns before any pointer is looked at
    assert lib.xv_plda_adapt(0, None, 7, None, 0, 7, None, None, None, 1.0, None, None, None, None, None, None, 0, None) == _lib.XV_OK


def test_python_refusals_need_no_gpu():
    from tf_kaldi_speaker_amd import plda
    for te in (0.0, 1.5, float("nan"), -1.0):
        with pytest.raises(ValueError, match="target_energy"):
            plda._check_target_energy(te)
    assert plda._check_target_energy(1) == 1.0
    ad = plda.AdaptedPlda(np.eye(2, 5), np.ones((2, 6)), [2.0, 1.0], np.arange(5.0)[::-1])
    assert ad.dim == 2 and ad.in_dim == 5 and ad.pca.dtype == np.float64 and ad.affine.shape == (2, 6)
    assert plda._same_model(ad, plda.AdaptedPlda(None, np.ones((2, 6)), [2.0, 1.0], None))
    assert not plda._same_model(ad, plda.AdaptedPlda(None, np.ones((2, 6)), [2.0, 0.5], None))
    assert not plda._same_model(ad, plda.Plda(np.zeros(2), np.eye(2), [2.0, 1.0]))
    with pytest.raises(ValueError):
        plda.AdaptedPlda(np.eye(3, 5), np.ones((2, 6)), [2.0, 1.0], None)


def test_parse_args():
    from tf_kaldi_speaker_amd import cluster
    tail = ["utt2reco", "ark:x.ark", "labels"]
    assert cluster.parse_args(["--plda", "plda"] + tail).target_energy is None
    assert cluster.parse_args(["--plda", "plda", "--target-energy", "0.1"] + tail).target_energy == 0.1
    assert cluster.parse_args(["--plda", "plda", "--target-energy", "1"] + tail).target_energy == 1.0
    for bad in (["--target-energy", "0.1"], ["--plda", "plda", "--target-energy", "0"], ["--plda", "plda", "--target-energy", "1.01"],
                ["--plda", "plda", "--target-energy", "nan"], ["--plda", "plda", "--target-energy", "-0.5"]):
        with pytest.raises(SystemExit):
            cluster.parse_args(bad + tail)


def test_cluster_sh_passes_the_option(repo_root):
    text = open(os.path.join(repo_root, "bin", "cluster.sh")).read()
    assert "target_energy=" in text and "--target-energy $target_energy" in text


def test_model_files_are_untouched(tmp_path):
    from tf_kaldi_speaker_amd import plda
    rng = np.random.default_rng(3)
    model = plda.Plda(*ref_plda.random_model(rng, 5))
    for binary in (True, False):
        path = str(tmp_path / ("plda_%d" % binary))
        plda.write_plda(path, model, binary=binary)
        back = plda.read_plda(path)
        assert type(back) is plda.Plda and back.dim == 5
        assert np.array_equal(back.mean, model.mean) and np.array_equal(back.transform, model.transform) and np.array_equal(back.psi, model.psi)
    data = open(str(tmp_path / "plda_1"), "rb").read()
    assert data.startswith(b"\0B<Plda> ") and data.endswith(b"</Plda> ") and len(data) == 9 + (3 + 5 + 40) + (3 + 10 + 200) + (3 + 5 + 40) + 8
