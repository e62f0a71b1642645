"""Host side of the VB-HMM resegmentation (xv_vbx, csrc/vbx.hip): the properties of the oracle, the declarations, the workspace
size, every refusal of the C entry point (all come before the first HIP call, so they answer on a machine without a GPU), the
host pieces of vbx.py and the command line."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_vbx as rv  # noqa: E402

NAN, INF = float("nan"), float("inf")


def _start(t_len, r, s, speakers, **kw):
    x, a, psi, init, _ = rv.case(t_len, r, s, speakers, **kw)
    g0, pi0 = rv.init_gamma(init, s)
    return x, a, psi, g0, pi0


# ------------------------------------------------------------------------------------------------- the oracle against itself

@pytest.mark.parametrize("shape", [(65, 7, 5, 3), (200, 16, 8, 3), (1, 4, 3, 1), (2, 5, 1, 1), (40, 3, 64, 5)])
def test_oracle_properties(shape):
    """gamma rows and pi sum to 1; the ELBO does not decrease by more than the bar of tests/test_gpu_vbx.py (16 x |float64 -
    longdouble| + the floor); the diagonal-plus-rank-one transition and the dense one agree within the same bar."""
    t_len, r, s, speakers = shape
    x, a, psi, g0, pi0 = _start(t_len, r, s, speakers, scale=0.5)
    opts = dict(loop_prob=0.9, max_iters=10, epsilon=-INF)
    ref, bar = rv.bars(x, a, psi, g0, pi0, **opts)
    assert ref.iters == 10 and ref.gamma.shape == (t_len, s) and ref.labels.shape == (t_len,)
    assert np.all(np.isfinite(ref.gamma)) and np.all(np.isfinite(ref.pi)) and np.all(np.isfinite(ref.elbo))
    assert np.max(np.abs(ref.gamma.sum(axis=1) - 1.0)) <= s * bar["gamma"].max()
    assert abs(ref.pi.sum() - 1.0) <= 4 * s * 2.0 ** -53
    drop = np.diff(ref.elbo)
    assert np.all(drop >= -(bar["elbo"][1:] + bar["elbo"][:-1])), drop.min()
    dense = rv.vb_hmm(x, a, psi, g0, pi0, dense=True, **opts)
    assert np.all(np.abs(dense.gamma - ref.gamma) <= bar["gamma"])
    assert np.all(np.abs(dense.pi - ref.pi) <= bar["pi"])
    assert np.all(np.abs(dense.elbo - ref.elbo) <= bar["elbo"])
    assert np.array_equal(ref.labels, np.argmax(ref.gamma, axis=1))


def test_oracle_dead_speaker_stays_dead():
    x, a, psi, g0, pi0 = _start(65, 7, 5, 3)
    pi0 = np.array([0.5, 0.0, 0.25, 0.0, 0.25])
    for dense in (False, True):
        res = rv.vb_hmm(x, a, psi, g0, pi0, max_iters=5, epsilon=-INF, dense=dense)
        assert np.all(res.gamma[:, [1, 3]] == 0.0) and np.all(res.pi[[1, 3]] == 0.0)
        assert not np.any(np.isnan(res.gamma)) and not np.any(np.isnan(res.pi)) and not np.any(np.isnan(res.elbo))
        assert abs(res.pi.sum() - 1.0) <= 1e-15 and np.max(np.abs(res.gamma.sum(axis=1) - 1.0)) <= 1e-9


def test_oracle_one_frame_one_speaker():
    x, a, psi, g0, pi0 = _start(1, 4, 1, 1)
    res = rv.vb_hmm(x, a, psi, g0, pi0, max_iters=3, epsilon=-INF)
    assert res.gamma.shape == (1, 1) and res.gamma[0, 0] == 1.0 and res.pi[0] == 1.0 and res.iters == 3 and res.labels[0] == 0
    x, a, psi, g0, pi0 = _start(1, 4, 3, 1)
    res = rv.vb_hmm(x, a, psi, g0, pi0, max_iters=2, epsilon=-INF)          # T = 1: pi <- gamma_0
    assert np.allclose(res.pi, res.gamma[0], rtol=0, atol=1e-15)


def test_oracle_stops_and_pads():
    x, a, psi, g0, pi0 = _start(200, 16, 8, 3, scale=0.5)
    res = rv.vb_hmm(x, a, psi, g0, pi0, loop_prob=0.9)
    assert 2 <= res.iters < 40 and np.all(np.isnan(res.elbo[res.iters:])) and np.all(np.isfinite(res.elbo[:res.iters]))
    assert res.elbo[res.iters - 1] - res.elbo[res.iters - 2] < 1e-6 <= res.elbo[res.iters - 2] - res.elbo[res.iters - 3]
    assert rv.vb_hmm(x, a, psi, g0, pi0, loop_prob=0.9, max_iters=1).iters == 1
    assert rv.floor(200, 16, 8, 0.5) == 402 * 32 * 2.0 ** -53


# ------------------------------------------------------------------------------------------------- declarations and refusals

def test_symbols_declared_listed_and_built(repo_root):
    import __graft_entry__ as g
    assert "vbx.hip" in g.SOURCES and os.path.isfile(os.path.join(g.CSRC, "vbx.hip"))
    assert "vbx.hip" not in g.NO_SCRATCH
    header = open(os.path.join(repo_root, "include", "xvec_hip.h")).read()
    assert "parity unpinned" in header[header.index("csrc/vbx.hip"):header.index("int64_t xv_vbx_workspace")]


def _lib_loaded():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    return _lib, _lib.load()


def test_workspace_values():
    _lib, lib = _lib_loaded()

    def ws(offsets, spk, r):
        off = (C.c_int64 * len(offsets))(*offsets)
        sp = (C.c_int32 * max(len(spk), 1))(*spk)
        return lib.xv_vbx_workspace(len(offsets) - 1, off, sp, r)

    assert ws((0, 10), (3,), 7) == 256 + 8 * (10 * 9 + 3 * 30)
    assert ws((5, 15), (3,), 7) == 256 + 8 * (10 * 9 + 3 * 30)                      # only differences of offsets count
    assert ws((0, 10, 10, 12), (3, 64, 1), 256) == 256 + 8 * (12 * 258 + 3 * (30 + 0 + 2))
    assert ws(tuple(range(0, 10)), (2,) * 9, 1) == 512 + 8 * (9 * 3 + 3 * 18)      # 9 groups: 288 bytes of table -> 512
    assert ws((0, 8192), (64,), 256) == 256 + 8 * (8192 * 258 + 3 * 8192 * 64)
    assert lib.xv_vbx_workspace(0, None, None, 7) == 0
    assert ws((0, 10), (3,), 0) == _lib.XV_ERR_UNSUPPORTED and ws((0, 10), (3,), 257) == _lib.XV_ERR_UNSUPPORTED
    assert ws((0, 10), (0,), 7) == _lib.XV_ERR_UNSUPPORTED and ws((0, 10), (65,), 7) == _lib.XV_ERR_UNSUPPORTED
    assert ws((0, 8193), (3,), 7) == _lib.XV_ERR_UNSUPPORTED
    assert ws((0, 10, 9), (3, 3), 7) == _lib.XV_ERR_INVALID and ws((-1, 10), (3,), 7) == _lib.XV_ERR_INVALID
    assert lib.xv_vbx_workspace(-1, None, None, 7) == _lib.XV_ERR_INVALID


def test_argument_refusals_need_no_gpu():
    _lib, lib = _lib_loaded()
    fake = C.c_void_p(0x10000)                               # never followed: every check comes before the first HIP call
    big = 1 << 40

    def call(offsets=(0, 2, 5), spk=(2, 3), r=7, d=9, ldx=None, fa=0.3, fb=17.0, loop=0.99, iters=40, eps=1e-6, ws=fake, ws_bytes=big,
             groups=None):
        off = (C.c_int64 * len(offsets))(*offsets)
        sp = (C.c_int32 * len(spk))(*spk)
        return lib.xv_vbx(0, fake, d if ldx is None else ldx, off, sp, len(offsets) - 1 if groups is None else groups, d, fake, fake, r,
                          fake, fake, fa, fb, loop, iters, eps, fake, fake, fake, ws, ws_bytes, None)

    U, I, W = _lib.XV_ERR_UNSUPPORTED, _lib.XV_ERR_INVALID, _lib.XV_ERR_WORKSPACE
    assert call(spk=(0, 3)) == U and call(spk=(2, 65)) == U and call(r=0) == U and call(r=257) == U
    assert call(d=0) == U and call(d=2049) == U and call(offsets=(0, 8193, 8194)) == U
    assert call(spk=(2, 64), r=256, d=2048, offsets=(0, 8192, 8193), ws_bytes=0) == W       # the limits themselves are legal
    assert call(offsets=(0, 4, 3)) == I and call(offsets=(-1, 4, 5)) == I and call(ldx=8) == I and call(groups=-1) == I
    for bad in (0.0, -1.0, NAN, INF):
        assert call(fa=bad) == I and call(fb=bad) == I, bad
    for bad in (-1e-9, 1.0000001, NAN, INF):
        assert call(loop=bad) == I, bad
    assert call(iters=0) == I and call(iters=-3) == I and call(eps=NAN) == I
    assert call(ws=C.c_void_p(0x10004)) == I
    need = lib.xv_vbx_workspace(2, (C.c_int64 * 3)(0, 2, 5), (C.c_int32 * 2)(2, 3), 7)
    assert need == 256 + 8 * (5 * 9 + 3 * (4 + 9))
    assert call(ws_bytes=need - 1) == W and call(ws=None) == W
    assert b"workspace" in lib.xv_last_error(None)
    assert call(ws_bytes=need, ws=C.c_void_p(0x10004)) == I
    assert call(groups=0) == _lib.XV_OK                      # nothing to do: returns before any pointer is looked at
    assert lib.xv_vbx(0, None, 9, None, None, 0, 9, None, None, 7, None, None, 0.3, 17.0, 0.99, 40, -INF, None, None, None, None, 0, None) == _lib.XV_OK
    assert call(loop=0.0, ws_bytes=0) == W and call(loop=1.0, ws_bytes=0) == W and call(eps=-INF, ws_bytes=0) == W     # legal options


# ------------------------------------------------------------------------------------------------- host pieces of vbx.py

def test_label_mapping_and_start_values():
    from tf_kaldi_speaker_amd import vbx
    lab, s = vbx.map_labels([7, 7, -2, 7, 100, -2, 3])
    assert s == 4 and lab.tolist() == [0, 0, 1, 0, 2, 1, 3]
    lab, s = vbx.map_labels(np.array([5]))
    assert s == 1 and lab.tolist() == [0]
    assert vbx.map_labels([2, 1, 0, 1])[0].tolist() == [0, 1, 2, 1]           # also the final renumbering: by lowest row
    g, pi = vbx.init_gamma([0, 2, 1], 3, 5.0)
    hot, cold = math.exp(5.0) / (math.exp(5.0) + 2.0), 1.0 / (math.exp(5.0) + 2.0)
    assert np.allclose(g, np.where(np.eye(3)[[0, 2, 1]] > 0, hot, cold), rtol=1e-15, atol=0) and np.array_equal(pi, np.full(3, 1.0 / 3.0))
    ref_g, ref_pi = rv.init_gamma([0, 2, 1], 3, 5.0)
    assert np.array_equal(g, ref_g) and np.array_equal(pi, ref_pi)
    assert np.array_equal(vbx.init_gamma([0, 1], 2, 0.0)[0], np.full((2, 2), 0.5))
    for name in ("fa", "fb", "loop_prob", "max_iters", "epsilon"):
        assert vbx.DEFAULTS[name] == rv.DEFAULTS[name]


def test_options_and_models():
    from tf_kaldi_speaker_amd import plda, vbx
    assert vbx.check_options(0.3, 17, 0.99, 40, -INF) == (0.3, 17.0, 0.99, 40, -INF)
    for bad in (dict(fa=0), dict(fb=-1), dict(fa=NAN), dict(fb=INF), dict(loop_prob=1.5), dict(loop_prob=NAN), dict(max_iters=0),
                dict(max_iters=2.5), dict(epsilon=NAN)):
        with pytest.raises(ValueError):
            vbx.check_options(**dict(dict(fa=0.3, fb=17.0, loop_prob=0.99, max_iters=40, epsilon=1e-6), **bad))
    rng = np.random.default_rng(5)
    model = plda.Plda(rng.standard_normal(4), rng.standard_normal((4, 4)), [3.0, 2.0, 1.0, 0.5])
    a, psi = vbx.model_operands(model)
    assert a.shape == (4, 5) and np.array_equal(a[:, :4], model.transform) and np.array_equal(a[:, 4], -(model.transform @ model.mean))
    ref_a, ref_psi = rv.model_affine(model.mean, model.transform, model.psi, 2)
    a, psi = vbx.model_operands(model, lda_dim=2)
    assert np.array_equal(a, ref_a) and np.array_equal(psi, ref_psi) and psi.tolist() == [3.0, 2.0]
    ad = plda.AdaptedPlda(None, np.arange(12.0).reshape(2, 6), [2.0, 1.0], None)
    a, psi = vbx.model_operands(ad)
    assert np.array_equal(a, ad.affine) and psi.tolist() == [2.0, 1.0]
    for bad in (0, 5):
        with pytest.raises(ValueError, match="lda_dim"):
            vbx.model_operands(model, lda_dim=bad)
    big = plda.Plda(np.zeros(257), np.eye(257), np.ones(257))
    with pytest.raises(ValueError, match="at most 256"):
        vbx.model_operands(big)
    assert vbx.model_operands(big, lda_dim=256)[0].shape == (256, 258)


def test_chunks_and_resegment_refusals():
    from tf_kaldi_speaker_amd import plda, vbx
    one = vbx._call_bytes(100, 4, 16, 40)
    assert one == 8 * (100 * 18 + 1200) + 3200 + 400 + 320 + 32 + 36
    assert vbx._chunks([100] * 5, [4] * 5, 16, 40, 2 * one) == [[0, 1], [2, 3], [4]]
    assert vbx._chunks([100] * 3, [4] * 3, 16, 40, 1) == [[0], [1], [2]]            # a run holds at least one group
    assert vbx._chunks([], [], 16, 40, 100) == []
    model = plda.Plda(np.zeros(3), np.eye(3), np.ones(3))
    x = np.zeros((70, 3), np.float32)
    groups = ["b"] * 66 + ["a"] * 4
    with pytest.raises(ValueError, match="recording b has 65 distinct initial labels"):
        vbx.resegment(model, x, groups, list(range(65)) + [0] * 5)
    with pytest.raises(ValueError, match="init_labels"):
        vbx.resegment(model, x, groups, [0] * 69)
    with pytest.raises(ValueError, match="loop_prob"):
        vbx.resegment(model, x, groups, [0] * 70, loop_prob=2.0)
    with pytest.raises(ValueError, match="no adapted model"):
        vbx.resegment({"a": plda.AdaptedPlda(None, np.ones((2, 4)), [2.0, 1.0], None)}, x, groups, [0] * 70)


# ------------------------------------------------------------------------------------------------- the command line

def test_time_order_and_label_file(tmp_path):
    from tf_kaldi_speaker_amd import vb_resegment as cmd
    keys = ["k3", "k1", "k2", "k0", "k4"]
    segments = [("k0", "r1", 0.0, 1.5), ("k1", "r1", 3.0, 4.5), ("k2", "r2", 0.5, 2.0), ("k3", "r1", 1.5, 3.0), ("k4", "r2", 0.5, 2.0),
                ("other", "r9", 0.0, 1.0)]
    order = cmd.time_order(keys, segments)
    assert [keys[i] for i in order] == ["k0", "k2", "k4", "k3", "k1"]         # (start, end, key); ties by key
    with pytest.raises(ValueError, match="1 keys have no segment .first: k9."):
        cmd.time_order(keys + ["k9"], segments)
    path = tmp_path / "labels"
    path.write_text("k0 1\nk1 2\n\nk2 -7\n")
    assert cmd.read_labels(str(path)) == {"k0": 1, "k1": 2, "k2": -7}
    path.write_text("k0 1\nk1 two\n")
    with pytest.raises(ValueError, match=":2: expected `key label`"):
        cmd.read_labels(str(path))
    path.write_text("k0 1 extra\n")
    with pytest.raises(ValueError, match=":1:"):
        cmd.read_labels(str(path))


def test_parse_args():
    from tf_kaldi_speaker_amd import vb_resegment as cmd
    tail = ["utt2reco", "ark:x.ark", "init", "labels"]
    args = cmd.parse_args(["--plda", "plda"] + tail)
    assert (args.fa, args.fb, args.loop_prob, args.init_smoothing, args.max_iters, args.epsilon) == (0.3, 17.0, 0.99, 5.0, 40, 1e-6)
    assert args.lda_dim is None and args.normalize is True and args.smoothing == 0.0 and args.init_labels == "init"
    args = cmd.parse_args(["--plda", "plda", "--lda-dim", "64", "--epsilon=-inf", "--loop-prob", "1", "--segments", "s", "--rttm-out", "r"] + tail)
    assert args.lda_dim == 64 and args.epsilon == -INF and args.loop_prob == 1.0 and args.rttm_out == "r"
    assert cmd.parse_args(["--plda", "plda", "--segments", "s"] + tail).rttm_out == ""      # ordering alone needs no RTTM
    for bad in ([], ["--plda", "plda", "--fa", "0"], ["--plda", "plda", "--fb", "-2"], ["--plda", "plda", "--loop-prob", "1.5"],
                ["--plda", "plda", "--max-iters", "0"], ["--plda", "plda", "--epsilon", "nan"], ["--plda", "plda", "--lda-dim", "0"],
                ["--plda", "plda", "--rttm-out", "r"], ["--plda", "plda", "--smoothing", "2"], ["--plda", "plda", "--init-smoothing", "-1"],
                ["--plda", "plda", "--fa", "nan"]):
        with pytest.raises(SystemExit):
            cmd.parse_args(bad + tail)
    with pytest.raises(SystemExit):
        cmd.parse_args(["--plda", "plda"] + tail[:3])


def test_wrapper_script_passes_the_options(repo_root):
    path = os.path.join(repo_root, "bin", "vb_resegment.sh")
    text = open(path).read()
    assert os.access(path, os.X_OK)
    assert "python -m tf_kaldi_speaker_amd.vb_resegment" in text
    for opt in ("--plda $plda", "--lda-dim $lda_dim", "--loop-prob $loop_prob", "--init-smoothing $init_smoothing", "--max-iters $max_iters",
                "--epsilon=$epsilon", "--fa $fa", "--fb $fb", "--segments $segments", "--rttm-out $rttm_out", "--smoothing $smoothing"):
        assert opt in text, opt
