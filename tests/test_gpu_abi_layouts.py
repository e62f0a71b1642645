"""GPU: padded and unaligned operand layouts through the C ABI (include/xvec_hip.h: "ld >= width", operands anywhere in device
memory, a few documented in-place forms).  The Python wrappers make every operand contiguous and pass ld == width, and the torch
allocator returns 16-byte aligned bases, so the rest of the suite never reaches the scalar kernels through a misaligned base,
the mixed branch of the vector kernels (a partial last float4: d = 150, ld = 156), or a real row stride in the row kernels.

Every entry point below is called raw (ctypes, the prototypes of tf_kaldi_speaker_amd._lib) once per layout of
tests/helpers/abi_layouts.py: inputs sit in NaN-poisoned frames, outputs in canary frames with ld > width.  Asserted per call:

 1. return code 0 and a finite result (a NaN means that a padding column was read);
 2. the oracle and the bar the contiguous case already has: ref_score.delta(d) for the cosine calls, ref_plda.score_bar for the
    PLDA scores, the bound of csrc/loss.hip through tests/test_gpu_loss.check, (n + 16) 2^-53 sum |w y y| for the Gram calls
    (tests/test_gpu_backend._oracle), and the comparisons the post-step, front-end and VAD tests make against oracle/ref_post.py,
    oracle/ref_frontend.py and tests/helpers/ref_mfcc.py.  No tolerance here is new;
 3. bit identity with the `tight` twin.  It holds for every entry point of this file, by reading: score_tile_kernel /
    loss_tile_kernel stage the same values into LDS whichever load instruction fetched them (the affine form subtracts the same
    mean element in both branches) and run the same MFMAs in the same order; score_pairs_kernel keeps the same four fmaf
    chains per lane in its vector and scalar branches; row_prepare_kernel, plda_rows_kernel, loss_classes_kernel,
    loss_rows_kernel, the Gram loader, class_mean_kernel, length_norm_kernel, speaker_mean_kernel, the CMN kernels and
    vad_kernel index scalars by (row * ld + column) and sum in an order that does not depend on ld.  Histograms are equal count
    for count;
 4. abi_layouts.untouched on every output frame and abi_layouts.intact on every input frame;
 5. the in-place forms: xv_length_normalize (out == x), xv_score_prepare without a transform (out == x), xv_plda_prepare
    without a transform (rows == x), each on padded frames.

xv_forward takes its one layout case through Trainer.predict_packed: features [rows, 30 + 2] whose two extra columns are NaN
(feat_ld != feat_dim: the strided arms of the staging and per-utterance guard kernels), all four precisions.

Shapes are the smallest that still cross a 128-row tile, a 32-wide K step and a float4: every case is milliseconds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import abi_layouts as L  # noqa: E402
import ref_mfcc  # noqa: E402
import ref_plda  # noqa: E402
import ref_score  # noqa: E402
from oracle import ref_frontend, ref_numpy, ref_post  # noqa: E402
from test_gpu_backend import _oracle as gram_oracle  # noqa: E402
from test_gpu_loss import check as loss_check, edge_labels  # noqa: E402
from test_gpu_plda import _check_bracket as plda_bracket, _f32_prepare  # noqa: E402
from test_gpu_scoring import _check_bracket as cosine_bracket, _f32_chain  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24, U53 = 2.0 ** -24, 2.0 ** -53
DIMS = [3, 33, 150, 200]             # below a float4; a 32-wide K step plus one; a partial float4 under pad4; clean
SETS = [(1, 1), (37, 129)]           # 129 = one 128-row tile plus one row
# the layout of an output next to an input of layout X: always ld > width
OUT_OF = {"tight": "pad4", "pad4": "pad_odd", "pad_odd": "shift1", "shift1": "shift3", "shift3": "pad4"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    return _lib.load()


def put(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def fp(frame):
    return C.c_void_p(frame.ptr)


def fin(a, layout):
    return L.place(a, layout, DEV, poison="nan")[0]


def fout(rows, width, layout, dtype=np.float32):
    return L.blank(rows, width, layout, DEV, dtype)[0]


def vout(n, dtype=np.float32):
    """A plain output vector [n] as a one-row canary frame at an odd element offset."""
    return fout(1, n, "shift1", dtype)


def done(rc):
    import torch
    torch.cuda.synchronize()
    assert rc == 0, rc


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def scaled_rows(rng, n, d, lo=-6, hi=6):
    return (rng.standard_normal((n, d)) * np.exp2(rng.integers(lo, hi + 1, (n, 1)))).astype(np.float32)


def unit_rows(rng, n, d):
    """Prepared rows as the scoring calls take them: unit in float64, rounded once to float32."""
    return ref_score.prepare(scaled_rows(rng, n, d)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ cosine: prepare
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("d", DIMS)
def test_score_prepare_rows(lib, d, n):
    """xv_score_prepare without a transform (row_prepare_kernel with ldx, ldy != dim): mean + length norm; the rule of
    tests/test_gpu_scoring.test_prepare, bar = max(delta(d), 4 x the error of the float32 numpy chain).  In place on padded frames."""
    rng = np.random.default_rng(10 * d + n)
    x = scaled_rows(rng, n, d)
    mean = (0.5 * rng.standard_normal(d)).astype(np.float32)
    meand = put(mean)
    want = ref_score.prepare(x, mean=mean)
    bar = max(ref_score.delta(d), 4 * np.max(np.abs(_f32_chain(x, mean, None, True, 0.0) - want)))
    twin = None
    for lay in L.LAYOUTS:
        fx, fo = fin(x, lay), fout(n, d, OUT_OF[lay])
        done(lib.xv_score_prepare(0, fp(fx), fx.ld, n, d, tp(meand), None, 0, d, 0, 1, 0.0, fp(fo), fo.ld, None))
        got = L.gather(fo)
        assert np.all(np.isfinite(got)), lay
        assert np.max(np.abs(got - want)) <= bar, lay
        assert L.intact(fx, x) and L.untouched(fo), lay
        twin = got if twin is None else twin
        assert same_bits(got, twin), lay
    for lay in ("pad4", "pad_odd", "shift1", "shift3"):
        fx = fin(x, lay)
        done(lib.xv_score_prepare(0, fp(fx), fx.ld, n, d, tp(meand), None, 0, d, 0, 1, 0.0, fp(fx), fx.ld, None))
        assert same_bits(L.gather(fx), twin) and L.untouched(fx), lay


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("d_in", [33, 150])
def test_score_prepare_transform(lib, d_in, offset):
    """xv_score_prepare with a transform [d_out, t_cols] behind ldt, t_cols = d_in and d_in + 1 (EPI_AFFINE of score_tile_kernel:
    the mean subtracted at load, column d_in of the transform read through ldb), then the length norm in place on the padded
    output.  Bar as above."""
    rng = np.random.default_rng(100 + d_in + offset)
    n, d_out = 37, 129
    x = scaled_rows(rng, n, d_in)
    mean = (0.5 * rng.standard_normal(d_in)).astype(np.float32)
    t = (rng.standard_normal((d_out, d_in + offset)) / np.sqrt(d_in)).astype(np.float32)
    meand = put(mean)
    want = ref_score.prepare(x, mean=mean, transform=t)
    bar = max(ref_score.delta(d_in), 4 * np.max(np.abs(_f32_chain(x, mean, t, True, 0.0) - want)))
    twin = None
    for la, lb in L.PAIRS:
        fx, ft, fo = fin(x, la), fin(t, lb), fout(n, d_out, OUT_OF[la])
        done(lib.xv_score_prepare(0, fp(fx), fx.ld, n, d_in, tp(meand), fp(ft), ft.ld, d_out, d_in + offset, 1, 0.0, fp(fo), fo.ld, None))
        got = L.gather(fo)
        assert np.all(np.isfinite(got)), (la, lb)
        assert np.max(np.abs(got - want)) <= bar, (la, lb)
        assert L.intact(fx, x) and L.intact(ft, t) and L.untouched(fo), (la, lb)
        twin = got if twin is None else twin
        assert same_bits(got, twin), (la, lb)


# ------------------------------------------------------------------------------------------------ cosine: scores
@pytest.mark.parametrize("n,m", SETS)
@pytest.mark.parametrize("d", DIMS)
def test_score_matrix_and_pairs(lib, d, n, m):
    """xv_score_matrix and xv_score_pairs over prepared rows: delta(d) against the float64 product of the rows the kernel saw."""
    rng = np.random.default_rng(1000 + d + n)
    a, b = unit_rows(rng, n, d), unit_rows(rng, m, d)
    want = ref_score.cosine_matrix(a, b)
    delta = ref_score.delta(d)
    k = min(n * m, 333)
    ia, ib = rng.integers(0, n, k).astype(np.int32), rng.integers(0, m, k).astype(np.int32)
    rep = k // 3
    if rep:
        ia[-rep:], ib[-rep:] = ia[:rep].copy(), ib[:rep].copy()                          # repeats
    iad, ibd = put(ia), put(ib)
    twin_m = twin_p = None
    for la, lb in L.PAIRS:
        fa, fb, fo = fin(a, la), fin(b, lb), fout(n, m, OUT_OF[la])
        done(lib.xv_score_matrix(0, fp(fa), fa.ld, n, fp(fb), fb.ld, m, d, fp(fo), fo.ld, None))
        got = L.gather(fo)
        assert np.all(np.isfinite(got)), ("matrix", la, lb)           # a NaN: a padding column reached a score
        assert np.max(np.abs(got - want)) <= delta, ("matrix", la, lb)
        assert L.untouched(fo), ("matrix", la, lb)
        po = vout(k)
        done(lib.xv_score_pairs(0, fp(fa), fa.ld, n, fp(fb), fb.ld, m, d, tp(iad), tp(ibd), k, fp(po), None))
        pairs = L.gather(po)[0]
        assert np.all(np.isfinite(pairs)), ("pairs", la, lb)
        assert np.max(np.abs(pairs - want[ia, ib])) <= delta, ("pairs", la, lb)
        assert same_bits(pairs[k - rep:], pairs[:rep]), ("pairs", la, lb)
        assert L.untouched(po) and L.intact(fa, a) and L.intact(fb, b), (la, lb)
        twin_m, twin_p = (got, pairs) if twin_m is None else (twin_m, twin_p)
        assert same_bits(got, twin_m) and same_bits(pairs, twin_p), (la, lb)


def hist_frames(nbins):
    zero = np.zeros((1, nbins), np.int64)              # the histograms are added to: zeros inside a canary frame
    return L.place(zero, "shift1", DEV, poison="canary")[0], L.place(zero, "pad4", DEV, poison="canary")[0]


def counts_of(frame):
    return L.gather(frame)[0].view(np.uint64)


@pytest.mark.parametrize("nbins", [256, 65536])        # LDS epilogue, global epilogue
@pytest.mark.parametrize("n,m", SETS)
@pytest.mark.parametrize("d", DIMS)
def test_score_histogram(lib, d, n, m, nbins):
    """xv_score_histogram over two sets (the five layout pairs) and over one set with `self` (a == b: one layout at a time).  The
    tight run is bracketed by the oracle's counts at delta(d) (tests/test_gpu_scoring._check_bracket); every other layout must
    give the same counts."""
    rng = np.random.default_rng(2000 + d + n)
    a, b = unit_rows(rng, n, d), unit_rows(rng, m, d)
    la_, lb_ = rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 5, m).astype(np.int32)
    lad, lbd = put(la_), put(lb_)
    delta = ref_score.delta(d)
    s = ref_score.cosine_matrix(a, b)
    eq = la_[:, None] == lb_[None, :]
    twin = None
    for la, lb in L.PAIRS:
        fa, fb = fin(a, la), fin(b, lb)
        hs, hd = hist_frames(nbins)
        done(lib.xv_score_histogram(0, fp(fa), fa.ld, n, tp(lad), fp(fb), fb.ld, m, tp(lbd), d, 0, nbins, fp(hs), fp(hd), None))
        cs, cd = counts_of(hs), counts_of(hd)
        assert int(cs.sum()) == int(eq.sum()) and int(cd.sum()) == eq.size - int(eq.sum()), (la, lb)
        assert L.untouched(hs) and L.untouched(hd) and L.intact(fa, a) and L.intact(fb, b), (la, lb)
        if twin is None:
            cosine_bracket(cs, np.sort(s[eq]), nbins, delta, "same-label")
            cosine_bracket(cd, np.sort(s[~eq]), nbins, delta, "different-label")
            twin = (cs, cd)
        assert np.array_equal(cs, twin[0]) and np.array_equal(cd, twin[1]), (la, lb)
    same, diff = ref_score.self_pairs(ref_score.cosine_matrix(b, b), lb_)
    twin = None
    for lay in L.LAYOUTS:
        fb = fin(b, lay)
        hs, hd = hist_frames(nbins)
        done(lib.xv_score_histogram(0, fp(fb), fb.ld, m, tp(lbd), fp(fb), fb.ld, m, tp(lbd), d, 1, nbins, fp(hs), fp(hd), None))
        cs, cd = counts_of(hs), counts_of(hd)
        assert int(cs.sum()) == same.size and int(cd.sum()) == diff.size, lay
        assert L.untouched(hs) and L.untouched(hd) and L.intact(fb, b), lay
        if twin is None:
            cosine_bracket(cs, np.sort(same), nbins, delta, "self same-label")
            cosine_bracket(cd, np.sort(diff), nbins, delta, "self different-label")
            twin = (cs, cd)
        assert np.array_equal(cs, twin[0]) and np.array_equal(cd, twin[1]), lay


# ------------------------------------------------------------------------------------------------ PLDA
PLDA_CASES = [(3, "n1"), (33, "n1"), (33, "mixed"), (150, "n1"), (200, "n1")]      # mixed: k = 2 d


def plda_model(d, kind):
    from tf_kaldi_speaker_amd import plda
    rng = np.random.default_rng(3000 + d + (kind == "mixed"))
    model = plda.Plda(*ref_plda.random_model(rng, d))

    def rows(count):
        x, _ = ref_plda.draw(rng, model.mean, model.transform, model.psi, count, 1)
        return ((x - model.mean) * np.exp2(rng.integers(-6, 7, (count, 1))) + model.mean).astype(np.float32)
    xe, xt = rows(37), rows(129)
    counts = rng.integers(1, 31, 37) if kind == "mixed" else np.ones(37, np.int64)
    return plda, rng, model, xe, xt, counts


def enrol_tables(plda, model, counts, d):
    """The per-n tables of tf_kaldi_speaker_amd.plda._prepare for an enrolment set -> (tables [T, 4, d], logdet [T], index)."""
    distinct, index = np.unique(counts, return_inverse=True)
    tab, logdet = np.zeros((distinct.size, 4, d)), np.zeros(distinct.size)
    for k, nu in enumerate(distinct):
        t = plda.tables(model.psi, int(nu))
        tab[k, 0], tab[k, 1], tab[k, 2], tab[k, 3], logdet[k] = t["inv"], t["a"], t["q"], t["w"], t["logdet"]
    return tab, logdet, index.astype(np.int32)


@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("d,kind", PLDA_CASES)
def test_plda_prepare(lib, d, kind, n):
    """xv_plda_prepare, enrolment side: x behind ldx, the affine transform [d, d + 1] behind ldt, rows behind ldr, packed rows
    (d or 2 d wide) behind ldp, the bias a plain vector.  Rows against Plda::TransformIvector in float64 by the rule of
    tests/test_gpu_plda.test_prepare; rho and the packed operand from the device's own rows, as there."""
    plda, rng, model, xe, _, counts = plda_model(d, kind)
    x, counts = xe[:n], counts[:n]
    second = int(kind == "mixed")
    kp = 2 * d if second else d
    tab, logdet, index = enrol_tables(plda, model, counts, d)
    aff = np.concatenate([model.transform, -(model.transform @ model.mean)[:, None]], axis=1).astype(np.float32)
    tabd, logd, idxd = put(tab), put(logdet), put(index)
    want = ref_plda.transform_ivector(model.mean, model.transform, model.psi, x, counts)
    f32_err = np.max(np.abs(_f32_prepare(model, x, counts, True, False) - want))
    bar = np.maximum(ref_score.delta(d) * np.linalg.norm(want, axis=1), 4 * f32_err)
    psi, nn = model.psi, counts.astype(np.float64)[:, None]
    c, v = nn * psi / (nn * psi + 1.0), 1.0 + psi / (nn * psi + 1.0)
    twin = None
    for la, lb in L.PAIRS:
        fx, ft = fin(x, la), fin(aff, lb)
        fr, fk, fb = fout(n, d, OUT_OF[la]), fout(n, kp, OUT_OF[lb]), vout(n)
        done(lib.xv_plda_prepare(0, fp(fx), fx.ld, n, d, fp(ft), ft.ld, d, 1, 0, second, tp(tabd), tp(logd), tab.shape[0], tp(idxd),
                                 fp(fr), fr.ld, fp(fk), fk.ld, fp(fb), None))
        rows, packed, rho = L.gather(fr), L.gather(fk), L.gather(fb)[0]
        assert np.all(np.isfinite(rows)) and np.all(np.isfinite(packed)) and np.all(np.isfinite(rho)), (la, lb)
        assert np.all(np.max(np.abs(rows - want), axis=1) <= bar), (la, lb)
        er = rows.astype(np.float64)
        logs, quad = 0.5 * (np.log1p(psi)[None, :] - np.log(v)), -0.5 * er * er * c * c / v
        assert np.all(np.abs(rho - (logs.sum(1) + quad.sum(1))) <= 4 * U24 * (np.abs(logs).sum(1) + np.abs(quad).sum(1))), (la, lb)
        assert np.all(np.abs(packed[:, :d] - er * c / v) <= U24 * np.abs(er * c / v) * 1.0001), (la, lb)
        if second:
            w = 0.5 * (1.0 / (1.0 + psi)[None, :] - 1.0 / v)
            assert np.all(np.abs(packed[:, d:] - w) <= U24 * np.abs(w) * 1.0001), (la, lb)
        assert L.intact(fx, x) and L.intact(ft, aff) and L.untouched(fr) and L.untouched(fk) and L.untouched(fb), (la, lb)
        twin = (rows, packed, rho) if twin is None else twin
        assert same_bits(rows, twin[0]) and same_bits(packed, twin[1]) and same_bits(rho, twin[2]), (la, lb)


@pytest.mark.parametrize("d", [33, 150])
def test_plda_prepare_in_place(lib, d):
    """xv_plda_prepare without a transform and rows_dev == x_dev (test side: packed = [y | y^2]) on padded frames, against the
    out-of-place run on tight frames."""
    plda, rng, model, _, _, _ = plda_model(d, "n1")
    n = 37
    u = scaled_rows(rng, n, d)
    tab = np.zeros((1, 4, d))
    tab[0, 0], tab[0, 1] = plda.tables(model.psi, 1)["inv"], 1.0
    tabd = put(tab)
    fx, fr, fk = fin(u, "tight"), fout(n, d, "tight"), fout(n, 2 * d, "tight")
    done(lib.xv_plda_prepare(0, fp(fx), fx.ld, n, d, None, 0, d, 1, 1, 1, tp(tabd), None, 1, None, fp(fr), fr.ld, fp(fk), fk.ld, None, None))
    rows, packed = L.gather(fr), L.gather(fk)
    want = u.astype(np.float64)
    ss = np.sum(want * want * tab[0, 0][None, :], axis=1)
    want = want * np.sqrt(d / ss)[:, None]
    assert np.all(np.isfinite(rows)) and np.all(np.max(np.abs(rows - want), axis=1) <= ref_score.delta(d) * np.linalg.norm(want, axis=1))
    assert np.array_equal(packed[:, :d], rows) and L.intact(fx, u)
    for lay in ("pad4", "pad_odd", "shift1", "shift3"):
        fx, fk = fin(u, lay), fout(n, 2 * d, OUT_OF[lay])
        done(lib.xv_plda_prepare(0, fp(fx), fx.ld, n, d, None, 0, d, 1, 1, 1, tp(tabd), None, 1, None, fp(fx), fx.ld, fp(fk), fk.ld, None, None))
        assert same_bits(L.gather(fx), rows) and same_bits(L.gather(fk), packed), lay
        assert L.untouched(fx) and L.untouched(fk), lay


_plda_sets = {}


def plda_operands(d, kind):
    """Packed operands of a 37 x 129 case from the wrappers (tight), on the host -> dict; made once per (d, kind)."""
    if (d, kind) not in _plda_sets:
        plda, rng, model, xe, xt, counts = plda_model(d, kind)
        e = plda.prepare_enroll(model, xe, num_utts=counts if kind == "mixed" else None)
        t = plda.prepare_test(model, xt)
        assert e.k == (2 * d if kind == "mixed" else d)
        tau = None if e.uniform_n is None else t.tau(e.uniform_n).cpu().numpy()
        _plda_sets[(d, kind)] = dict(a=np.ascontiguousarray(e.packed.cpu().numpy()[:, :e.k]), b=np.ascontiguousarray(t.packed.cpu().numpy()[:, :e.k]),
                                     rho=e.bias.cpu().numpy(), tau=tau, k=e.k, psi=model.psi, counts=counts.astype(np.float64),
                                     erows=e.rows.cpu().numpy(), trows=t.rows.cpu().numpy())
    return _plda_sets[(d, kind)]


def plda_case(d, kind, n, m):
    o = plda_operands(d, kind)
    a, b, rho = o["a"][:n], o["b"][:m], o["rho"][:n]
    tau = None if o["tau"] is None else o["tau"][:m]
    want = ref_plda.llr(o["psi"], o["erows"][:n], o["counts"][:n], o["trows"][:m])
    _, dot_bar, bias_bar = ref_plda.score_bar(a, b, rho, tau)
    return a, b, rho, tau, o["k"], want, dot_bar + bias_bar + 4 * U24 * np.abs(want)


@pytest.mark.parametrize("n,m", SETS)
@pytest.mark.parametrize("d,kind", PLDA_CASES)
def test_plda_matrix_and_pairs(lib, d, kind, n, m):
    """xv_plda_matrix and xv_plda_pairs over packed rows [*, k] (k = d, or 2 d for mixed n) behind lda, ldb: plda.cc in float64
    from the device's prepared rows, the derived bar of tests/test_gpu_plda.py (ref_plda.score_bar)."""
    a, b, rho, tau, k, want, bar = plda_case(d, kind, n, m)
    rng = np.random.default_rng(4000 + d + n)
    npairs = min(n * m, 333)
    ia, ib = rng.integers(0, n, npairs).astype(np.int32), rng.integers(0, m, npairs).astype(np.int32)
    rhod, taud, iad, ibd = put(rho), put(tau), put(ia), put(ib)
    twin = None
    for la, lb in L.PAIRS:
        fa, fb, fo, po = fin(a, la), fin(b, lb), fout(n, m, OUT_OF[la]), vout(npairs)
        done(lib.xv_plda_matrix(0, fp(fa), fa.ld, n, tp(rhod), fp(fb), fb.ld, m, tp(taud), k, fp(fo), fo.ld, None))
        done(lib.xv_plda_pairs(0, fp(fa), fa.ld, n, tp(rhod), fp(fb), fb.ld, m, tp(taud), k, tp(iad), tp(ibd), npairs, fp(po), None))
        got, pairs = L.gather(fo), L.gather(po)[0]
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(pairs)), (la, lb)
        assert np.all(np.abs(got - want) <= bar) and np.all(np.abs(pairs - want[ia, ib]) <= bar[ia, ib]), (la, lb)
        assert L.untouched(fo) and L.untouched(po) and L.intact(fa, a) and L.intact(fb, b), (la, lb)
        twin = (got, pairs) if twin is None else twin
        assert same_bits(got, twin[0]) and same_bits(pairs, twin[1]), (la, lb)


@pytest.mark.parametrize("nbins", [256, 65536])
@pytest.mark.parametrize("n,m", SETS)
@pytest.mark.parametrize("d,kind", PLDA_CASES)
def test_plda_histogram(lib, d, kind, n, m, nbins):
    """xv_plda_histogram: the tight run bracketed by the oracle's counts at the largest bar of the set
    (tests/test_gpu_plda._check_bracket), every other layout pair equal to it count for count."""
    a, b, rho, tau, k, want, bar = plda_case(d, kind, n, m)
    rng = np.random.default_rng(5000 + d + n)
    la_, lb_ = rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 5, m).astype(np.int32)
    eq = la_[:, None] == lb_[None, :]
    lo, hi = (float(np.quantile(want, 0.02)), float(np.quantile(want, 0.995))) if want.size > 1 else (float(want[0, 0]) - 1.0, float(want[0, 0]) + 1.0)
    rhod, taud, lad, lbd = put(rho), put(tau), put(la_), put(lb_)
    twin = None
    for la, lb in L.PAIRS:
        fa, fb = fin(a, la), fin(b, lb)
        hs, hd = hist_frames(nbins)
        done(lib.xv_plda_histogram(0, fp(fa), fa.ld, n, tp(rhod), tp(lad), fp(fb), fb.ld, m, tp(taud), tp(lbd), k, lo, hi, nbins, fp(hs), fp(hd), None))
        cs, cd = counts_of(hs), counts_of(hd)
        assert int(cs.sum()) == int(eq.sum()) and int(cd.sum()) == eq.size - int(eq.sum()), (la, lb)
        assert L.untouched(hs) and L.untouched(hd) and L.intact(fa, a) and L.intact(fb, b), (la, lb)
        if twin is None:
            plda_bracket(cs, np.sort(want[eq]), lo, hi, nbins, float(bar.max()), "same-label")
            plda_bracket(cd, np.sort(want[~eq]), lo, hi, nbins, float(bar.max()), "different-label")
            twin = (cs, cd)
        assert np.array_equal(cs, twin[0]) and np.array_equal(cd, twin[1]), (la, lb)


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("head", ["softmax", "additive_margin_softmax"])
@pytest.mark.parametrize("e", [33, 150])
def test_loss(lib, e, head):
    """xv_loss_prepare_classes (kernel [E, C] behind ldk, class rows behind ldc) and xv_loss_classifier (x behind ldx, the class
    rows behind ldc): the bound of csrc/loss.hip as tests/test_gpu_loss.check asserts it.  The class rows the classifier reads
    are the ones xv_loss_prepare_classes wrote into a frame of that layout."""
    n, c = 37, 129
    rs = np.random.RandomState(1000 * n + 10 * c + e)
    x = (rs.standard_normal((n, e)) * rs.uniform(0.5, 3.0, (n, 1))).astype(np.float32)
    w = (rs.standard_normal((e, c)) * rs.uniform(0.2, 2.0, (1, c))).astype(np.float32)
    bias = rs.standard_normal(c).astype(np.float32) if head == "softmax" else None
    margin, fa = (0.0, 0.0) if head == "softmax" else (0.25, 0.8)
    head_id = 0 if head == "softmax" else 2
    labels = edge_labels(rs, n, c)
    labd, biasd = put(labels), put(bias)

    def classes_in(kernel_layout, layout):
        fk, fc = fin(w, kernel_layout), L.blank(c, e, layout, DEV)[0]
        done(lib.xv_loss_prepare_classes(0, fp(fk), fk.ld, e, c, int(head != "softmax"), fp(fc), fc.ld, None))
        assert L.intact(fk, w) and L.untouched(fc), (kernel_layout, layout)
        return fc

    twin_c = None
    for lay in L.LAYOUTS:
        rows = L.gather(classes_in(lay, OUT_OF[lay]))
        assert np.all(np.isfinite(rows)), lay
        if head == "softmax":
            assert np.array_equal(rows, w.T), lay
        twin_c = rows if twin_c is None else twin_c
        assert same_bits(rows, twin_c), lay

    import torch
    need = int(lib.xv_loss_workspace(n, c))
    twin = None
    for la, lb in L.PAIRS:
        fx, fc = fin(x, la), classes_in("tight", lb)
        assert same_bits(L.gather(fc), twin_c), (la, lb)
        out = [vout(n), vout(n), vout(n), vout(n, np.int32)]
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        done(lib.xv_loss_classifier(0, fp(fx), fx.ld, n, e, tp(labd), fp(fc), fc.ld, c, tp(biasd), head_id, margin, fa, fp(out[0]),
                                    fp(out[1]), fp(out[2]), fp(out[3]), tp(ws), need, None))
        got = dict(loss=L.gather(out[0])[0], target_logit=L.gather(out[1])[0], lse=L.gather(out[2])[0], top1=L.gather(out[3])[0])
        assert all(np.all(np.isfinite(got[k])) for k in ("loss", "target_logit", "lse")), (la, lb)
        loss_check(got, x, labels, w, bias, head, margin, fa, "layouts %s %s" % (la, lb))
        assert all(L.untouched(o) for o in out) and L.intact(fx, x) and same_bits(L.gather(fc), twin_c) and L.untouched(fc), (la, lb)
        twin = got if twin is None else twin
        assert all(same_bits(got[k], twin[k]) for k in got), (la, lb)


# ------------------------------------------------------------------------------------------------ back-end statistics
@pytest.mark.parametrize("d", [3, 17, 70])
def test_gram(lib, d):
    """xv_gram_f64 (float rows) and xv_gram_f64_rows64 (double rows, offsets counted in elements) with c_dev and w_dev given:
    (n + 16) 2^-53 sum |w y y| (tests/test_gpu_backend._oracle); G == G^T; the [d, d] output has no leading dimension, so it
    sits tight in a canary frame whose slack must stay as it is."""
    import torch
    rng = np.random.default_rng(100 * d + 301)
    n = 301
    x32 = (rng.standard_normal((n, d)) * np.exp2(rng.integers(-3, 4, (1, d))) + 0.5).astype(np.float32)
    x64 = rng.standard_normal((n, d)) + 1.0 / 3.0
    c, w = rng.standard_normal(d) * 0.3 + 0.5, rng.uniform(0.5, 3.0, n)
    cd, wd = put(c), put(w)
    need = int(lib.xv_gram_f64_workspace(n, d))
    for x, fn in ((x32, lib.xv_gram_f64), (x64, lib.xv_gram_f64_rows64)):
        want, bar = gram_oracle(x, d, c, w)
        twin = None
        for lay in L.LAYOUTS:
            fx, fg = fin(x, lay), fout(d, d, "tight", np.float64)
            ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=DEV)
            done(fn(0, fp(fx), fx.ld, n, d, tp(cd), tp(wd), fp(fg), tp(ws), need, None))
            g = L.gather(fg)
            assert np.all(np.isfinite(g)), (x.dtype, lay)
            assert np.all(np.abs(g - want) <= bar) and np.array_equal(g, g.T), (x.dtype, lay)
            assert L.untouched(fg) and L.intact(fx, x), (x.dtype, lay)
            twin = g if twin is None else twin
            assert same_bits(g, twin), (x.dtype, lay)


def test_class_mean(lib):
    """xv_class_mean_f64: float rows behind ldx, double means behind ldo.  The bar of tests/test_gpu_backend.test_class_mean:
    (n_s + 2) 2^-53 sum |x|, and with c one more rounding, 2^-53 (|mean| + |c|)."""
    rng = np.random.default_rng(9)
    n, d = 301, 17
    x = (rng.standard_normal((n, d)) * 4.0 + 1.0).astype(np.float32)
    sizes = [1, 7, 0, 33, 64, 150, 2, 0, 0]
    index = rng.permutation(n)[:sum(sizes)].astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    c = rng.standard_normal(d)
    offd, idxd, cd = put(off), put(index), put(c)
    twin = None
    for lay in L.LAYOUTS:
        fx, fo = fin(x, lay), fout(len(sizes), d, OUT_OF[lay], np.float64)
        done(lib.xv_class_mean_f64(0, fp(fx), fx.ld, n, d, tp(offd), tp(idxd), len(sizes), tp(cd), fp(fo), fo.ld, None))
        got = L.gather(fo)
        assert np.all(np.isfinite(got)) and L.untouched(fo) and L.intact(fx, x), lay
        for s, k in enumerate(sizes):
            if k == 0:
                assert np.all(got[s] == 0.0), lay
                continue
            rows = x[index[off[s]:off[s + 1]]].astype(np.float64)
            bar = (k + 2) * U53 * np.abs(rows).sum(axis=0) + U53 * (np.abs(rows.sum(axis=0) / k) + np.abs(c))
            assert np.all(np.abs(got[s] - (rows.sum(axis=0) / k - c)) <= bar), (lay, s)
        twin = got if twin is None else twin
        assert same_bits(got, twin), lay


# ------------------------------------------------------------------------------------------------ post-step
@pytest.mark.parametrize("d", DIMS)
def test_length_normalize(lib, d):
    """xv_length_normalize against oracle/ref_post.py at the tolerance of tests/test_gpu_launcher.py, out of place and in place."""
    rs = np.random.RandomState(3 + d)
    n = 37
    x = (rs.standard_normal((n, d)) * 7).astype(np.float32)
    x[5] = 0.0
    for scaleup in (0, 1):
        want = ref_post.normalize_length(x, bool(scaleup))
        twin = None
        for lay in L.LAYOUTS:
            fx, fo = fin(x, lay), fout(n, d, OUT_OF[lay])
            done(lib.xv_length_normalize(0, fp(fx), fx.ld, n, d, scaleup, fp(fo), fo.ld, None))
            got = L.gather(fo)
            assert np.all(np.isfinite(got)) and np.array_equal(got[5], x[5]), lay
            np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-9)
            assert L.untouched(fo) and L.intact(fx, x), lay
            twin = got if twin is None else twin
            assert same_bits(got, twin), lay
        for lay in ("pad4", "pad_odd", "shift1", "shift3"):
            fx = fin(x, lay)
            done(lib.xv_length_normalize(0, fp(fx), fx.ld, n, d, scaleup, fp(fx), fx.ld, None))
            assert same_bits(L.gather(fx), twin) and L.untouched(fx), lay


@pytest.mark.parametrize("d", DIMS)
def test_speaker_mean(lib, d):
    """xv_speaker_mean: bit-exact against oracle/ref_post.py (the same float32 adds in the same order); an empty speaker gets zeros."""
    rs = np.random.RandomState(5 + d)
    n = 37
    x = (rs.standard_normal((n, d)) * 7).astype(np.float32)
    off = np.array([0, 1, 8, 8, 30], np.int32)
    index = rs.permutation(n)[:30].astype(np.int32)
    keys = ["u%d" % i for i in range(n)]
    spk2utt = [("s%d" % s, [keys[i] for i in index[off[s]:off[s + 1]]]) for s in range(4)]
    means = dict(ref_post.speaker_mean(dict(zip(keys, x)), spk2utt)[0])
    want = np.stack([means.get("s%d" % s, np.zeros(d, np.float32)) for s in range(4)])
    offd, idxd = put(off), put(index)
    for lay in L.LAYOUTS:
        fx, fo = fin(x, lay), fout(4, d, OUT_OF[lay])
        done(lib.xv_speaker_mean(0, fp(fx), fx.ld, d, tp(offd), tp(idxd), 4, fp(fo), fo.ld, None))
        got = L.gather(fo)
        assert np.array_equal(got, want), lay
        assert L.untouched(fo) and L.intact(fx, x), lay


# ------------------------------------------------------------------------------------------------ front-end
LENS = [1, 24, 301, 40]


def test_frontend_cmn_select(lib):
    """xv_frontend_cmn_select with the features behind ld: the comparison of tests/test_frontend.py against oracle/ref_frontend.py
    (window 51, centred)."""
    import torch
    rng = np.random.default_rng(5)
    dim, window = 30, 51
    feats = [(rng.standard_normal((t, dim)) * 4 + rng.standard_normal(dim) * 10).astype(np.float32) for t in LENS]
    vads = [(rng.random(t) < 0.7).astype(np.float32) for t in LENS]
    vads[0][:] = 0
    offsets = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    src = np.concatenate([np.flatnonzero(v != 0).astype(np.int32) + offsets[b] for b, v in enumerate(vads)])
    want = np.concatenate([ref_frontend.select_voiced(ref_frontend.sliding_cmn(f, window, True, 100), v) for f, v in zip(feats, vads)])
    packed = np.concatenate(feats)
    offd, srcd = put(offsets), put(src)
    twin = None
    for lay in L.LAYOUTS:
        fx, fo = fin(packed, lay), fout(src.shape[0], dim, "tight")
        scratch = torch.empty((packed.shape[0] + len(LENS)) * dim, dtype=torch.float64, device=DEV)
        done(lib.xv_frontend_cmn_select(0, fp(fx), fx.ld, dim, tp(offd), len(LENS), tp(srcd), src.shape[0], window, 1, 100, tp(scratch),
                                        fp(fo), None))
        got = L.gather(fo)
        assert got.shape == want.shape and np.all(np.isfinite(got)), lay
        np.testing.assert_allclose(got, want, atol=2e-6 * np.abs(want).max())
        assert L.untouched(fo) and L.intact(fx, packed), lay
        twin = got if twin is None else twin
        assert same_bits(got, twin), lay


def test_vad_energy(lib):
    """xv_vad_energy with the log energies in column 0 behind ld, every other column poison: equal to tests/helpers/ref_mfcc.vad
    on every frame (no frame lies near the threshold, from the oracle alone)."""
    rng = np.random.default_rng(6)
    vo = ref_mfcc.VAD_VOXCELEB
    # a loud frame in eight: with a context of 2 and a proportion of 0.12 about half of the frames come out voiced
    utts = [np.where(rng.random(t) < 0.125, rng.uniform(14.0, 20.0, t), rng.uniform(0.0, 4.0, t)).astype(np.float32)[:, None] for t in LENS]
    for f in utts:
        assert np.abs(f[:, 0] - ref_mfcc.vad_threshold(f, vo)).min() > 1e-3
    want = np.concatenate([ref_mfcc.vad(f, vo) for f in utts])
    assert 0.2 < want.mean() < 0.8
    packed = np.concatenate(utts)
    offsets = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    offd = put(offsets)
    for lay in L.LAYOUTS:
        fx, fo = fin(packed, lay), vout(packed.shape[0])
        done(lib.xv_vad_energy(0, fp(fx), fx.ld, tp(offd), len(LENS), vo["vad_energy_threshold"], vo["vad_energy_mean_scale"],
                               vo["vad_frames_context"], vo["vad_proportion_threshold"], fp(fo), None))
        assert np.array_equal(L.gather(fo)[0], want), lay
        assert L.untouched(fo) and L.intact(fx, packed), lay


# ------------------------------------------------------------------------------------------------ xv_forward
@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x3", "f16f6"])
def test_forward_feature_stride(precision):
    """xv_forward through Trainer.predict_packed with feat_ld = 32 for a 30-dimensional network, the two extra columns NaN:
    against oracle/ref_numpy at the usual 1e-4, and bit-identical to the run on the 30-column tensor."""
    import torch
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import synth
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params = dict(synth.TDNN_STAT_PARAMS, num_nodes_pooling_layer=160, num_nodes_last_layer=48)
    weights = synth.synth_weights(params, 30, seed=3, channels=64)
    lens = [15, 64, 129]
    utts = synth.synth_features(len(lens), lens, 30, seed=5)
    packed = np.concatenate(utts, axis=0).astype(np.float32)
    wide = np.concatenate([packed, np.full((packed.shape[0], 2), np.nan, np.float32)], axis=1)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    tr = Trainer(Params(**params), None, 30, single_cpu=True, device=0, precision=precision)
    tr.build("predict")
    tr.load_weights(weights)
    plain = tr.predict_packed(torch.from_numpy(packed).cuda(), offsets).cpu().numpy()
    wided = torch.from_numpy(wide).cuda()
    got = tr.predict_packed(wided, offsets).cpu().numpy()
    assert np.all(np.isfinite(got))
    for i, u in enumerate(utts):
        ref = ref_numpy.predict(u, weights, params, 30)
        rel = float(np.linalg.norm(got[i] - ref) / np.linalg.norm(ref))
        print("forward feat_ld 32 %s T=%d: rel-L2 %.3e" % (precision, lens[i], rel))
        assert rel <= 1e-4, (i, rel)
    assert same_bits(got, plain)
    assert wided.cpu().numpy().tobytes() == wide.tobytes()               # the features are never written
    tr.close()
