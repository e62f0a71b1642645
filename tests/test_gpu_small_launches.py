"""GPU: the small launches around the GEMMs of a forward, through the C ABI.

* feature staging + per-utterance range guard in one pass (csrc/pool.hip, feat_stage_sb_kernel), in both of its grids (one
  workgroup per utterance up to 512 frames; 128-row chunks + feat_utt_fold_kernel beyond): utterance lengths around the
  kernel's 256-row pass and 128-row chunk, feature matrices with a row stride of 30 and 33 floats and a base pointer that is only 4-byte aligned
  (the 8-byte loads and the scalar fallback), the guard's answers through both read-outs (xv_flags_async: the snapshot kernel;
  xv_check_overflow: the host loop), their reset, and that an utterance is judged in the forward that staged it;
* the finalize of the fused statistics pooling (pool_finalize_kernel): utterance boundaries at, before and behind a 64-row slot
  edge, the shortest utterance and a long one;
* the segment-level layers in one launch (csrc/gemm_f32.hip, gemm_f32_seg_kernel): B = 1, 2, 33, 256.
Tolerance as in test_gpu_parity.py: relative L2 <= 1e-4 against the float64 oracle."""
import numpy as np
import pytest

from oracle import ref_numpy

pytestmark = pytest.mark.gpu
TOL = 1e-4
CHUNK = 128                     # kStageRows
SINGLE = 512                    # kStageSingleRows: up to here one workgroup stages a whole utterance, 256 rows per pass
PRECISIONS = ["f32", "bf16x3", "f16x3", "f16f6"]


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(b.shape)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _trainer(params, weights, dim, precision, **kw):
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    tr = Trainer(Params(**dict(params)), None, dim, single_cpu=True, device=0, precision=precision, **kw)
    tr.build("predict")
    tr.load_weights(weights)
    return tr


@pytest.fixture(scope="module")
def stat_model():
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.TDNN_STAT_PARAMS)
    return params, synth.synth_weights(params, 30, seed=0)


def _packed(utts, ld, misalign):
    """The utterances back to back as a CUDA tensor [frames, ld]; columns 30.. hold 1e9 (never to be read: in the fp16 formats they
    would raise the overflow flag); misalign: the matrix starts one float behind an allocation boundary."""
    import torch
    rows = np.concatenate(utts).astype(np.float32)
    host = np.full((rows.shape[0], ld), 1.0e9, np.float32)
    host[:, :rows.shape[1]] = rows
    flat = torch.empty(host.size + 1, dtype=torch.float32, device="cuda")
    view = flat[1:] if misalign else flat[:-1]
    view.copy_(torch.from_numpy(host.reshape(-1)))
    dev = view.view(host.shape)
    assert dev.is_contiguous() and (dev.data_ptr() % 8 == 4) == bool(misalign)
    return dev


# ------------------------------------------------------------------------------------------------ staging
STAGE_LENS = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 44, 15, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, SINGLE, SINGLE + 1]
STAGE_GRIDS = {"single": slice(0, 9), "chunked": slice(0, 10)}      # the longest utterance picks the grid


@pytest.fixture(scope="module")
def stage_case(stat_model):
    from tf_kaldi_speaker_amd import synth
    params, weights = stat_model
    utts = synth.synth_features(len(STAGE_LENS), STAGE_LENS, 30, seed=21)
    refs = [ref_numpy.predict(u, weights, params, 30, node="tdnn1_relu") for u in utts]
    return utts, refs


@pytest.mark.parametrize("grid", ["single", "chunked"])
@pytest.mark.parametrize("precision", ["f16f6", "f16x3", "bf16x3"])
def test_staging_layouts(stat_model, stage_case, precision, grid):
    """tdnn1_relu behind the staging pass for every (row stride, alignment) form of the feature matrix."""
    params, weights = stat_model
    utts, refs = stage_case[0][STAGE_GRIDS[grid]], stage_case[1][STAGE_GRIDS[grid]]
    offs = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int32)
    out_offs = np.concatenate([[0], np.cumsum([r.shape[-2] for r in refs])])
    tr = _trainer(params, weights, 30, precision, range_fallback=False)
    first = None
    for ld in (30, 33):
        for misalign in (0, 1):
            feats = _packed(utts, ld, misalign)
            got = tr.predict_packed(feats, offs, "tdnn1_relu").cpu().numpy()
            assert tr.check_overflow() == 0, (precision, ld, misalign)
            assert got.shape[0] == out_offs[-1]
            for i, ref in enumerate(refs):
                err = _rel(got[out_offs[i]:out_offs[i + 1]], ref)
                print("staging %s ld %d misalign %d utt %d: %.3e" % (precision, ld, misalign, i, err))
                assert err <= TOL, (precision, ld, misalign, i, err)
            if first is None:
                first = got
            assert np.array_equal(got, first), (precision, ld, misalign, "the forms stage different values")
    tr.close()


def _guard_cases(grid):
    from tf_kaldi_speaker_amd import synth
    lens = [200 if grid == "single" else SINGLE + 88, 3 * CHUNK - 60, 150]
    base = synth.synth_features(len(lens), lens, 30, seed=22)            # N(0, 1)
    cases = {}
    z = [u.copy() for u in base]
    z[1][:] = 0.0
    cases["all-zero utterance"] = (z, 0)
    s = [u.copy() for u in base]
    s[1] *= 2.0 ** -12                                                     # everything below 2^-8 ...
    s[1][-1, 17] = 1.0                                                     # ... but one value in the last row (third chunk)
    cases["one normal value in the last chunk"] = (s, 0)
    t = [u.copy() for u in base]
    t[1] = np.clip(t[1], -3.0, 3.0) * np.float32(2.0 ** -10)         # largest magnitude 3 * 2^-10 < 2^-8
    cases["utterance at 2^-10"] = (t, 2)
    o = [u.copy() for u in base]
    o[2][149, 29] = -1.0e5
    cases["beyond 65504"] = (o, 1)
    return lens, cases


def _read(tr, how, host_flags):
    """One read-out of the guard: the snapshot kernel (xv_flags_async into pinned memory) or the host loop (xv_check_overflow)."""
    import torch
    if how == "xv_check_overflow":
        return tr.check_overflow()
    tr.flags_async(host_flags)
    torch.cuda.synchronize()
    return tr.decode_flags(host_flags)


@pytest.mark.parametrize("grid", ["single", "chunked"])
@pytest.mark.parametrize("how", ["xv_flags_async", "xv_check_overflow"])
@pytest.mark.parametrize("precision", ["f16f6", "f16x3"])
def test_guard_answers_and_reset(stat_model, precision, how, grid):
    """What the guard reports, one forward per read-out, through ONE kind of read-out only (so that nothing but that read-out and
    the forward itself clears anything), the cases twice in a row and each followed by a different one: a word of the previous
    forward that survived -- a per-utterance maximum, the sticky small-utterance word, the overflow flag -- changes an answer
    (the 1.0 of 'one normal value' would hide the utterance at 2^-10 behind it; its code 2 would show in 'beyond 65504' and in
    the clean cases)."""
    import torch
    params, weights = stat_model
    lens, cases = _guard_cases(grid)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    tr = _trainer(params, weights, 30, precision, range_fallback=False)
    host_flags = torch.zeros(2, dtype=torch.int32).pin_memory()
    order = ["one normal value in the last chunk", "utterance at 2^-10", "all-zero utterance", "beyond 65504"]
    for name in order + order:
        utts, want = cases[name]
        tr.predict_packed(_packed(utts, 30, 0), offs, "tdnn1_relu")
        assert _read(tr, how, host_flags) == want, (precision, name, how, host_flags.tolist())
    assert _read(tr, how, host_flags) == 0                 # nothing staged since the last read-out
    tr.close()


@pytest.mark.parametrize("grid", ["single", "chunked"])
@pytest.mark.parametrize("how", ["xv_flags_async", "xv_check_overflow"])
@pytest.mark.parametrize("precision", ["f16f6", "f16x3"])
def test_guard_is_decided_per_forward(stat_model, precision, how, grid):
    """Code 2 means "an utterance staged since the last clear ...": forward A has utterance 1 at 2^-10, forward B -- same batch
    size, so the same per-utterance words -- is all N(0, 1), then ONE read-out: it must still report A's utterance.  Then a ragged
    pair with another batch size in between, and the bf16 split, which has nothing to report."""
    import torch
    from tf_kaldi_speaker_amd import synth
    params, weights = stat_model
    lens, cases = _guard_cases(grid)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    small, normal = cases["utterance at 2^-10"][0], synth.synth_features(len(lens), lens, 30, seed=25)
    tr = _trainer(params, weights, 30, precision, range_fallback=False)
    host_flags = torch.zeros(2, dtype=torch.int32).pin_memory()
    tr.predict_packed(_packed(small, 30, 0), offs, "tdnn1_relu")
    tr.predict_packed(_packed(normal, 30, 0), offs, "tdnn1_relu")
    assert _read(tr, how, host_flags) == 2, (precision, how, "small utterance, then a normal batch of the same size")
    tr.predict_packed(_packed(normal, 30, 0), offs, "tdnn1_relu")
    assert _read(tr, how, host_flags) == 0, (precision, how, "the read-out did not clear")
    tr.predict_packed(_packed(small, 30, 0), offs, "tdnn1_relu")
    tr.predict_packed(_packed(normal[1:2], 30, 0), offs[1:3] - offs[1], "tdnn1_relu")   # B = 1 behind B = 3 (always the single grid)
    tr.predict_packed(_packed(normal, 30, 0), offs, "tdnn1_relu")
    assert _read(tr, how, host_flags) == 2, (precision, how, "small utterance, then other batch sizes")
    tr.close()
    tr = _trainer(params, weights, 30, "bf16x3")          # the bf16 split has the full fp32 exponent range: nothing to report
    tr.predict_packed(_packed(small, 30, 0), offs, "tdnn1_relu")
    assert tr.check_overflow() == 0
    tr.close()


# ------------------------------------------------------------------------------------------------ finalize
# pooled rows = frames - 14: boundaries at row 64 (a slot edge), 127 (one before), 193 (one behind), 194 (the shortest utterance),
# then an utterance of 600 rows = 10 or 11 slots
POOL_LENS = [64 + 14, 63 + 14, 66 + 14, 15, 600 + 14]


@pytest.mark.parametrize("precision", ["f32", "f16f6"])
def test_pool_finalize_slot_edges(stat_model, precision):
    from tf_kaldi_speaker_amd import synth
    params, weights = stat_model
    utts = synth.synth_features(len(POOL_LENS), POOL_LENS, 30, seed=23)
    tr = _trainer(params, weights, 30, precision)
    got = np.asarray(tr.predict_list(utts, node="pooling"))
    again = np.asarray(tr.predict_list(utts, node="pooling"))
    tr.close()
    assert np.array_equal(got, again)
    for i, u in enumerate(utts):
        ref = ref_numpy.predict(u, weights, params, 30, node="pooling")
        err = _rel(got[i], ref)
        print("pooling %s utt %d (%d frames): %.3e" % (precision, i, POOL_LENS[i], err))
        assert err <= TOL, (precision, i, err)


# ------------------------------------------------------------------------------------------------ segment GEMM
SEG_T = 20


@pytest.fixture(scope="module")
def seg_case(stat_model):
    from tf_kaldi_speaker_amd import synth
    params, weights = stat_model
    feats = np.stack(synth.synth_features(256, SEG_T, 30, seed=24))
    _, ep = ref_numpy.entire_network(feats, weights, params)
    nodes = [n for n in ("tdnn6_dense", "output") if n in ep]
    return feats, {n: np.asarray(ep[n], dtype=np.float64) for n in nodes}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("batch", [1, 2, 33, 256])
def test_segment_layers_one_launch(stat_model, seg_case, precision, batch):
    import torch
    params, weights = stat_model
    feats, refs = seg_case
    dev = torch.from_numpy(feats[:batch].reshape(batch * SEG_T, 30)).cuda()
    offs = np.arange(batch + 1, dtype=np.int32) * SEG_T
    tr = _trainer(params, weights, 30, precision)
    for node, ref in refs.items():
        a = tr.predict_packed(dev, offs, node).cpu().numpy()
        b = tr.predict_packed(dev, offs, node).cpu().numpy()
        assert np.array_equal(a, b), (precision, batch, node, "not bit-identical on repetition")
        assert a.shape == ref[:batch].shape
        errs = [_rel(a[i], ref[i]) for i in range(batch)]
        print("segment %s B %d %s: max rel-L2 %.3e" % (precision, batch, node, max(errs)))
        assert max(errs) <= TOL, (precision, batch, node, max(errs))
    assert tr.check_overflow() == 0
    tr.close()
