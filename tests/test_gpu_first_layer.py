"""GPU: the first TDNN layer on the walking-workgroup kernel (csrc/gemm_first.hip, xv_set_option "first_walk").

The kernel computes the sums of the tile kernel (csrc/gemm_bf16x3.hip) in the same order, so everything here is either the
float64 oracle at the bar of test_gpu_parity.py (relative L2 <= 1e-4) or bit-for-bit equality with the tile kernel's route.
The tests set first_walk 2 (the kernel for every shape it takes), so that its three instantiations run under every precision:

* small ragged batch [5, 132, 300, 129, 7]: one output frame, a tile edge inside an utterance, tiles across utterance borders,
  a partial last tile; nodes tdnn1_relu (the layer writes the requested fp32 value) and tdnn2_relu (it writes the operand format
  of the next layer: split-blocked rows, or the two-unit block format under f16f6).  tdnn2_relu needs more than 8 frames, so for
  that node the two shortest utterances are 9 frames long, again one output frame;
* the walking shape, 112 x 300 frames = 263 M tiles x 4 N tiles on at most two workgroups per CU: with 256 CUs some workgroups
  walk three tiles, which uses both slab-buffer hand-overs (0 -> 1 and 1 -> 0).  The oracle is too slow for it; the tile kernel
  is the reference.  Repeats, hipGraph replay and a workspace full of 0xFF (a slab row read outside the tile kernel's footprint
  would meet NaN patterns) must all give the same bytes;
* the shapes the kernel refuses (here a 40-dim input: two 32-channel blocks) and first_walk 0 stay on the tile kernel."""
import functools

import numpy as np
import pytest

from oracle import ref_numpy

pytestmark = pytest.mark.gpu
TOL = 1e-4
SMALL_LENS = [5, 132, 300, 129, 7]
MIN_LEN = {"tdnn1_relu": 5, "tdnn2_relu": 9}          # context + 1 of the node: one output frame
WALK_B, WALK_T = 112, 300


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(b.shape)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@functools.lru_cache(maxsize=None)
def _model(dim=30, channels=512):
    from tf_kaldi_speaker_amd import synth
    params = dict(synth.TDNN_STAT_PARAMS)
    return params, synth.synth_weights(params, dim, seed=5, channels=channels)


def _trainer(precision, dim=30, channels=512):
    """first_walk 2: the walking kernel for every shape it takes (the default, 1, takes it only where the layer writes the two-unit
    block format: f16f6 with a later node requested)."""
    from tf_kaldi_speaker_amd.params import Params
    from tf_kaldi_speaker_amd.trainer import Trainer
    params, weights = _model(dim, channels)
    tr = Trainer(Params(**dict(params)), None, dim, single_cpu=True, device=0, precision=precision)
    tr.build("predict")
    tr.load_weights(weights)
    tr.set_option("first_walk", 2)
    return tr


@functools.lru_cache(maxsize=None)
def _small(node, dim=30, channels=512):
    """(packed features on the device, offsets, float64 oracle of the packed output), computed once per node."""
    import torch
    from tf_kaldi_speaker_amd import synth
    params, weights = _model(dim, channels)
    lens = [max(n, MIN_LEN[node]) for n in SMALL_LENS]
    utts = synth.synth_features(len(lens), lens, dim, seed=61)
    ref = np.concatenate([ref_numpy.predict(u, weights, params, dim, node=node).reshape(-1, channels) for u in utts])
    ref.setflags(write=False)
    feats = torch.from_numpy(np.concatenate(utts)).cuda()
    return feats, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), ref


@functools.lru_cache(maxsize=None)
def _walk_batch():
    import torch
    from tf_kaldi_speaker_amd import synth
    feats = torch.from_numpy(np.concatenate(synth.synth_features(WALK_B, WALK_T, 30, seed=62))).cuda()
    return feats, np.arange(WALK_B + 1, dtype=np.int32) * WALK_T


def _run(tr, feats, offs, node):
    import torch
    out = tr.predict_packed(feats, offs, node)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _walked_tiles():
    """The most M tiles a workgroup of the walking kernel takes at the walking shape (the launcher's arithmetic: two workgroups
    per CU, not more than the tile count, a multiple of the 4 N tiles)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_mt = (WALK_B * WALK_T - 4 + 127) // 128
    grid = min(2 * cus, n_mt * 4)
    grid -= grid % 4
    return -(-n_mt // (grid // 4)), n_mt, grid


def _need_three_tiles():
    walks, n_mt, grid = _walked_tiles()
    if walks < 3:
        pytest.skip("%d M tiles on a grid of %d workgroups: no workgroup walks three tiles on this device" % (n_mt, grid))


@pytest.mark.parametrize("precision", ["f16f6", "f16x3", "bf16x3"])
@pytest.mark.parametrize("node", ["tdnn1_relu", "tdnn2_relu"])
def test_small_shapes_against_the_oracle(node, precision):
    feats, offs, ref = _small(node)
    tr = _trainer(precision)
    walk = _run(tr, feats, offs, node)
    tr.set_option("first_walk", 0)
    tile = _run(tr, feats, offs, node)
    tr.close()
    err = _rel(walk, ref)
    print("%s %s: rel-L2 %.3e (rows %d)" % (node, precision, err, ref.shape[0]))
    assert walk.shape == ref.shape
    assert err <= TOL, (node, precision, err)
    assert np.array_equal(walk.view(np.uint32), tile.view(np.uint32)), (node, precision, "first_walk 2 against 0")


@pytest.mark.parametrize("precision", ["f16f6", "bf16x3"])
@pytest.mark.parametrize("node", ["tdnn2_relu", "tdnn6_dense"])
def test_walking_shape_bit_for_bit(node, precision):
    _need_three_tiles()
    feats, offs = _walk_batch()
    tr = _trainer(precision)
    a = _run(tr, feats, offs, node)
    b = _run(tr, feats, offs, node)
    tr.set_option("first_walk", 1)
    default = _run(tr, feats, offs, node)
    tr.set_option("first_walk", 0)
    tile = _run(tr, feats, offs, node)
    tr.close()
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (node, precision, "two repeats")
    assert np.array_equal(a.view(np.uint32), default.view(np.uint32)), (node, precision, "first_walk 2 against the default")
    assert np.array_equal(a.view(np.uint32), tile.view(np.uint32)), (node, precision, "first_walk 2 against 0")


def test_graph_replay_at_the_walking_shape():
    import torch
    _need_three_tiles()
    feats, offs = _walk_batch()
    tr = _trainer("f16f6")
    stream = _run(tr, feats, offs, "tdnn2_relu")
    graph, out = tr.capture_graph(feats, offs, "tdnn2_relu")
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replay = out.cpu().numpy()
    del graph
    tr.release_graphs()
    tr.close()
    assert np.array_equal(replay.view(np.uint32), stream.view(np.uint32))


@pytest.mark.parametrize("precision", ["f16f6", "bf16x3"])
def test_poisoned_workspace_at_the_walking_shape(precision):
    _need_three_tiles()
    feats, offs = _walk_batch()
    tr = _trainer(precision)
    _run(tr, feats, offs, "tdnn6_dense")                  # the workspace exists
    tr._ws.fill_(255)
    walk = _run(tr, feats, offs, "tdnn6_dense")
    tr.set_option("first_walk", 0)
    tr._ws.fill_(255)
    tile = _run(tr, feats, offs, "tdnn6_dense")
    tr.close()
    assert not np.isnan(walk).any()
    assert np.array_equal(walk.view(np.uint32), tile.view(np.uint32)), precision


def test_fallback_routes_pass_the_oracle():
    # first_walk 0: the tile kernel, on its own against the oracle
    feats, offs, ref = _small("tdnn1_relu")
    tr = _trainer("f16f6")
    tr.set_option("first_walk", 0)
    tile = _run(tr, feats, offs, "tdnn1_relu")
    tr.close()
    assert _rel(tile, ref) <= TOL
    # 40-dim input: two 32-channel blocks per frame, which the walking kernel does not take
    feats, offs, ref = _small("tdnn2_relu", 40, 128)
    tr = _trainer("bf16x3", 40, 128)
    got = _run(tr, feats, offs, "tdnn2_relu")
    tr.set_option("first_walk", 0)
    same = _run(tr, feats, offs, "tdnn2_relu")
    tr.close()
    assert _rel(got, ref) <= TOL
    assert np.array_equal(got.view(np.uint32), same.view(np.uint32))
