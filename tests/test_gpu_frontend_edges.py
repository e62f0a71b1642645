"""GPU: the parts of mfcc_kernel, fbank_kernel and vad_kernel (csrc/mfcc.hip) that the eight-utterance batches of
tests/test_gpu_mfcc.py and tests/test_gpu_fbank.py never reach, against the float64 oracles tests/helpers/ref_mfcc.py and
tests/helpers/ref_fbank.py.

a. Every option and frame size the kernels accept but those tests do not set (mfcc_cases.EDGE_CONFIGS and FBANK_EDGE_CONFIGS),
   written into NaN-filled outputs: every row written, nothing beyond the feature columns touched, two runs the same bits.
b. A batch with 1.5 times as many tiles as the launch has workgroups, so that workgroups take a second tile (the barrier that
   guards `span`, the idle-tile `continue`, the binary search over many utterances), bit for bit against the same utterances in
   slices of 64.
c. Full-scale input: a +-32767/-32768 square wave, all -32768, alternating +-1.
d. vad_kernel on hand-made energies: empty utterances, a context wider than the utterance, more than 256 and 512 frames, energies
   equal to the threshold, and the three window counts at which Kaldi's float comparison and a double comparison disagree.

Feature tolerance, as in tests/test_gpu_mfcc.py: e32 is the largest absolute difference between the oracle's float32 mode and its
float64 mode on the same batch; the GPU must be within 4 x e32 of the float64 oracle.  Linear fbank output is compared after
log(max(., FLT_EPSILON)).  Every test prints e32 and the GPU's error.

Measured on an MI355X (256 CUs); the figures are the same for both leading dimensions of a case:
  case                     frames   e32        GPU error   (side energy)   bound 4 x e32
  a mfcc  wide16ms             87   2.801e-05  8.689e-05                   1.120e-04    coefficient 0 (from the DCT) 8.689e-05, others 3.391e-05
  a mfcc  min129             2964   1.005e-05  1.275e-05                   4.019e-05
  a mfcc  full512              46   1.173e-04  8.566e-05                   4.692e-04    coefficient 0 (the windowed energy) 1.522e-06
  a mfcc  n257                292   9.534e-05  7.678e-05                   3.813e-04
  a fbank amp256               87   1.416e-05  1.336e-05   2.447e-06       5.666e-05
  a fbank lin512               46   5.927e-05  3.992e-05   1.522e-06       2.371e-04
  b mfcc  voxceleb          18415   1.273e-04  9.211e-05                   5.094e-04    2030 utterances, 3180 tiles on 2048 workgroups
  b mfcc  kaldi_defaults    16965   9.317e-05  8.283e-05                   3.727e-04    2030 utterances, 3090 tiles on 2048 workgroups
  b fbank v3                18415   2.677e-05  2.156e-05   2.402e-06       1.071e-04
  b fbank kaldi_defaults    16965   1.708e-05  1.516e-05   2.454e-06       6.834e-05
  c square wave                25   4.961e-05  4.091e-05                   1.985e-04
  c all -32768                 25   2.322e-05  5.206e-07                   9.289e-05
  c alternating +-1            25   1.602e-02  1.208e-02                   6.408e-02    every mel energy is leakage: the tone sits at the Nyquist frequency, above --high-freq
  c the three as one batch     75   1.602e-02  1.208e-02                   6.408e-02
No case came out beyond its bound, so no second float32 restatement was needed.  The closest is coefficient 0 of wide16ms, a sum
of 64 log mel energies of which one is the floor of the filter without an FFT bin."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mfcc_cases  # noqa: E402
import ref_fbank  # noqa: E402
import ref_mfcc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
GRID_FACTOR, RUN = 8, 16          # csrc/mfcc.hip: the launch has 8 workgroups per CU (front_upload), a tile is kRun = 16 frames
_ref = {}


def _pack(utts):
    import torch
    off = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int64)
    return torch.from_numpy(np.concatenate(utts).astype(np.int16)).cuda(), off


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _mfcc_into_nan(h, wave_dev, soff, ld):
    """Mfcc.compute into a freshly NaN-filled [frames, ld] tensor."""
    from tf_kaldi_speaker_amd import mfcc as M
    _, foff = M.packed_offsets(h.opts, wave_dev, soff)
    out = _nan(int(foff[-1]), ld)
    got, foff2 = h.compute(wave_dev, soff, ld=ld, out=out)
    assert got is out and (foff2 == foff).all()
    return out, foff


def _fbank_into_nan(h, wave_dev, soff, ld):
    """xv_fbank_compute on the handle of `h` with NaN-filled features and a NaN-filled side energy (Fbank.compute allocates the
    side energy itself, so this goes through the C ABI)."""
    import torch
    from tf_kaldi_speaker_amd import _lib, mfcc as M
    soff, foff = M.packed_offsets(h.opts, wave_dev, soff)
    out, energy = _nan(int(foff[-1]), ld), _nan(int(foff[-1]))
    if foff[-1]:
        soff_dev, foff_dev = torch.from_numpy(soff).cuda(), torch.from_numpy(foff).cuda()
        _lib.check(h._lib.xv_fbank_compute(h._h, C.c_void_p(wave_dev.data_ptr()), C.c_void_p(soff_dev.data_ptr()),
                                           C.c_void_p(foff_dev.data_ptr()), len(soff) - 1, C.c_void_p(out.data_ptr()), ld,
                                           C.c_void_p(energy.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    return out, foff, energy


def _vad_into_nan(feats_dev, foff, vo):
    """xv_vad_energy into a NaN-filled vector (vad_packed allocates its own)."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    foff = np.ascontiguousarray(foff, dtype=np.int32)
    assert feats_dev.is_contiguous() and feats_dev.shape[0] == foff[-1]
    vad = _nan(int(foff[-1]))
    foff_dev = torch.from_numpy(foff).cuda()
    _lib.check(_lib.load().xv_vad_energy(0, C.c_void_p(feats_dev.data_ptr()), int(feats_dev.shape[1]), C.c_void_p(foff_dev.data_ptr()),
                                         len(foff) - 1, vo["vad_energy_threshold"], vo["vad_energy_mean_scale"], vo["vad_frames_context"],
                                         vo["vad_proportion_threshold"], C.c_void_p(vad.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return vad


def _comparable(o, feats):
    """What the tolerance is measured on: the features, or their floored log for the linear fbank output."""
    feats = np.asarray(feats, dtype=np.float64)
    return feats if o.get("use_log_fbank", True) else np.log(np.maximum(feats, EPS))


def _mfcc_oracle(utts, o):
    """(float64 features per utterance, e32) of an MFCC batch."""
    f64 = [ref_mfcc.mfcc(x, o) for x in utts]
    f32 = [ref_mfcc.mfcc(x, o, dtype=np.float32) for x in utts]
    return f64, float(max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(f32, f64) if b.shape[0]))


def _fbank_oracle(utts, o):
    """(float64 features per utterance, float64 energies per utterance, e32) of an fbank batch."""
    f64 = [ref_fbank.fbank(x, o) for x in utts]
    f32 = [ref_fbank.fbank(x, o, dtype=np.float32) for x in utts]
    e32 = max(max(np.abs(_comparable(o, a[0]) - _comparable(o, b[0])).max(), np.abs(a[1].astype(np.float64) - b[1]).max())
              for a, b in zip(f32, f64) if b[0].shape[0])
    return [f for f, _ in f64], [e for _, e in f64], float(e32)


def _cached(key, make):
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


# --------------------------------------------------------------------------------------------- a. every option, every row
@pytest.mark.parametrize("extra_ld", [0, 5])
@pytest.mark.parametrize("name", sorted(mfcc_cases.EDGE_CONFIGS))
def test_mfcc_edge_sets_write_every_row_and_match_the_oracle(name, extra_ld):
    from tf_kaldi_speaker_amd import mfcc as M
    o = mfcc_cases.EDGE_CONFIGS[name]
    utts = mfcc_cases.edge_batch(name, o)
    f64, e32 = _cached(("mfcc", name), lambda: _mfcc_oracle(utts, o))
    want = np.concatenate(f64)
    nc = o["num_ceps"]
    ld = nc + extra_ld
    h = M.Mfcc(M.MfccOptions(**o))
    wave_dev, soff = _pack(utts)
    out, foff = _mfcc_into_nan(h, wave_dev, soff, ld)
    counts = [ref_mfcc.num_frames(len(u), o) for u in utts]
    assert foff.dtype == np.int32 and foff.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    got = out.cpu().numpy()
    assert got.shape == (sum(counts), ld) and sum(counts) == want.shape[0]
    assert not np.isnan(got[:, :nc]).any(), "rows never written: %s" % np.flatnonzero(np.isnan(got[:, :nc]).any(axis=1))[:20]
    assert np.isnan(got[:, nc:]).all()                                  # nothing beyond num_ceps is touched
    assert np.isfinite(got[:, :nc]).all()
    diff = np.abs(got[:, :nc] - want)
    err = float(diff.max())
    print("[edges a] mfcc %s ld=%d: %d frames, e32 %.3e, GPU max abs error %.3e (coefficient 0: %.3e, others: %.3e), bound %.3e"
          % (name, ld, want.shape[0], e32, err, diff[:, 0].max(), diff[:, 1:].max(), 4 * e32))
    assert err <= 4 * e32
    if o["energy_floor"] > 0:                                           # frames on the floor carry the floor itself
        floor = np.log(o["energy_floor"])
        on_floor = want[:, 0] == floor
        assert 10 <= on_floor.sum() <= len(on_floor) - 10
        assert (got[on_floor, 0] == np.float32(floor)).all() and (got[~on_floor, 0] > np.float32(floor)).all()
    again, _ = _mfcc_into_nan(h, wave_dev, soff, ld)
    assert again.data_ptr() != out.data_ptr() and _same_bits(out, again)
    h.close()


@pytest.mark.parametrize("extra_ld", [0, 5])
@pytest.mark.parametrize("name", sorted(mfcc_cases.FBANK_EDGE_CONFIGS))
def test_fbank_edge_sets_write_every_row_and_match_the_oracle(name, extra_ld):
    import torch
    from tf_kaldi_speaker_amd import fbank as F
    o = mfcc_cases.FBANK_EDGE_CONFIGS[name]
    utts = mfcc_cases.edge_batch(name, o)
    f64, en64, e32 = _cached(("fbank", name), lambda: _fbank_oracle(utts, o))
    want, want_e = np.concatenate(f64), np.concatenate(en64)
    nf = ref_fbank.num_feats(o)
    ld = nf + extra_ld
    h = F.Fbank(F.FbankOptions(**o))
    wave_dev, soff = _pack(utts)
    # through the class into a NaN-filled tensor, then through the C ABI with the side energy NaN-filled as well
    out = _nan(want.shape[0], ld)
    got_t, foff, energy = h.compute(wave_dev, soff, ld=ld, out=out, energy=True)
    assert got_t is out
    out2, foff2, energy2 = _fbank_into_nan(h, wave_dev, soff, ld)
    counts = [ref_mfcc.num_frames(len(u), o) for u in utts]
    assert foff.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist() == foff2.tolist()
    got, got_e = out2.cpu().numpy(), energy2.cpu().numpy()
    assert not np.isnan(got[:, :nf]).any() and not np.isnan(got_e).any()
    assert np.isnan(got[:, nf:]).all()
    assert np.isfinite(got[:, :nf]).all() and np.isfinite(got_e).all()
    assert _same_bits(out, out2) and torch.equal(energy, energy2)
    err = float(np.abs(_comparable(o, got[:, :nf]) - _comparable(o, want)).max())
    err_e = float(np.abs(got_e - want_e).max())
    print("[edges a] fbank %s ld=%d: %d frames, e32 %.3e, GPU max abs error %.3e, side energy %.3e, bound %.3e"
          % (name, ld, want.shape[0], e32, err, err_e, 4 * e32))
    assert err <= 4 * e32
    assert err_e <= 4 * e32
    if o["use_energy"]:
        assert (got[:, 0] == got_e).all()
    empty = np.flatnonzero(ref_mfcc.mel_bank(o).sum(axis=1) == 0)
    assert len(empty) == (1 if name == "amp256" else 0)
    if len(empty):                                                       # a filter without an FFT bin: the floor, on every frame
        assert np.abs(got[:, empty + int(o["use_energy"])] - np.log(EPS)).max() <= 1e-5
    if o["energy_floor"] > 0:
        on_floor = want_e == np.log(o["energy_floor"])
        assert 10 <= on_floor.sum() <= len(on_floor) - 10
        assert (got_e[on_floor] == np.float32(np.log(o["energy_floor"]))).all()
    h.close()


# --------------------------------------------------------------------------------------------- b. the second grid pass
GRID_SETS = {"mfcc-voxceleb": ("mfcc", ref_mfcc.VOXCELEB), "mfcc-kaldi_defaults": ("mfcc", ref_mfcc.DEFAULTS),
             "fbank-v3": ("fbank", ref_fbank.V3), "fbank-kaldi_defaults": ("fbank", ref_fbank.DEFAULTS)}
GRID_SEEDS = 5


def _grid_unique(kind, o):
    """The distinct utterances of the many-tile batch (every length of mfcc_cases.grid_lengths with every seed: utterance i of
    the batch is number i % len of these) with their oracle results.  e32 over them is e32 over any batch made of them."""
    lengths = mfcc_cases.grid_lengths(o)
    utts = [mfcc_cases.signal(lengths[u % len(lengths)], o["sample_frequency"], seed=60 + u % GRID_SEEDS, dc=(-200.0, 0.0, 350.0)[u % 3])
            for u in range(len(lengths) * GRID_SEEDS)]
    assert len(lengths) == 14 and len(utts) == 70                        # 14 and 5 share no factor: every pair occurs
    if kind == "mfcc":
        f64, e32 = _mfcc_oracle(utts, o)
        return utts, f64, None, e32
    return (utts,) + _fbank_oracle(utts, o)


@pytest.mark.parametrize("case", sorted(GRID_SETS))
def test_workgroups_that_take_a_second_tile(case):
    import torch
    from tf_kaldi_speaker_amd import fbank as F, mfcc as M
    kind, o = GRID_SETS[case]
    uniq, f64, en64, e32 = _cached(("grid", case), lambda: _grid_unique(kind, o))
    grid = GRID_FACTOR * torch.cuda.get_device_properties(0).multi_processor_count
    counts = [ref_mfcc.num_frames(len(u), o) for u in uniq]
    B, tiles = 0, 0
    while tiles < 1.5 * grid:                                            # whole cycles of the 70 utterances
        B += len(uniq)
        tiles = B // len(uniq) * sum(counts) // RUN + B
    ids = np.arange(B) % len(uniq)
    utts = [uniq[u] for u in ids]
    want_off = np.concatenate([[0], np.cumsum([counts[u] for u in ids])])
    # the launch of csrc/mfcc.hip has 8 x CUs workgroups and foff[B] / 16 + B tiles of kRun = 16 frames: half of the workgroups
    # take a second tile, and the last tiles belong to utterances far into the binary search
    assert want_off[-1] // RUN + B >= 1.5 * GRID_FACTOR * torch.cuda.get_device_properties(0).multi_processor_count
    busy, idle = mfcc_cases.tile_cover(want_off, RUN)
    assert idle >= B // 14 and sum(1 for w, _, _, _ in busy if w >= grid) >= grid // 8      # idle tiles, and busy ones in pass two
    h = (M.Mfcc(M.MfccOptions(**o)) if kind == "mfcc" else F.Fbank(F.FbankOptions(**o)))
    width = o["num_ceps"] if kind == "mfcc" else ref_fbank.num_feats(o)
    ld = width + 3

    def run(part):
        wave_dev, soff = _pack(part)
        if kind == "mfcc":
            out, foff = _mfcc_into_nan(h, wave_dev, soff, ld)
            return out, foff, None
        return _fbank_into_nan(h, wave_dev, soff, ld)

    out, foff, energy = run(utts)
    assert foff.dtype == np.int32 and foff.tolist() == want_off.tolist()
    got = out.cpu().numpy()
    unwritten = np.flatnonzero(np.isnan(got[:, :width]).any(axis=1))
    assert len(unwritten) == 0, "%d of %d rows hold NaN, first %s" % (len(unwritten), len(got), unwritten[:10])
    assert np.isnan(got[:, width:]).all()
    want = np.concatenate([f64[u] for u in ids])
    err = float(np.abs(got[:, :width] - want).max())
    err_e = 0.0
    if energy is not None:
        got_e = energy.cpu().numpy()
        assert not np.isnan(got_e).any()
        err_e = float(np.abs(got_e - np.concatenate([en64[u] for u in ids])).max())
    print("[edges b] %s: %d CUs, %d utterances, %d samples, %d frames, %d tiles on %d workgroups (%d idle); e32 %.3e, GPU max abs "
          "error %.3e, side energy %.3e, bound %.3e" % (case, grid // GRID_FACTOR, B, sum(len(u) for u in utts), len(got),
                                                        want_off[-1] // RUN + B, grid, idle, e32, err, err_e, 4 * e32))
    assert err <= 4 * e32 and err_e <= 4 * e32
    # the same utterances 64 at a time: few tiles, every workgroup at most one.  No tolerance: a stale `span`, a tile given to the
    # wrong utterance or a missed barrier changes bits
    parts, parts_e = [], []
    for k in range(0, B, 64):
        assert (want_off[min(k + 64, B)] - want_off[k]) // RUN + 64 <= grid
        part, _, part_e = run(utts[k:k + 64])
        parts.append(part)
        parts_e.append(part_e)
    assert _same_bits(out, torch.cat(parts))
    if energy is not None:
        assert _same_bits(energy, torch.cat(parts_e))
    h.close()


# --------------------------------------------------------------------------------------------- c. full-scale input
def _full_scale():
    k = np.arange(4000)
    utts = [np.where((k // 32) % 2 == 0, 32767, -32768).astype(np.int16),        # 250 Hz square wave over the whole int16 range
            np.full(4000, -32768, np.int16),
            np.where(k % 2 == 0, 1, -1).astype(np.int16)]                        # the Nyquist frequency at the smallest amplitude
    o = ref_mfcc.VOXCELEB
    f64 = [ref_mfcc.mfcc(x, o) for x in utts]
    e32 = [float(np.abs(ref_mfcc.mfcc(x, o, dtype=np.float32).astype(np.float64) - f).max()) for x, f in zip(utts, f64)]
    return utts, f64, e32


def test_full_scale_input():
    from tf_kaldi_speaker_amd import mfcc as M
    o = ref_mfcc.VOXCELEB
    utts, f64, e32 = _cached("full-scale", _full_scale)
    h = M.Mfcc(M.MfccOptions(**o))
    wave_dev, soff = _pack(utts)
    out, foff = _mfcc_into_nan(h, wave_dev, soff, o["num_ceps"])
    got = out.cpu().numpy()
    assert foff.tolist() == [0, 25, 50, 75] and np.isfinite(got).all()
    errs = [float(np.abs(got[foff[i]:foff[i + 1]] - f64[i]).max()) for i in range(3)]
    for label, e, err in zip(("square wave", "all -32768", "alternating +-1"), e32, errs):
        print("[edges c] %s: e32 %.3e, GPU max abs error %.3e, bound %.3e" % (label, e, err, 4 * e))
    print("[edges c] the batch: e32 %.3e, GPU max abs error %.3e, bound %.3e" % (max(e32), max(errs), 4 * max(e32)))
    assert max(errs) <= 4 * max(e32)                                             # the rule: e32 of the batch
    # all -32768: digital silence whatever the level
    row = np.zeros(o["num_ceps"])
    row[0] = np.log(EPS)
    assert np.abs(got[25:50] - row).max() <= 1e-5
    # the square wave alone, by its own e32 (the batch's is set by the leakage of the alternating signal)
    assert errs[0] <= 4 * e32[0]
    h.close()


# --------------------------------------------------------------------------------------------- d. vad_kernel
def _vad_tracks():
    """Energies 4, 5 and 6 around a constant threshold of 5 (the comparison is strict: 5 is not above it)."""
    rng = np.random.RandomState(11)
    tie = lambda above: np.where(np.isin(np.arange(25), np.arange(above) * 25 // above), 6.0, 4.0)       # noqa: E731
    tracks = [np.zeros(0), np.zeros(0), np.array([6.0]), np.array([5.0]), np.array([6.0, 4.0, 5.0, 6.0, 4.0]),
              rng.choice([4.0, 5.0, 6.0], size=257), rng.choice([4.0, 5.0, 6.0], size=513),
              tie(15), tie(7), tie(14), np.full(30, 5.0), np.zeros(0)]
    assert [int((t > 5.0).sum()) for t in tracks[7:10]] == [15, 7, 14]
    return tracks


def _vad_feats(tracks, ld):
    import torch
    e = np.concatenate(tracks).astype(np.float32)
    feats = np.full((len(e), ld), 1e6, dtype=np.float32)                 # whatever sits beside column 0 is above any threshold
    feats[:, 0] = e
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    return torch.from_numpy(feats).cuda(), off


@pytest.mark.parametrize("ld", [1, 7])
def test_vad_on_hand_made_energies(ld):
    tracks = _vad_tracks()
    feats_dev, off = _vad_feats(tracks, ld)
    ties = {}
    for context, proportion in ((12, 0.6), (12, 0.28), (12, 0.56), (2, 0.6), (2, 0.12), (0, 0.6)):
        vo = dict(vad_energy_threshold=5.0, vad_energy_mean_scale=0.0, vad_frames_context=context, vad_proportion_threshold=proportion)
        want = np.concatenate([ref_mfcc.vad(t[:, None], vo) for t in tracks])
        got = _vad_into_nan(feats_dev, off, vo).cpu().numpy()
        assert not np.isnan(got).any()
        wrong = np.flatnonzero(got != want)
        assert len(wrong) == 0, "context %d proportion %g: frames %s differ" % (context, proportion, wrong[:10])
        assert set(want.tolist()) == {0.0, 1.0}
        ties[(context, proportion)] = [int(got[off[u] + 12]) for u in (7, 8, 9)]
    # the full 25-frame windows with 15, 7 and 14 frames above: 25 * 0.6f > 15, 25 * 0.28f == 7, 25 * 0.56f == 14 in float
    assert ties[(12, 0.6)][0] == 0
    assert ties[(12, 0.28)][1] == 1
    assert ties[(12, 0.56)][2] == 1
    assert (ties[(12, 0.6)], ties[(12, 0.28)], ties[(12, 0.56)]) == ([0, 0, 0], [1, 1, 1], [1, 0, 1])


@pytest.mark.parametrize("ld", [1, 7])
def test_vad_with_a_mean_scaled_threshold(ld):
    rng = np.random.RandomState(12)
    tracks = [rng.uniform(0.0, 20.0, size=n).astype(np.float32).astype(np.float64) for n in (0, 1, 5, 257, 513, 0, 700)]
    feats_dev, off = _vad_feats(tracks, ld)
    for vo in (ref_mfcc.VAD_DEFAULTS, ref_mfcc.VAD_VOXCELEB, dict(ref_mfcc.VAD_DEFAULTS, vad_frames_context=12)):
        for t in tracks:                                                 # from the oracle alone: no energy near the threshold
            assert len(t) == 0 or np.abs(t - ref_mfcc.vad_threshold(t[:, None], vo)).min() > 1e-3
        want = np.concatenate([ref_mfcc.vad(t[:, None], vo) for t in tracks])
        got = _vad_into_nan(feats_dev, off, vo).cpu().numpy()
        assert not np.isnan(got).any() and (got == want).all()
        assert set(want.tolist()) == {0.0, 1.0}
