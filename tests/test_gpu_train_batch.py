"""GPU: xv_train_batch_decode (csrc/train_batch.hip) against the native reader's decode (xv_ark_next_batch), bit for bit.
Records come from the encoder of tests/helpers/train_arks.py and are staged by xv_train_stage; hand-made descriptors cover a
first staged row above 0.  The refusals are host-side: nothing here launches with a bad descriptor."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import train_arks as ta                                            # noqa: E402
import poison                                                       # noqa: E402

pytestmark = pytest.mark.gpu

COLS = (1, 3, 30, 33)
LENGTHS = (1, 2, 63, 64, 65)
POISON = 0x7B


def _records():
    """[(key, record bytes)]: for every cols one FM, one DM and two CM records of 300 rows (one with all 256 byte values in
    every column), a CM record with a zero-slope column (p0 == p25), one with range = 0, a 70-column record (two column tiles)
    and a 1-row record."""
    rs = np.random.RandomState(11)
    recs = []
    for cols in COLS:
        recs.append(("fm_c%d" % cols, ta.random_record(ta.FM, 300, cols, rs)))
        recs.append(("dm_c%d" % cols, ta.random_record(ta.DM, 300, cols, rs)))
        recs.append(("cm_c%d" % cols, ta.random_record(ta.CM, 300, cols, rs)))
        recs.append(("all_c%d" % cols, ta.all_bytes_record(cols, rs)))
    headers = np.sort(rs.randint(0, 65536, (3, 4)), axis=1)
    headers[1, 1] = headers[1, 0]                                                     # p0 == p25
    headers[2, :] = headers[2, 0]                                                     # a constant column
    recs.append(("flat", ta.cm_record(-1.5, 9.0, headers, np.stack([np.arange(300) % 256] * 3))))
    recs.append(("norange", ta.cm_record(2.75, 0.0, np.sort(rs.randint(0, 65536, (3, 4)), axis=1), rs.randint(0, 256, (3, 300)))))
    recs.append(("wide_cm", ta.random_record(ta.CM, 130, 70, rs)))
    recs.append(("wide_dm", ta.random_record(ta.DM, 130, 70, rs)))
    recs.append(("one", ta.random_record(ta.CM, 1, 3, rs)))
    return recs


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    import torch
    assert torch.cuda.is_available()
    path = str(tmp_path_factory.mktemp("batch") / "mixed.ark")
    recs = _records()
    rx = dict(zip([k for k, _ in recs], ta.write_ark(path, recs)))
    return rx, ta.native_decode(path)


def gpu_decode(rxfiles, starts, length, dim, ld=None, chunks=None, buf=None, nbytes=None):
    """Stage (unless chunks / buf are given) and decode -> (rc, the whole poisoned output [n * length, ld] as numpy)."""
    import torch
    from tf_kaldi_speaker_amd import _lib, train_input
    lib = _lib.load()
    if chunks is None:
        buf = np.zeros(1 << 21, dtype=np.uint8)
        rc, chunks, status, nbytes, msg = train_input.stage(rxfiles, starts, length, buf)
        assert rc == 0, msg
    n = len(chunks)
    ld = dim if ld is None else ld
    staged = torch.from_numpy(buf[:max(nbytes, 16)].copy()).cuda()
    out = poison.fill(torch.empty((n * max(length, 1), ld), dtype=torch.float32, device="cuda"), POISON)
    ws = poison.fill(torch.empty(max(train_input.workspace_bytes(n), 256), dtype=torch.uint8, device="cuda"), 0xFF)
    rc = lib.xv_train_batch_decode(0, _lib.ptr(staged), nbytes, C.cast(chunks, C.c_void_p), n, length, dim, _lib.ptr(out), ld,
                                   _lib.ptr(ws), ws.numel(), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _is_poison(a):
    return np.ascontiguousarray(a).view(np.uint8) == POISON


@pytest.mark.parametrize("length", LENGTHS)
def test_one_launch_of_37_mixed_chunks_has_the_native_readers_bits(world, length):
    """37 chunks over every kind and every record of 3 columns or more, dim = 3 < cols for most; ld > dim: the padding columns
    keep the poison, no chunk element does.  A repeat gives the same bits."""
    rx, oracle = world
    rs = np.random.RandomState(length)
    keys = [k for k in sorted(rx) if oracle[k].shape[1] >= 3 and oracle[k].shape[0] >= length]
    picks = [keys[i % len(keys)] for i in range(37)]
    starts = [int(rs.randint(oracle[k].shape[0] - length + 1)) for k in picks]
    starts[0], starts[1] = 0, oracle[picks[1]].shape[0] - length
    rc, out = gpu_decode([rx[k] for k in picks], starts, length, 3, ld=5)
    assert rc == 0
    out = out.reshape(37, length, 5)
    for j, (k, s) in enumerate(zip(picks, starts)):
        assert ta.same_bits(out[j, :, :3], oracle[k][s:s + length, :3]), (j, k, s)
    assert _is_poison(out[:, :, 3:]).all() and not _is_poison(out[:, :, :3]).reshape(37, length, 3, 4).all(axis=3).any()
    rc2, again = gpu_decode([rx[k] for k in picks], starts, length, 3, ld=5)
    assert rc2 == 0 and np.array_equal(out.view(np.uint32).reshape(-1), again.view(np.uint32).reshape(-1))


@pytest.mark.parametrize("cols", COLS)
def test_every_width_with_dim_equal_to_and_below_cols(world, cols):
    rx, oracle = world
    keys = ["fm_c%d" % cols, "dm_c%d" % cols, "cm_c%d" % cols, "all_c%d" % cols]
    for dim in sorted({cols, max(1, cols - 1)}):
        for length, starts in ((300, [0, 0, 0, 0]), (65, [235, 0, 117, 235])):
            rc, out = gpu_decode([rx[k] for k in keys], starts, length, dim)
            assert rc == 0
            out = out.reshape(4, length, dim)
            for j, (k, s) in enumerate(zip(keys, starts)):
                assert ta.same_bits(out[j], oracle[k][s:s + length, :dim]), (k, dim, length)


def test_piece_borders_zero_slopes_and_a_zero_range(world):
    """all_c*: every byte value in every column (64 | 65 and 192 | 193 decide the piece).  flat: p0 == p25 and a constant
    column.  norange: range = 0, every element is the global minimum."""
    rx, oracle = world
    rc, out = gpu_decode([rx["flat"], rx["norange"], rx["all_c3"]], [0, 0, 0], 300, 3)
    assert rc == 0
    out = out.reshape(3, 300, 3)
    for j, k in enumerate(("flat", "norange", "all_c3")):
        assert ta.same_bits(out[j], oracle[k]), k
    assert np.all(out[1] == np.float32(2.75)) and np.unique(out[0][:65, 1]).size == 1 and np.unique(out[0][:, 2]).size == 1


def test_one_chunk_two_column_tiles_and_a_first_row_above_zero(world):
    rx, oracle = world
    rc, out = gpu_decode([rx["one"]], [0], 1, 3)                                      # B = 1, one row
    assert rc == 0 and ta.same_bits(out, oracle["one"])
    for k in ("wide_cm", "wide_dm"):
        rc, out = gpu_decode([rx[k]], [0], 130, 70, ld=72)
        assert rc == 0 and ta.same_bits(out[:, :70], oracle[k]) and _is_poison(out[:, 70:]).all()
        rc, out = gpu_decode([rx[k]], [1], 129, 65)
        assert rc == 0 and ta.same_bits(out, oracle[k][1:, :65])
    # hand-made descriptors on whole staged records: the chunk starts at staged row 7
    from tf_kaldi_speaker_amd import train_input
    buf = np.zeros(1 << 20, dtype=np.uint8)
    keys = ["cm_c33", "fm_c33", "dm_c33"]
    rc, chunks, status, nbytes, msg = train_input.stage([rx[k] for k in keys], [0, 0, 0], 300, buf)
    assert rc == 0, msg
    for c in chunks:
        c.first_row = 7
    rc, out = gpu_decode(None, None, 293, 33, chunks=chunks, buf=buf, nbytes=nbytes)
    assert rc == 0
    for j, k in enumerate(keys):
        assert ta.same_bits(out.reshape(3, 293, 33)[j], oracle[k][7:]), k


def test_invalid_descriptors_are_refused_on_the_host_and_nothing_is_written(world):
    from tf_kaldi_speaker_amd import _lib
    good = dict(kind=ta.CM, po=64, ho=0, cols=4, rows=20, first=2, gmin=0.0, grange=1.0)      # 32 header bytes, 80 payload bytes
    nbytes, length, dim = 64 + 80, 10, 3
    buf = np.zeros(256, dtype=np.uint8)

    def run(length=length, dim=dim, ld=None, nbytes=nbytes, **over):
        d = dict(good, **over)
        chunks = ta.chunk_array([(d["kind"], d["po"], d["ho"], d["cols"], d["rows"], d["first"], d["gmin"], d["grange"])])
        rc, out = gpu_decode(None, None, length, dim, ld=ld, chunks=chunks, buf=buf, nbytes=nbytes)
        assert _is_poison(out).all() or rc == 0
        return rc

    assert run() == 0
    assert run(po=72) == _lib.XV_ERR_INVALID                       # a misaligned payload
    assert run(ho=4) == _lib.XV_ERR_INVALID                        # misaligned column headers
    assert run(first=11) == _lib.XV_ERR_INVALID                    # first_row + length > staged rows
    assert run(dim=5) == _lib.XV_ERR_INVALID                       # dim > cols
    assert run(cols=0, dim=1) == _lib.XV_ERR_INVALID               # cols < 1
    assert run(length=0) == _lib.XV_ERR_INVALID                    # length < 1
    assert run(nbytes=nbytes - 1) == _lib.XV_ERR_INVALID           # the payload reaches past the staged bytes
    assert run(ho=128) == _lib.XV_ERR_INVALID                      # the headers do
    assert run(kind=ta.DM) == _lib.XV_ERR_INVALID                  # as doubles the payload does
    assert run(kind=0) == _lib.XV_ERR_INVALID and run(kind=4) == _lib.XV_ERR_INVALID
    assert run(first=-1) == _lib.XV_ERR_INVALID
    assert run(ld=2) == _lib.XV_ERR_INVALID                        # ld < dim
