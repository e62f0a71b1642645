"""No GPU: xv_train_stage (csrc/train_stage.cpp) against the native reader.  Archives come from the encoder of
tests/helpers/train_arks.py; the staged bytes and descriptors, decoded by the numpy restatement of the rule of
include/xvec_hip.h, must have the bits xv_ark_next_batch gives for the same record, cut to the chunk.  Refused inputs give a
status and a message, and the loader's stage_batch falls back to kaldi_io.read_mat for them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import train_arks as ta                                            # noqa: E402

COLS = (1, 3, 30, 33)
ROWS = (1, 64, 65, 300)
KINDS = {"FM": ta.FM, "DM": ta.DM, "CM": ta.CM}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def arks(lib, tmp_path_factory):
    """One ark per kind with every cols x rows record -> {kind name: (path, {key: rx}, {key: oracle matrix})}."""
    tmp = tmp_path_factory.mktemp("stage")
    out = {}
    for name, kind in KINDS.items():
        rs = np.random.RandomState(kind)
        recs = [("%s_c%d_r%d" % (name, c, r), ta.random_record(kind, r, c, rs)) for c in COLS for r in ROWS]
        path = str(tmp / (name + ".ark"))
        rx = ta.write_ark(path, recs)
        out[name] = (path, dict(zip([k for k, _ in recs], rx)), ta.native_decode(path))
    return out


def test_the_descriptor_mirror_has_the_headers_size(lib):
    assert ta.chunk_sizeof() == 40
    assert (lib.XV_TRAIN_FM, lib.XV_TRAIN_DM, lib.XV_TRAIN_CM) == (ta.FM, ta.DM, ta.CM)


@pytest.mark.parametrize("name", sorted(KINDS))
@pytest.mark.parametrize("threads", (1, 16))
def test_staged_chunks_decode_to_the_native_readers_bits(lib, arks, name, threads):
    from tf_kaldi_speaker_amd import train_input
    path, rxs, oracle = arks[name]
    for length_of in (lambda r: 1, lambda r: (r + 1) // 2, lambda r: r):            # one row, a part, the whole record
        for cols in COLS:
            for rows in ROWS:
                n = length_of(rows)
                for start in sorted({0, rows - n}):
                    buf = np.full(1 << 17, 0xA5, dtype=np.uint8)
                    key = "%s_c%d_r%d" % (name, cols, rows)
                    rc, chunks, status, nbytes, msg = train_input.stage([rxs[key]], [start], n, buf, threads)
                    assert rc == 0 and msg == "" and status[0] == 0, msg
                    c = chunks[0]
                    assert (c.kind, c.cols, c.rows, c.first_row) == (KINDS[name], cols, n, 0) and c.payload_off % 16 == 0
                    assert nbytes % 16 == 0 and np.all(buf[nbytes:] == 0xA5)         # nothing behind the layout is written
                    for dim in sorted({cols, max(1, cols - 2)}):
                        got = ta.numpy_decode(buf, c, n, dim)
                        assert ta.same_bits(got, oracle[key][start:start + n, :dim]), (key, start, n, dim)


def test_a_batch_of_mixed_kinds_has_one_layout_for_every_thread_count(lib, arks):
    from tf_kaldi_speaker_amd import train_input
    rs = np.random.RandomState(5)
    picks = []
    for name in sorted(KINDS):
        for cols in COLS:
            for rows in (64, 65, 300):
                picks.append((name, "%s_c%d_r%d" % (name, cols, rows), int(rs.randint(rows - 40 + 1))))
    rxs = [arks[n][1][k] for n, k, _ in picks]
    starts = [s for _, _, s in picks]
    first = None
    for threads in (1, 3, 16):
        buf = np.zeros(1 << 20, dtype=np.uint8)
        rc, chunks, status, nbytes, msg = train_input.stage(rxs, starts, 40, buf, threads)
        assert rc == 0 and not status.any(), msg
        desc = bytes(C.string_at(C.addressof(chunks), C.sizeof(chunks)))
        if first is None:
            first = (desc, buf[:nbytes].copy())
        assert desc == first[0] and np.array_equal(buf[:nbytes], first[1])
    offs = [c.header_off if c.kind == ta.CM else c.payload_off for c in chunks]
    assert offs == sorted(offs) and offs[0] == 0                                     # chunk order, no holes in front
    for c, (name, key, start) in zip(chunks, picks):
        assert ta.same_bits(ta.numpy_decode(buf, c, 40, c.cols), arks[name][2][key][start:start + 40])


def test_too_small_a_buffer_is_reported_with_the_size_needed(lib, arks):
    from tf_kaldi_speaker_amd import train_input
    buf = np.full(64, 0xA5, dtype=np.uint8)
    rc, _, _, nbytes, msg = train_input.stage([arks["FM"][1]["FM_c30_r300"]], [0], 300, buf)
    assert rc == lib.XV_ERR_WORKSPACE and nbytes == 300 * 30 * 4 and "36000" in msg and np.all(buf == 0xA5)


def _one(train_input, rx, start, length):
    buf = np.zeros(1 << 16, dtype=np.uint8)
    rc, chunks, status, nbytes, msg = train_input.stage([rx], [start], length, buf)
    return rc, int(status[0]), chunks[0].kind, nbytes, msg


def test_refused_inputs_give_a_status_and_a_message(lib, arks, tmp_path):
    from tf_kaldi_speaker_amd import train_input
    rs = np.random.RandomState(0)
    # a short record
    rc, st, kind, nbytes, msg = _one(train_input, arks["CM"][1]["CM_c3_r64"], 60, 5)
    assert (rc, st, kind, nbytes) == (1, lib.XV_ERR_INVALID, 0, 0) and "short record" in msg and "64 rows" in msg
    # an unknown kind
    path = str(tmp_path / "odd.ark")
    rx = ta.write_ark(path, [("u", b"\0BCM2" + bytes(64))])
    rc, st, kind, _, msg = _one(train_input, rx[0], 0, 1)
    assert (rc, st, kind) == (1, lib.XV_ERR_INVALID, 0) and "unknown kind" in msg
    # truncated files: inside the payload, inside the header, and an offset behind the end
    for name, kind_id in KINDS.items():
        path = str(tmp_path / ("cut_%s.ark" % name))
        rx = ta.write_ark(path, [("u", ta.random_record(kind_id, 20, 4, rs))])
        size = os.path.getsize(path)
        for keep in (size - 1, int(rx[0].rsplit(":", 1)[1]) + 7, 1):
            ta.truncate(path, keep)
            rc, st, kind, _, msg = _one(train_input, rx[0], 0, 20)
            assert (rc, st, kind) == (1, lib.XV_ERR_INVALID, 0) and ("truncated" in msg or "beyond the end" in msg), (name, keep, msg)
    # pipes and ranges, a missing file
    for rx in ("copy-feats ark:x.ark ark:- |", arks["FM"][1]["FM_c3_r64"] + "[0:3]"):
        rc, st, kind, _, msg = _one(train_input, rx, 0, 1)
        assert (rc, st, kind) == (1, lib.XV_ERR_UNSUPPORTED, 0) and "pipe or a range" in msg
    rc, st, kind, _, msg = _one(train_input, str(tmp_path / "nothing.ark") + ":5", 0, 1)
    assert (rc, st) == (1, lib.XV_ERR_INVALID) and "cannot open" in msg
    # one refused chunk does not stop the others, and the message names it
    buf = np.zeros(1 << 16, dtype=np.uint8)
    good = arks["DM"][1]["DM_c3_r65"]
    rc, chunks, status, nbytes, msg = train_input.stage([good, "cmd |", good], [0, 0, 5], 60, buf)
    assert rc == 1 and list(status) == [0, lib.XV_ERR_UNSUPPORTED, 0] and msg.startswith("chunk 1 ")
    assert ta.same_bits(ta.numpy_decode(buf, chunks[2], 60, 3), arks["DM"][2]["DM_c3_r65"][5:65])


def test_bad_arguments_are_invalid(lib):
    raw = lib.load()
    buf = np.zeros(64, dtype=np.uint8)
    chunks = (lib.TrainChunk * 1)()
    status, starts, nbytes = np.zeros(1, np.int32), np.zeros(1, np.int32), C.c_int64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                      # noqa: E731
    args = lambda rx, n, length: (rx, n, p(starts), length, 1, p(buf), buf.size, C.cast(chunks, C.c_void_p), p(status),    # noqa: E731
                                  C.cast(C.pointer(nbytes), C.c_void_p), None, 0)
    assert raw.xv_train_stage(*args(b"a\n", 0, 1)) == lib.XV_ERR_INVALID
    assert raw.xv_train_stage(*args(b"a\n", 1, 0)) == lib.XV_ERR_INVALID
    assert raw.xv_train_stage(*args(b"a", 1, 1)) == lib.XV_ERR_INVALID                # no newline: fewer names than n
    assert raw.xv_train_stage(*args(None, 1, 1)) == lib.XV_ERR_INVALID


def test_stage_batch_falls_back_to_read_mat_for_what_the_stager_refuses(lib, arks, tmp_path):
    """Piped rxfilenames among native chunks: the batch decodes to what read_train_batch returns."""
    from tf_kaldi_speaker_amd import head_train, train_input
    fm, cm = arks["FM"], arks["CM"]
    piped = "cat %s |" % _single(tmp_path, fm[2]["FM_c30_r65"])
    rxfiles = [cm[1]["CM_c30_r300"], piped, fm[1]["FM_c33_r64"], piped]
    batch = head_train.TrainBatch(["a", "b", "c", "d"], rxfiles, np.arange(4, dtype=np.int32), 24, [270, 41, 0, 3])
    want = head_train.read_train_batch(batch, 30)
    held = {}

    def reserve(n):
        if "a" not in held or held["a"].size < n:
            held["a"] = np.zeros(max(n, 1 << 12), dtype=np.uint8)                    # small: the fallback has to grow it
        return held["a"]

    buf, staged = train_input.stage_batch(batch, 30, reserve)
    assert staged.fallbacks == [1, 3] and staged.nbytes <= buf.size
    for j in range(4):
        assert ta.same_bits(ta.numpy_decode(buf, staged.chunks[j], 24, 30), want[j]), j
    with pytest.raises(ValueError, match="features have 30 columns, the network needs 31"):
        train_input.stage_batch(batch, 31, reserve)


def _single(tmp_path, mat):
    from tf_kaldi_speaker_amd import kaldi_io
    path = str(tmp_path / "single.ark")
    with open(path, "wb") as f:
        kaldi_io.write_mat(f, mat)
    return path
