"""Test-side encoder of Kaldi matrix archives for the training-input tests, the oracle decode through the native reader, and a
numpy restatement of the rule of xv_train_batch_decode (include/xvec_hip.h) on staged bytes.

Any bytes are a valid 'CM ' record (kOneByteWithColHeaders: a global min / range, four uint16 per column, one byte per element,
column-major), so no Kaldi is needed to write one."""
import ctypes as C
import os
import struct

import numpy as np

FM, DM, CM = 1, 2, 3


def fm_record(mat):
    mat = np.ascontiguousarray(mat, dtype=np.float32)
    return b"\0BFM \4" + struct.pack("<i", mat.shape[0]) + b"\4" + struct.pack("<i", mat.shape[1]) + mat.tobytes()


def dm_record(mat):
    mat = np.ascontiguousarray(mat, dtype=np.float64)
    return b"\0BDM \4" + struct.pack("<i", mat.shape[0]) + b"\4" + struct.pack("<i", mat.shape[1]) + mat.tobytes()


def cm_record(gmin, grange, headers, payload):
    """headers uint16 [cols, 4]; payload uint8 [cols, rows] (column-major, as the file holds it)."""
    headers = np.ascontiguousarray(headers, dtype=np.uint16)
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    cols, rows = payload.shape
    assert headers.shape == (cols, 4)
    return b"\0BCM " + struct.pack("<ffii", gmin, grange, rows, cols) + headers.tobytes() + payload.tobytes()


def random_record(kind, rows, cols, rs, gmin=-12.5, grange=31.0):
    if kind == FM:
        return fm_record(rs.standard_normal((rows, cols)) * 3)
    if kind == DM:
        # doubles that are not floats: the one rounding is visible; a few beyond float's normal range on either side
        m = rs.standard_normal((rows, cols)) * np.exp(rs.uniform(-3, 3, (rows, cols)))
        m.flat[::17] *= 1e-42
        return dm_record(m)
    headers = np.sort(rs.randint(0, 65536, (cols, 4)), axis=1)
    return cm_record(gmin, grange, headers, rs.randint(0, 256, (cols, rows)))


def all_bytes_record(cols, rs, rows=300):
    """Every column holds all 256 byte values (the borders 64 / 65 and 192 / 193 included), in its own order."""
    assert rows >= 256
    payload = np.stack([rs.permutation(np.concatenate([np.arange(256), rs.randint(0, 256, rows - 256)])) for _ in range(cols)])
    headers = np.sort(rs.randint(0, 65536, (cols, 4)), axis=1)
    return cm_record(-3.25, 17.5, headers, payload)


def write_ark(path, records):
    """records: [(key, record bytes)] -> rxfilenames `path:offset`, the offset behind "key " as Kaldi's feats.scp has it."""
    rx = []
    with open(path, "wb") as f:
        for key, rec in records:
            f.write(key.encode() + b" ")
            rx.append("%s:%d" % (path, f.tell()))
            f.write(rec)
    return rx


def native_decode(path):
    """{key: float32 [rows, cols]} of every record of the ark, decoded by the native reader (xv_ark_next_batch): the oracle."""
    from tf_kaldi_speaker_amd.native_ark import ArkBatchReader
    r = ArkBatchReader("ark:" + path, batch_frames=1, max_utts=1, capacity=1 << 22)
    out = {}
    try:
        for keys, offsets, feats in r:
            assert len(keys) == 1
            out[keys[0]] = feats.copy()
    finally:
        r.close()
    return out


def numpy_decode(buf, c, length, dim):
    """Chunk descriptor `c` on the staged bytes `buf` (uint8) -> float32 [length, dim], by the header's rule."""
    rows, cols, a = c.rows, c.cols, c.first_row
    if c.kind == FM:
        return buf[c.payload_off:c.payload_off + rows * cols * 4].view(np.float32).reshape(rows, cols)[a:a + length, :dim].copy()
    if c.kind == DM:
        return buf[c.payload_off:c.payload_off + rows * cols * 8].view(np.float64).reshape(rows, cols)[a:a + length, :dim].astype(np.float32)
    assert c.kind == CM
    h = buf[c.header_off:c.header_off + cols * 8].view(np.uint16).reshape(cols, 4).astype(np.float64)
    p = (np.float64(np.float32(c.gmin)) + np.float64(np.float32(c.grange)) * 1.52590218966964e-05 * h).astype(np.float32).astype(np.float64)
    v = buf[c.payload_off:c.payload_off + cols * rows].reshape(cols, rows)[:dim, a:a + length].astype(np.float64)
    p0, p1, p2, p3 = (p[:dim, k:k + 1] for k in range(4))
    x = np.where(v <= 64, p0 + (p1 - p0) / 64. * v,
                 np.where(v <= 192, p1 + (p2 - p1) / 128. * (v - 64), p2 + (p3 - p2) / 63. * (v - 192)))
    return np.ascontiguousarray(x.T.astype(np.float32))


def chunk_array(specs):
    """[(kind, payload_off, header_off, cols, rows, first_row, gmin, grange)] -> ctypes array of _lib.TrainChunk."""
    from tf_kaldi_speaker_amd import _lib
    arr = (_lib.TrainChunk * len(specs))()
    for c, (kind, po, ho, cols, rows, first, gmin, grange) in zip(arr, specs):
        c.kind, c.payload_off, c.header_off, c.cols, c.rows, c.first_row, c.gmin, c.grange = kind, po, ho, cols, rows, first, gmin, grange
    return arr


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def chunk_sizeof():
    from tf_kaldi_speaker_amd import _lib
    return C.sizeof(_lib.TrainChunk)


def truncate(path, nbytes):
    with open(path, "r+b") as f:
        f.truncate(nbytes)
    return os.path.getsize(path)


def cm_encode(mat):
    """A float matrix -> the bytes of a 'CM ' record that decodes to about the same values (Kaldi's kOneByteWithColHeaders:
    the global range, per column the percentiles 0, 25, 75 and 100 as uint16, the elements on the three linear pieces)."""
    mat = np.asarray(mat, dtype=np.float64)
    gmin = float(np.float32(mat.min()))
    grange = float(np.float32(max(mat.max() - gmin, 1e-3) * 1.001))
    q = np.quantile(mat, [0.0, 0.25, 0.75, 1.0], axis=0).T                                  # [cols, 4]
    h = np.clip(np.rint((q - gmin) / grange * 65535.0), 0, 65535).astype(np.int64)
    for k in (1, 2, 3):
        h[:, k] = np.maximum(h[:, k], h[:, k - 1] + 1)                                      # strictly rising percentiles
    assert h.max() <= 65535
    p = gmin + grange * 1.52590218966964e-05 * h
    v = mat.T                                                                               # [cols, rows]
    p0, p1, p2, p3 = (p[:, k:k + 1] for k in range(4))
    b = np.where(v < p1, (v - p0) / (p1 - p0) * 64.0,
                 np.where(v < p2, 64.0 + (v - p1) / (p2 - p1) * 128.0, 192.0 + (v - p2) / (p3 - p2) * 63.0))
    return cm_record(gmin, grange, h, np.clip(np.rint(b), 0, 255))


def make_train_dir(tmp, speakers=6, utts=4, dim=8, frames=(40, 80), offset=1.0, seed=0):
    """A Kaldi data directory for the training tests: `speakers` x `utts` utterances of frames[0] .. frames[1] frames, unit
    noise around a mean per speaker, the utterances alternately in a 'CM ' and an 'FM ' archive -> (data dir, spklist path,
    {utt: the matrix the native reader decodes}).  Speaker s has the mean `offset` on axis s mod dim and 0 elsewhere: a batch
    of three speakers normalised by its own statistics (batch norm in training mode) keeps the sign of a speaker's own axis
    whoever the other two are, so the task stays learnable at that batch size."""
    rs = np.random.RandomState(seed)
    data = os.path.join(str(tmp), "data")
    os.makedirs(data, exist_ok=True)
    recs, spk2utt, lengths = {"cm": [], "fm": []}, [], {}
    for s in range(speakers):
        mean = np.zeros(dim)
        mean[s % dim] = offset
        names = []
        for u in range(utts):
            key = "spk%d-u%d" % (s, u)
            mat = (mean + rs.standard_normal((int(rs.randint(frames[0], frames[1] + 1)), dim))).astype(np.float32)
            lengths[key] = mat.shape[0]
            which = "cm" if (s * utts + u) % 2 == 0 else "fm"
            recs[which].append((key, cm_encode(mat) if which == "cm" else fm_record(mat)))
            names.append(key)
        spk2utt.append(("spk%d" % s, names))
    rx, mats = {}, {}
    for which in ("cm", "fm"):
        path = os.path.join(data, which + ".ark")
        rx.update(zip([k for k, _ in recs[which]], write_ark(path, recs[which])))
        mats.update(native_decode(path))
    with open(os.path.join(data, "feats.scp"), "w") as f:
        for _, names in spk2utt:
            for key in names:
                f.write("%s %s\n" % (key, rx[key]))
    with open(os.path.join(data, "spk2utt"), "w") as f:
        for spk, names in spk2utt:
            f.write("%s %s\n" % (spk, " ".join(names)))
    with open(os.path.join(data, "utt2num_frames"), "w") as f:
        for key, t in lengths.items():
            f.write("%s %d\n" % (key, t))
    spklist = os.path.join(str(tmp), "spklist")
    with open(spklist, "w") as f:
        for i, (spk, _) in enumerate(spk2utt):
            f.write("%s %d\n" % (spk, i))
    return data, spklist, mats
