"""No GPU: the layout helper of the C ABI tests (tests/helpers/abi_layouts.py) on CPU tensors, and the `ld < width` refusals of
the library, which include/xvec_hip.h promises to make before the first HIP call (host buffers, an expected status: the
pattern of tests/test_plda_host.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi_layouts as L  # noqa: E402

BASE = {"tight": 0, "pad4": 0, "pad_odd": 0, "shift1": 1, "shift3": 3}


def _source(dtype, rows, width):
    rng = np.random.default_rng(rows * 1000 + width)
    if np.dtype(dtype).kind == "f":
        return rng.standard_normal((rows, width)).astype(dtype)
    return rng.integers(-1000, 1000, (rows, width)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
@pytest.mark.parametrize("rows,width", [(1, 1), (5, 3), (3, 33), (2, 150), (2, 200)])
@pytest.mark.parametrize("layout", L.LAYOUTS)
def test_place(layout, rows, width, dtype):
    src = _source(dtype, rows, width)
    frame, ptr, ld = L.place(src, layout, "cpu")
    size = np.dtype(dtype).itemsize
    assert ld >= width and ld == frame.ld and ptr == frame.ptr
    assert ptr % 16 == (BASE[layout] * size) % 16                 # the base alignment of the table, in elements
    if layout == "tight":
        assert ld == width
    elif layout == "pad_odd":
        assert ld % 2 == 1 and ld in (width + 1, width + 2)
    else:
        assert ld % 4 == 0 and ld >= width + 4
    assert L.gather(frame).dtype == np.dtype(dtype) and L.gather(frame).tobytes() == src.tobytes()
    assert L.untouched(frame) and L.intact(frame, src)
    # the window is where the pointer says: row r at ptr + r * ld
    h = frame.host()
    first = (ptr - frame.buf.data_ptr()) // size
    assert first == frame.base
    for r in range(rows):
        assert h[first + r * ld:first + r * ld + width].tobytes() == src[r].tobytes()
    # one full row of slack on both sides, and all of it poison
    assert frame.base >= ld and h.shape[0] - (frame.base + rows * ld) >= ld
    view, bits = L.poison_bits(dtype, "nan")
    outside = np.ones(h.shape[0], bool)
    for r in range(rows):
        outside[first + r * ld:first + r * ld + width] = False
    assert outside.sum() == h.shape[0] - rows * width and np.all(h[outside] == bits)
    if np.dtype(dtype).kind == "f":
        assert np.all(np.isnan(h[outside].view(dtype)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
@pytest.mark.parametrize("layout", L.LAYOUTS)
def test_blank_and_untouched(layout, dtype):
    rows, width = 4, 7
    frame, ptr, ld = L.blank(rows, width, layout, "cpu", dtype)
    view, canary = L.poison_bits(dtype, "canary")
    assert np.all(frame.host() == canary) and L.untouched(frame)
    if np.dtype(dtype).kind == "f":
        assert canary != L.poison_bits(dtype, "nan")[1] and np.all(np.isnan(L.gather(frame)))
    # a write inside the window is not a disturbance; one element to either side of a row, or in the slack, is
    flat = frame.buf.numpy().view(view)                  # the frame's own memory, as raw bits
    flat[frame.base:frame.base + width] = 1
    flat[frame.base + (rows - 1) * ld + width - 1] = 2
    assert L.untouched(frame)
    for pos in (frame.base - 1, frame.base + (rows - 1) * ld + width, 0, flat.shape[0] - 1) + (() if ld == width else (frame.base + width,)):
        keep = flat[pos].copy()
        flat[pos] = 3
        assert not L.untouched(frame), pos
        flat[pos] = keep
        assert L.untouched(frame)
    # the comparison is of bits: another NaN is not the canary
    if np.dtype(dtype).kind == "f":
        frame.buf.numpy()[0] = np.nan
        assert not L.untouched(frame)


def test_intact_sees_a_changed_window():
    src = _source(np.float32, 3, 5)
    frame, _, _ = L.place(src, "pad4", "cpu")
    assert L.intact(frame, src)
    frame.buf.numpy()[frame.base + frame.ld + 2] += 1.0
    assert L.untouched(frame) and not L.intact(frame, src)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tf_kaldi_speaker_amd import _lib
    return _lib, _lib.load()


class Host(object):
    """Host buffers big enough for every call below; a refused call never touches them."""

    def __init__(self):
        self.f, self.g, self.d, self.i = ((ctypes.c_float * 65536)(), (ctypes.c_float * 65536)(), (ctypes.c_double * 65536)(),
                                          (ctypes.c_int32 * 4096)())
        self.h1, self.h2 = (ctypes.c_uint64 * 256)(), (ctypes.c_uint64 * 256)()
        self.x, self.o, self.dp, self.ip, self.ph1, self.ph2 = (ctypes.cast(b, ctypes.c_void_p) for b in
                                                                (self.f, self.g, self.d, self.i, self.h1, self.h2))


def test_post_step_refuses_a_short_leading_dimension(lib):
    _lib, lb = lib
    b, bad = Host(), _lib.XV_ERR_INVALID
    assert lb.xv_length_normalize(0, b.x, 7, 4, 8, 0, b.o, 8, None) == bad            # ldx < dim
    assert lb.xv_length_normalize(0, b.x, 8, 4, 8, 0, b.o, 7, None) == bad            # ldo < dim
    assert lb.xv_speaker_mean(0, b.x, 7, 8, b.ip, b.ip, 2, b.o, 8, None) == bad       # ldx < dim
    assert lb.xv_speaker_mean(0, b.x, 8, 8, b.ip, b.ip, 2, b.o, 7, None) == bad       # ldo < dim


def test_backend_refuses_a_short_leading_dimension(lib):
    _lib, lb = lib
    b, bad = Host(), _lib.XV_ERR_INVALID
    need = int(lb.xv_gram_f64_workspace(40, 8))
    assert need > 0
    assert lb.xv_gram_f64(0, b.x, 7, 40, 8, None, None, b.dp, b.o, need, None) == bad           # ldx < d
    assert lb.xv_gram_f64_rows64(0, b.dp, 7, 40, 8, None, None, b.dp, b.o, need, None) == bad   # ldx < d
    assert lb.xv_class_mean_f64(0, b.x, 7, 40, 8, b.ip, b.ip, 2, None, b.dp, 8, None) == bad    # ldx < dim
    assert lb.xv_class_mean_f64(0, b.x, 8, 40, 8, b.ip, b.ip, 2, None, b.dp, 7, None) == bad    # ldo < dim


def test_front_end_refuses_a_short_leading_dimension(lib):
    _lib, lb = lib
    b, bad = Host(), _lib.XV_ERR_INVALID
    assert lb.xv_frontend_cmn_select(0, b.x, 29, 30, b.ip, 1, b.ip, 4, 51, 1, 100, b.dp, b.o, None) == bad   # ld < dim
    assert lb.xv_vad_energy(0, b.x, 0, b.ip, 1, 5.0, 0.5, 0, 0.6, b.o, None) == bad                          # ld < 1


def test_cosine_scoring_refuses_a_short_leading_dimension(lib):
    _lib, lb = lib
    b, bad = Host(), _lib.XV_ERR_INVALID
    for lda, ldb, ldo in ((7, 8, 5), (8, 7, 5), (8, 8, 4)):                            # lda < d, ldb < d, ldo < m
        assert lb.xv_score_matrix(0, b.x, lda, 3, b.x, ldb, 5, 8, b.o, ldo, None) == bad
    for lda, ldb in ((7, 8), (8, 7)):
        assert lb.xv_score_pairs(0, b.x, lda, 3, b.x, ldb, 5, 8, b.ip, b.ip, 2, b.o, None) == bad
        assert lb.xv_score_histogram(0, b.x, lda, 3, b.ip, b.o, ldb, 5, b.ip, 8, 0, 256, b.ph1, b.ph2, None) == bad
    # xv_score_prepare: ldx < d_in, ldo < d_out without and with a transform, ldt < t_cols for both column counts
    assert lb.xv_score_prepare(0, b.x, 7, 3, 8, None, None, 0, 8, 0, 1, 0.0, b.o, 8, None) == bad
    assert lb.xv_score_prepare(0, b.x, 8, 3, 8, None, None, 0, 8, 0, 1, 0.0, b.o, 7, None) == bad
    t = ctypes.cast((ctypes.c_float * 4096)(), ctypes.c_void_p)
    assert lb.xv_score_prepare(0, b.x, 7, 3, 8, None, t, 8, 5, 8, 1, 0.0, b.o, 5, None) == bad
    assert lb.xv_score_prepare(0, b.x, 8, 3, 8, None, t, 7, 5, 8, 1, 0.0, b.o, 5, None) == bad
    assert lb.xv_score_prepare(0, b.x, 8, 3, 8, None, t, 8, 5, 9, 1, 0.0, b.o, 5, None) == bad      # t_cols = d_in + 1 needs ldt >= 9
    assert lb.xv_score_prepare(0, b.x, 8, 3, 8, None, t, 9, 5, 9, 1, 0.0, b.o, 4, None) == bad      # ldo < d_out


def test_loss_refuses_a_short_leading_dimension(lib):
    _lib, lb = lib
    b, bad = Host(), _lib.XV_ERR_INVALID
    assert lb.xv_loss_prepare_classes(0, b.x, 4, 8, 5, 0, b.o, 8, None) == bad         # ldk < num_classes
    assert lb.xv_loss_prepare_classes(0, b.x, 5, 8, 5, 0, b.o, 7, None) == bad         # ldc < embed_dim
    ws = int(lb.xv_loss_workspace(3, 5))
    out = [ctypes.cast((ctypes.c_float * 16)(), ctypes.c_void_p) for _ in range(4)]
    wsb = ctypes.cast((ctypes.c_char * ws)(), ctypes.c_void_p)
    for ldx, ldc in ((7, 8), (8, 7)):                                                  # ldx < embed_dim, ldc < embed_dim
        assert lb.xv_loss_classifier(0, b.x, ldx, 3, 8, b.ip, b.o, ldc, 5, None, 0, 0.0, 0.0, out[0], out[1], out[2], out[3], wsb, ws,
                                     None) == bad
