"""Operand layouts for tests of the C ABI (include/xvec_hip.h: "ld >= width", operands anywhere in device memory).

place() / blank() put a [rows, width] matrix into one flat torch allocation, the *frame*, filled with a poison: row r of the
operand starts at element base + r * ld, and at least one full row of slack lies in front of row 0 and behind the last row, so
a kernel that reads or writes a vector too far stays inside the allocation and shows up as a NaN in its result or as a
disturbed canary, never as a fault.

    name      base (elements past a 16-byte boundary)   ld                       what it selects in csrc/score.hip, loss.hip
    tight     0                                         width                    what the wrappers pass
    pad4      0                                         roundup(width, 4) + 4    vector kernels; a partial last float4 when width % 4 != 0
    pad_odd   0                                         width + 1, made odd      scalar kernels through ld % 4
    shift1    1                                         roundup(width, 4) + 4    scalar kernels through the alignment test alone
    shift3    3                                         roundup(width, 4) + 4    the same

Poisons are fixed bit patterns and are compared as raw bits: inputs get a quiet NaN (float) that no arithmetic produces,
outputs a canary (for floats another quiet NaN with a recognisable payload).  Doubles and integers use the same layouts with
offsets counted in elements."""
import numpy as np

LAYOUTS = ("tight", "pad4", "pad_odd", "shift1", "shift3")
# (A, B) layouts of the two-operand calls
PAIRS = (("tight", "tight"), ("pad4", "pad4"), ("pad4", "shift1"), ("shift3", "pad4"), ("pad_odd", "pad_odd"))

_BITS = {      # itemsize -> (unsigned view, NaN poison of inputs, canary of outputs)
    4: (np.uint32, 0x7FC1DEAD, 0x7FC5A5A5),
    8: (np.uint64, 0x7FF81DEAD1DEAD11, 0x7FF8A5A5A5A5A5A5),
}
_INT_CANARY = {4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}


def _roundup(v, q):
    return (v + q - 1) // q * q


def geometry(name, width):
    """-> (base in elements past a 16-byte boundary, ld)."""
    wide = _roundup(width, 4) + 4
    return {"tight": (0, width), "pad4": (0, wide), "pad_odd": (0, width + 1 + (width % 2)), "shift1": (1, wide),
            "shift3": (3, wide)}[name]


def poison_bits(dtype, kind):
    """The fill of a frame as an unsigned integer: kind "nan" (inputs) or "canary" (outputs)."""
    dtype = np.dtype(dtype)
    view, nan, canary = _BITS[dtype.itemsize]
    if dtype.kind != "f":
        return view, _INT_CANARY[dtype.itemsize]
    return view, nan if kind == "nan" else canary


class Frame(object):
    """One flat allocation `buf` (torch, 1-D) holding a [rows, width] window at element `base` with row stride `ld`."""

    def __init__(self, buf, base, rows, width, ld, dtype, bits, layout):
        self.buf, self.base, self.rows, self.width, self.ld = buf, base, rows, width, ld
        self.dtype, self.bits, self.layout = np.dtype(dtype), bits, layout

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.base * self.dtype.itemsize

    def host(self):
        """The whole frame as a host array of the unsigned view."""
        return self.buf.cpu().numpy().view(_BITS[self.dtype.itemsize][0])


def _build(rows, width, layout, device, dtype, kind, src):
    import torch
    dtype = np.dtype(dtype)
    shift, ld = geometry(layout, width)
    view, bits = poison_bits(dtype, kind)
    per16 = 16 // dtype.itemsize
    front = _roundup(ld, per16) + per16             # >= one row, a multiple of 16 bytes
    total = per16 + front + shift + max(rows, 1) * ld + ld + per16
    buf = torch.empty(total, dtype=getattr(torch, dtype.name), device=device)
    assert buf.data_ptr() % dtype.itemsize == 0
    lead = (-buf.data_ptr() % 16) // dtype.itemsize   # elements up to the first 16-byte boundary of the allocation
    base = lead + front + shift
    host = np.full(total, bits, dtype=view)
    if src is not None:
        win = np.lib.stride_tricks.as_strided(host[base:], shape=(rows, width), strides=(ld * host.itemsize, host.itemsize))
        win[...] = np.ascontiguousarray(src, dtype=dtype).view(view)
    buf.copy_(torch.from_numpy(host.view(dtype)))
    return Frame(buf, base, rows, width, ld, dtype, bits, layout)


def place(host, layout, device, poison="nan"):
    """Host array [rows, width] (float32, float64 or an integer type) -> (frame, view_ptr, ld): the rows at
    frame.base + r * ld of a frame otherwise filled with the poison ("nan" for inputs, "canary" for outputs)."""
    host = np.asarray(host)
    assert host.ndim == 2
    f = _build(host.shape[0], host.shape[1], layout, device, host.dtype, poison, host)
    return f, f.ptr, f.ld


def blank(rows, width, layout, device, dtype=np.float32):
    """An output operand: a frame that is canary everywhere, the window included -> (frame, view_ptr, ld)."""
    f = _build(rows, width, layout, device, dtype, "canary", None)
    return f, f.ptr, f.ld


def _window_mask(n, rows, width, ld, base):
    mask = np.zeros(n, dtype=bool)
    idx = base + (np.arange(rows)[:, None] * ld + np.arange(width)[None, :])
    mask[idx.reshape(-1)] = True
    return mask


def untouched(frame, rows=None, width=None, ld=None, base=None):
    """True when every element of the frame outside the [rows, width] window still holds the frame's poison, bit for bit."""
    rows = frame.rows if rows is None else rows
    width = frame.width if width is None else width
    ld = frame.ld if ld is None else ld
    base = frame.base if base is None else base
    h = frame.host()
    return bool(np.all(h[~_window_mask(h.shape[0], rows, width, ld, base)] == frame.bits))


def gather(frame, rows=None, width=None, ld=None, base=None):
    """The window as a contiguous host array of the frame's dtype."""
    rows = frame.rows if rows is None else rows
    width = frame.width if width is None else width
    ld = frame.ld if ld is None else ld
    base = frame.base if base is None else base
    h = frame.host()
    idx = base + (np.arange(rows)[:, None] * ld + np.arange(width)[None, :])
    return np.ascontiguousarray(h[idx]).view(frame.dtype)


def intact(frame, src):
    """An input after a call: the window still equals `src` bit for bit and everything else is poison."""
    view = _BITS[frame.dtype.itemsize][0]
    want = np.ascontiguousarray(src, dtype=frame.dtype).view(view)
    return untouched(frame) and bool(np.array_equal(gather(frame).view(view), want))
