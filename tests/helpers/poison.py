"""Defined garbage for the memory the library does not clear.

The library clears almost nothing: every byte a kernel reads from the caller's workspace or output must have been written
earlier in the same call ("The workspace contract").  A test that hands the library `torch.empty` memory cannot
see a violation, because that memory is either fresh (zero) or whatever the caching allocator's previous tenant left there.
The tests built on this module put a chosen byte under every buffer and require the same bits for every choice.

FILLS, and why each byte:

0xFF    NaN in f32, f16 and bf16; NaN as an E8M0 block scale; -1 as an index or a count.  Catches a garbage read even
        under a zero weight (NaN x 0 = NaN).
0x7B    about 1.3e36 in f32 and as a bf16 pair, 61 280 in f16, a legal fp6 code, an E8M0 scale of 2^-4.  Catches the reads
        a max launders away: a ReLU or a max-pool written with fmaxf returns its non-NaN operand, so NaN poison can vanish
        there.  This byte is a large finite positive number in every format the kernels read, so it survives.
0x00    zero everywhere.  The baseline the other two are compared with -- and what a fresh allocation usually looks like,
        that is, what the suite has effectively tested before.
"""
import torch

FILLS = (0x00, 0xFF, 0x7B)


def fill(t, byte):
    """Fill the contiguous tensor `t` bytewise with `byte` (on the current stream for a device tensor); returns `t`."""
    assert 0 <= byte <= 0xFF and t.is_contiguous()
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(byte)
    return t


def poisoned_empty(monkeypatch, byte):
    """Replace `torch.empty` until the end of the test (pytest's monkeypatch restores it): every tensor it returns for a
    CUDA device, and every pinned host tensor (the kernels write results straight into those), comes back filled with
    `byte`.  Plain host tensors are filled as well -- they are what the host test can look at.  The op wrappers call
    `torch.empty` through the module attribute, so they get the replacement; `torch.zeros` and `torch.full` are untouched:
    a wrapper that asks for zeros has made that part of its own contract.  A request it cannot fill (not strided, or not
    contiguous, such as channels_last) fails an assertion instead of escaping the poison.  Returns the list of
    (shape, dtype, where) of the requests served, `where` being "cuda", "pinned" or "cpu", so that a test can tell that a
    wrapper really allocated device-visible memory through it."""
    real = getattr(torch.empty, "poison_real", torch.empty)      # a second call in one test replaces the first, it does not stack
    served = []

    def empty(*args, **kwargs):
        t = real(*args, **kwargs)
        # nothing may escape the poison: a wrapper that starts to allocate another layout or memory format fails here
        assert t.layout == torch.strided and t.is_contiguous(), \
            ("poisoned_empty cannot fill this request", args, kwargs)
        fill(t, byte)
        served.append((tuple(t.shape), t.dtype, "pinned" if kwargs.get("pin_memory") else t.device.type))
        return t

    empty.poison_real = real
    monkeypatch.setattr(torch, "empty", empty)
    return served
