"""Host: tests/helpers/poison.py itself -- the replacement of torch.empty fills what it hands out, leaves torch.zeros alone
and is gone when the test that installed it ends.  No GPU: CPU and (where the build can pin memory) pinned tensors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import poison                                                                   # noqa: E402

DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.float32, torch.float64]
_REAL_EMPTY = torch.empty                       # bound at import, before any test patches it


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8).numpy()


def test_fills_have_their_documented_meaning():
    assert poison.FILLS == (0x00, 0xFF, 0x7B)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert torch.isnan(poison.fill(_REAL_EMPTY(4, dtype=dt), 0xFF)).all(), dt
        big = poison.fill(_REAL_EMPTY(4, dtype=dt), 0x7B).double()
        assert torch.isfinite(big).all() and (big > 6.0e4).all(), dt
    assert float(poison.fill(_REAL_EMPTY(1, dtype=torch.float16), 0x7B)[0]) == 61280.0
    assert abs(float(poison.fill(_REAL_EMPTY(1), 0x7B)[0]) / 1.3e36 - 1.0) < 0.01
    assert int(poison.fill(_REAL_EMPTY(1, dtype=torch.int32), 0xFF)[0]) == -1
    assert 0x7B - 127 == -4                                                    # E8M0: 2^(byte - 127)
    assert torch.equal(poison.fill(_REAL_EMPTY(3, 5), 0x00), torch.zeros(3, 5))


@pytest.mark.parametrize("byte", poison.FILLS)
def test_replacement_fills_every_dtype_and_size(monkeypatch, byte):
    served = poison.poisoned_empty(monkeypatch, byte)
    assert torch.empty is not _REAL_EMPTY
    n = 0
    for dt in DTYPES:
        for shape in ((0,), (7,), (3, 5), (2, 0, 4), (1025,)):
            for t in (torch.empty(shape, dtype=dt), torch.empty(*shape, dtype=dt, device="cpu")):
                n += 1
                assert t.shape == shape and t.dtype == dt
                assert np.all(_bytes(t) == byte), (dt, shape)
    assert len(served) == n and served[-1] == ((1025,), torch.float64, "cpu")


@pytest.mark.parametrize("byte", poison.FILLS)
def test_replacement_fills_pinned_tensors(monkeypatch, byte):
    try:
        _REAL_EMPTY(1, pin_memory=True)
    except RuntimeError:                        # a build or a machine that cannot pin: the request must still fail the same way
        poison.poisoned_empty(monkeypatch, byte)
        with pytest.raises(RuntimeError):
            torch.empty(1, pin_memory=True)
        return
    served = poison.poisoned_empty(monkeypatch, byte)
    for dt in DTYPES:
        for shape in ((0,), (9,), (4, 6)):
            t = torch.empty(shape, dtype=dt, pin_memory=True)
            assert t.is_pinned() or t.numel() == 0
            assert np.all(_bytes(t) == byte), (dt, shape)
            assert served[-1] == (shape, dt, "pinned")


def test_a_request_it_cannot_fill_is_refused(monkeypatch):
    """A memory format or a layout that `fill` cannot reach bytewise must not come back unpoisoned."""
    poison.poisoned_empty(monkeypatch, 0xFF)
    with pytest.raises(AssertionError):
        torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
    with pytest.raises(AssertionError):
        torch.empty((4, 4), layout=torch.sparse_coo)
    assert np.all(_bytes(torch.empty((2, 3, 4, 5))) == 0xFF)


def test_zeros_and_full_are_left_alone(monkeypatch):
    zeros, full = torch.zeros, torch.full
    poison.poisoned_empty(monkeypatch, 0xFF)
    assert torch.zeros is zeros and torch.full is full
    for dt in DTYPES:
        assert not _bytes(torch.zeros((5, 3), dtype=dt)).any(), dt
    assert torch.equal(torch.full((4,), 2.5), torch.tensor([2.5] * 4))
    assert torch.equal(torch.zeros_like(torch.empty(6)), torch.zeros(6))


def test_empty_is_restored_afterwards():
    """Runs behind the tests above (file order): their monkeypatch fixtures have been undone."""
    assert torch.empty is _REAL_EMPTY
    with pytest.MonkeyPatch.context() as mp:
        poison.poisoned_empty(mp, 0x7B)
        assert torch.empty is not _REAL_EMPTY
        assert np.all(_bytes(torch.empty(8)) == 0x7B)
    assert torch.empty is _REAL_EMPTY
