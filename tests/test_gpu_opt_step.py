"""GPU: xv_opt_step (csrc/opt_step.hip) against the float32 numpy oracle tests/helpers/ref_loss_grad.opt_step, bit for bit:
the header states the operation order and every operation is rounded on its own."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref_loss_grad as rg                                          # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = (1, 255, 256, 257, 70001)
KINDS = [("sgd", rg.SGD, False), ("momentum", rg.MOMENTUM, False), ("nesterov", rg.MOMENTUM, True), ("adam", rg.ADAM, False)]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def gpu_step(kind, nesterov, w, g, s0, s1, lr, l2, clip, mom, step):
    """One xv_opt_step on device tensors (updated in place) -> rc."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    ws = torch.empty(max(int(lib.xv_opt_workspace(w.numel())), 8), dtype=torch.uint8, device="cuda")
    ws.fill_(0xFF)
    rc = lib.xv_opt_step(0, kind, int(nesterov), _p(w), _p(g), _p(s0), _p(s1), w.numel(), lr, l2, clip, mom, step, _p(ws), ws.numel(), None)
    torch.cuda.synchronize()
    return rc


def run_three(count, kind, nesterov, l2, clip, first_step, seed=0):
    """Three consecutive steps on the GPU and in numpy -> nothing; asserts equal bits of w and the slots after each."""
    import torch
    rs = np.random.RandomState(seed + count)
    w = rs.standard_normal(count).astype(np.float32)
    s0 = None if kind == rg.SGD else (0.1 * rs.standard_normal(count)).astype(np.float32)
    s1 = None if kind != rg.ADAM else (0.01 * rs.standard_normal(count) ** 2).astype(np.float32)
    wd = torch.from_numpy(w).cuda()
    s0d = None if s0 is None else torch.from_numpy(s0).cuda()
    s1d = None if s1 is None else torch.from_numpy(s1).cuda()
    for k in range(3):
        g = (rs.standard_normal(count) * 0.5).astype(np.float32)
        gd = torch.from_numpy(g).cuda()
        cn = clip(g, w, l2) if callable(clip) else clip
        assert gpu_step(kind, nesterov, wd, gd, s0d, s1d, 0.05, l2, cn, 0.9, first_step + k) == 0
        w, s0, s1 = rg.opt_step(kind, w, g, s0, s1, lr=0.05, l2=l2, clip_norm=cn, momentum=0.9, use_nesterov=nesterov,
                                step=first_step + k)
        assert gd.cpu().numpy().tobytes() == g.tobytes()                              # the gradient is not written
        assert wd.cpu().numpy().tobytes() == w.tobytes(), ("w", count, k)
        if s0 is not None:
            assert s0d.cpu().numpy().tobytes() == s0.tobytes(), ("slot0", count, k)
        if s1 is not None:
            assert s1d.cpu().numpy().tobytes() == s1.tobytes(), ("slot1", count, k)
    return wd.cpu().numpy()


@pytest.mark.parametrize("name,kind,nesterov", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("count", COUNTS)
def test_three_steps_are_bit_equal_to_numpy(count, name, kind, nesterov):
    for first_step in (1, 7):
        for l2 in (0.0, 1e-2):
            a = run_three(count, kind, nesterov, l2, 0.0, first_step)
            b = run_three(count, kind, nesterov, l2, 0.0, first_step)
            assert a.tobytes() == b.tobytes()                                         # repeats


@pytest.mark.parametrize("count", COUNTS)
def test_clip_above_below_and_at_the_norm(count):
    def norm_of(g, w, l2):
        gg = g + np.float32(l2) * w if l2 else g
        return float(rg.grad_norm(gg))
    for l2 in (0.0, 1e-2):
        run_three(count, rg.MOMENTUM, False, l2, 1e6, 1)                              # clip_norm above ||g||: g * c / c
        run_three(count, rg.SGD, False, l2, 1e-3, 1)                                  # below: scaled down
        run_three(count, rg.ADAM, False, l2, lambda g, w, l2=l2: norm_of(g, w, l2), 7)   # equal to ||g||
    import torch
    g = np.array([3.0, 4.0], dtype=np.float32)                                        # ||g|| = 5 exactly
    wd, gd = torch.zeros(2, device="cuda"), torch.from_numpy(g).cuda()
    assert gpu_step(rg.SGD, False, wd, gd, None, None, 1.0, 0.0, 5.0, 0.0, 1) == 0
    assert wd.cpu().numpy().tobytes() == (-g).tobytes()
    assert float(rg.grad_norm(g)) == 5.0


def test_invalid_arguments_are_refused_before_any_launch():
    import torch
    from tf_kaldi_speaker_amd import _lib
    w = torch.ones(8, device="cuda")
    g = torch.ones(8, device="cuda")
    a = torch.zeros(8, device="cuda")
    bad = [dict(lr=float("nan")), dict(lr=float("inf")), dict(lr=-0.1), dict(l2=-1e-3), dict(clip=-1.0), dict(kind=3), dict(kind=-1)]
    for kw in bad:
        args = dict(kind=rg.MOMENTUM, lr=0.1, l2=0.0, clip=0.0)
        args.update(kw)
        rc = gpu_step(args["kind"], False, w, g, a, a.clone(), args["lr"], args["l2"], args["clip"], 0.9, 1)
        assert rc == _lib.XV_ERR_INVALID, kw
    assert gpu_step(rg.ADAM, False, w, g, a, None, 0.1, 0.0, 0.0, 0.9, 1) == _lib.XV_ERR_INVALID      # adam needs both slots
    assert gpu_step(rg.ADAM, False, w, g, a, a.clone(), 0.1, 0.0, 0.0, 0.9, 0) == _lib.XV_ERR_INVALID  # steps count from 1
    lib = _lib.load()
    assert lib.xv_opt_step(0, rg.SGD, 0, _p(w), _p(g), None, None, 8, 0.1, 0.0, 1.0, 0.0, 1, None, 0, None) == _lib.XV_ERR_WORKSPACE
    assert np.all(w.cpu().numpy() == 1.0) and np.all(a.cpu().numpy() == 0.0)
