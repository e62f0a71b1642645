"""The inputs of tests/test_gpu_pool_grad.py and tests/test_pool_grad_host.py (statistics pooling of packed rows and its
gradient, csrc/pool_grad.hip), and the toy data of tests/test_gpu_frame_train.py.

One batch: twelve utterances of LENGTHS frames, packed back to back behind LEAD rows that no utterance owns, so that no
utterance starts at an aligned row.  Channel classes, by c mod 4 for C >= 4 (so that the four adjacent columns of one 16-byte
access hold different classes):
    0 ordinary     N(0, 1)
    1 offset       N(0, 1) 2^-4 + 100: a mean far above the spread (the one-pass variance E[x^2] - m^2 loses it)
    2 ordinary     N(0, 1) times a per-channel scale in [2^-3, 2^3]
    3 ordinary     as 0
and ONE constant channel, CONST_VALUE on every frame: a power of two, so that every partial sum, the division and x - m are
exact, the variance is an exact zero and the channel is floored in the kernel exactly as in float64.  For C >= 5 the channel
behind it is NEAR constant, 0.5 +- 2^-21 on alternating frames: its variance, about 2.3e-13, is floored in float32 and in
float64 alike while x - m is not zero, so a backward that ignores the floor mask is far off there (b d would be of the size of
a).  C < 4: ordinary channels, the constant one where C > 1.  The seeds are fixed here."""
import numpy as np

F = np.float32
CHANNELS = (1, 3, 4, 5, 63, 64, 65, 257)
LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025)
LEAD = 3
CONST_VALUE = 0.5
NEAR_STEP = 2.0 ** -21


def const_channel(C):
    return None if C == 1 else C // 2


def offsets():
    return np.concatenate([[LEAD], LEAD + np.cumsum(LENGTHS)]).astype(np.int32)


def make(C, seed=None):
    """-> dict(x [rows, C] float32 (the LEAD unowned rows are NaN), offsets int32 [13], gp [12, 2 C] float32, const)."""
    r = np.random.RandomState(1000 + C if seed is None else seed)
    off = offsets()
    rows = int(off[-1])
    x = r.standard_normal((rows, C)).astype(F)
    if C >= 4:
        cls = np.arange(C) % 4
        x[:, cls == 1] = (x[:, cls == 1] * F(2.0 ** -4) + F(100.0)).astype(F)
        scale = (2.0 ** r.randint(-3, 4, C)).astype(F)
        x[:, cls == 2] *= scale[cls == 2][None, :]
    const = const_channel(C)
    if const is not None:
        x[:, const] = CONST_VALUE
    if C >= 5:
        x[:, const + 1] = (CONST_VALUE + NEAR_STEP * (1.0 - 2.0 * (np.arange(rows) % 2))).astype(F)
    x[:LEAD] = np.nan
    gp = r.standard_normal((len(LENGTHS), 2 * C)).astype(F)
    return dict(x=x, offsets=off, gp=gp, const=const, C=C)


def utterance(case, u):
    """The rows of utterance u."""
    return case["x"][case["offsets"][u]:case["offsets"][u + 1]]


# ---------------------------------------------------------------------------------------------- the frame trainer's toy task
def separable_frames(seed, speakers, segments, dim, lengths):
    """Packed frames of a separable toy set, as a ReLU node hands them on: `speakers` centres, `segments` utterances each, the
    utterance lengths cycling through `lengths` -> (frames [rows, dim] float32 >= 0, offsets int32, labels int32)."""
    r = np.random.RandomState(seed)
    centres = r.standard_normal((speakers, dim))
    labels = np.repeat(np.arange(speakers), segments)
    lens = [int(lengths[i % len(lengths)]) for i in range(labels.size)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    frames = np.concatenate([centres[l][None, :] + 0.5 * r.standard_normal((n, dim)) for l, n in zip(labels, lens)])
    return np.maximum(frames, 0.0).astype(F), off, labels.astype(np.int32)
