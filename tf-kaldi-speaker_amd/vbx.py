"""VB-HMM resegmentation of clustered x-vectors on the GPU (xv_vbx, csrc/vbx.hip): the step current x-vector diarization
recipes put after the first clustering, "VBx" (Landini et al., "Bayesian HMM clustering of x-vector sequences", 2022; the
function VBx of the published VB_diarization.py).  The labels of cluster.py initialise a Bayesian HMM whose states are the
speakers, each a Gaussian in the PLDA space with the between-class variances psi as its prior; a few tens of variational
iterations, each with a forward-backward pass over the recording, let surplus speakers die out and smooth the labels in
time.  Neither the reference nor Kaldi's x-vector recipe has the step: **parity unpinned**; include/xvec_hip.h states the
rule and tests/helpers/ref_vbx.py restates it in numpy.

    vb_hmm(model, rows, offsets, gamma, pi, ...)     the raw batch call: start values in, final values out
    resegment(model, x, groups, init_labels, ...)    front, start values from labels, batching, final renumbering

The model is a plda.Plda (its affine is [transform | -transform mean]) or a plda.AdaptedPlda (its own affine); lda_dim = k
keeps the first k rows.  No length normalisation happens behind the affine.  Everything needs a HIP device (no CPU path)."""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr
from . import scoring

MAX_ROWS = 8192
MAX_SPEAKERS = 64
MAX_DIM = 256
BUDGET_BYTES = 1 << 30            # what gamma, the outputs and the workspace of one xv_vbx call may take together

RawResult = collections.namedtuple("RawResult", ["gamma", "pi", "elbo", "iters", "labels"])
VbxResult = collections.namedtuple("VbxResult", ["labels", "gamma", "pi", "elbo", "iterations", "num_speakers"])

DEFAULTS = dict(fa=0.3, fb=17.0, loop_prob=0.99, max_iters=40, epsilon=1e-6)


def model_operands(model, lda_dim=None):
    """(A [r, D + 1], psi [r]) float64 of a plda.Plda or plda.AdaptedPlda, the first lda_dim rows / entries."""
    from . import plda
    if isinstance(model, plda.AdaptedPlda):
        a = model.affine
    else:
        a = np.concatenate([model.transform, -(model.transform @ model.mean)[:, None]], axis=1)
    r = a.shape[0]
    if lda_dim is not None:
        if not 1 <= int(lda_dim) <= r:
            raise ValueError("lda_dim = %r for a model of dimension %d" % (lda_dim, r))
        r = int(lda_dim)
    if r > MAX_DIM:
        raise ValueError("a model of dimension %d: at most %d (use lda_dim)" % (r, MAX_DIM))
    return np.ascontiguousarray(a[:r], dtype=np.float64), np.ascontiguousarray(model.psi[:r], dtype=np.float64)


def _operands_device(model, lda_dim, device, torch):
    key = ("vbx", device, lda_dim)
    if key not in model._device:
        model._device[key] = tuple(torch.from_numpy(t).to("cuda:%d" % device) for t in model_operands(model, lda_dim))
    return model._device[key]


def _f64(t, device, torch, what):
    if isinstance(t, torch.Tensor):
        out = t.to(device="cuda:%d" % device, dtype=torch.float64).reshape(-1).clone()
    else:
        out = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64).reshape(-1)).to("cuda:%d" % device)
    return out.contiguous()


def check_options(fa, fb, loop_prob, max_iters, epsilon):
    """The option rules of xv_vbx as ValueError -> (fa, fb, loop_prob, max_iters, epsilon) as floats / int."""
    fa, fb, loop_prob, epsilon = float(fa), float(fb), float(loop_prob), float(epsilon)
    if not (0.0 < fa < np.inf and 0.0 < fb < np.inf):
        raise ValueError("fa and fb must be positive and finite, got %r, %r" % (fa, fb))
    if not 0.0 <= loop_prob <= 1.0:
        raise ValueError("loop_prob must be in [0, 1], got %r" % (loop_prob,))
    if int(max_iters) != max_iters or int(max_iters) < 1:
        raise ValueError("max_iters must be an integer >= 1, got %r" % (max_iters,))
    if epsilon != epsilon:
        raise ValueError("epsilon is NaN (-inf means: run all max_iters iterations)")
    return fa, fb, loop_prob, int(max_iters), epsilon


def vb_hmm(model, rows, offsets, gamma, pi, num_spk=None, fa=0.3, fb=17.0, loop_prob=0.99, max_iters=40, epsilon=1e-6,
           lda_dim=None, device=0, as_tensor=False, ws_bytes=None):
    """One xv_vbx call.  `rows` [N, D] float32 (numpy or a device tensor) are the x-vectors behind the front, sorted by group
    and in time order inside a group; group g owns the rows offsets[g] .. offsets[g + 1].  Start values: `gamma` and `pi` are
    lists with one [T_g, S_g] and one [S_g] array per group, or, with `num_spk` [G], the packed 1-D buffers of the C ABI
    (group g at the offsets sum_{h<g} T_h S_h and sum_{h<g} S_h); gamma has rows >= 0 and pi is >= 0 with a positive sum.
    -> RawResult(gamma, pi, elbo [G, max_iters] with NaN past the iterations run, iters [G] int32, labels [N] int32), gamma and
    pi packed; numpy, or device tensors with as_tensor.  `ws_bytes` None takes the least workspace; by the rule the result
    does not depend on it."""
    fa, fb, loop_prob, max_iters, epsilon = check_options(fa, fb, loop_prob, max_iters, epsilon)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    groups = offsets.shape[0] - 1
    if groups < 0:
        raise ValueError("offsets: expected [G + 1] entries")
    sizes = np.diff(offsets)
    if isinstance(gamma, (list, tuple)):
        if len(gamma) != groups or len(pi) != groups:
            raise ValueError("gamma, pi: %d and %d entries for %d groups" % (len(gamma), len(pi), groups))
        for g, (ga, p) in enumerate(zip(gamma, pi)):
            if np.ndim(ga) != 2 or np.shape(ga)[0] != sizes[g] or np.shape(p) != (np.shape(ga)[1],):
                raise ValueError("group %d: gamma of shape %s and pi of shape %s for %d rows" % (g, np.shape(ga), np.shape(p), sizes[g]))
        num_spk = [np.shape(ga)[1] for ga in gamma]
        gamma = np.concatenate([np.asarray(ga, np.float64).reshape(-1) for ga in gamma]) if groups else np.zeros(0)
        pi = np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in pi]) if groups else np.zeros(0)
    elif num_spk is None:
        raise ValueError("packed gamma and pi need num_spk")
    spk = np.ascontiguousarray(num_spk, dtype=np.int32).reshape(-1)
    if spk.shape[0] != groups:
        raise ValueError("num_spk: %d entries for %d groups" % (spk.shape[0], groups))
    torch = scoring._need_device()
    lib = _lib.load()
    cells, total_spk = int(np.sum(sizes * spk)), int(spk.sum())
    with torch.cuda.device(device):
        dev = torch.device("cuda:%d" % device)
        xd = scoring._rows(rows, device, "rows")
        a, psi = _operands_device(model, lda_dim, device, torch)
        r, d = int(a.shape[0]), int(a.shape[1]) - 1
        if int(xd.shape[1]) != d:
            raise ValueError("rows of dimension %d for a model that takes %d" % (int(xd.shape[1]), d))
        if groups and int(offsets[-1]) > int(xd.shape[0]):
            raise ValueError("offsets end at %d, there are %d rows" % (int(offsets[-1]), int(xd.shape[0])))
        gd, pd = _f64(gamma, device, torch, "gamma"), _f64(pi, device, torch, "pi")
        if gd.numel() != cells or pd.numel() != total_spk:
            raise ValueError("gamma, pi: %d and %d entries, the groups need %d and %d" % (gd.numel(), pd.numel(), cells, total_spk))
        labels = torch.empty((max(int(xd.shape[0]), 1),), dtype=torch.int32, device=dev)
        elbo = torch.empty((max(groups, 1), max_iters), dtype=torch.float64, device=dev)
        iters = torch.empty((max(groups, 1),), dtype=torch.int32, device=dev)
        need = int(lib.xv_vbx_workspace(groups, offsets.ctypes.data_as(C.c_void_p), spk.ctypes.data_as(C.c_void_p), r))
        if need < 0:
            raise _lib.XvError(need, (lib.xv_last_error(None) or b"").decode("utf-8", "replace"))
        size = need if ws_bytes is None else int(ws_bytes)
        ws = torch.empty((max(size, 8),), dtype=torch.uint8, device=dev)
        stream = _lib.stream(device)
        _lib.check(lib.xv_vbx(device, ptr(xd), d, offsets.ctypes.data_as(C.c_void_p), spk.ctypes.data_as(C.c_void_p), groups, d, ptr(a),
                              ptr(psi), r, ptr(gd), ptr(pd), fa, fb, loop_prob, max_iters, epsilon, ptr(labels), ptr(elbo), ptr(iters), ptr(ws),
                              size, stream))
        lo, hi = (int(offsets[0]), int(offsets[-1])) if groups else (0, 0)
        out = RawResult(gd, pd, elbo[:groups], iters[:groups], labels[lo:hi])
        if not as_tensor:
            out = RawResult(*(t.cpu().numpy() for t in out))
    return out


# ---------------------------------------------------------------------------------------------------- host pieces

def map_labels(labels):
    """Any integers -> (0 .. S - 1 by first appearance [T] int64, S)."""
    labels = np.asarray(labels).reshape(-1)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(first.shape[0], np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.shape[0])
    return rank[inverse.reshape(-1)], int(first.shape[0])


def init_gamma(labels, num_spk, smoothing=5.0):
    """The published start: gamma = the row softmax of smoothing * onehot(label) [T, S], pi = 1 / S."""
    labels = np.asarray(labels, np.int64)
    z = np.zeros((labels.shape[0], num_spk))
    z[np.arange(labels.shape[0]), labels] = float(smoothing)
    e = np.exp(z - z.max(axis=1, keepdims=True)) if labels.shape[0] else z
    return e / e.sum(axis=1, keepdims=True), np.full(num_spk, 1.0 / num_spk)


def _call_bytes(t, s, r, max_iters):
    """Device bytes one group adds to a call: workspace, gamma, labels, its ELBO row."""
    return 8 * (t * (r + 2) + 3 * t * s) + 8 * t * s + 4 * t + 8 * max_iters + 8 * s + 36


def _chunks(sizes, spk, r, max_iters, budget):
    """The groups in order, in runs whose device bytes fit `budget` together (a run holds at least one group)."""
    runs, cur, used = [], [], 0
    for g, (t, s) in enumerate(zip(sizes, spk)):
        need = _call_bytes(int(t), int(s), r, max_iters)
        if cur and used + need > budget:
            runs.append(cur)
            cur, used = [], 0
        cur.append(g)
        used += need
    if cur:
        runs.append(cur)
    return runs


def resegment(model, x, groups, init_labels, fa=0.3, fb=17.0, loop_prob=0.99, init_smoothing=5.0, max_iters=40, epsilon=1e-6,
              lda_dim=None, mean=None, transform=None, normalize=True, device=0, budget=None):
    """Resegment every group (recording) of the rows x [N, d] from the labels of a first clustering -> (labels [N] int32 in
    input order, OrderedDict group -> VbxResult(labels, gamma [T, S], pi [S], elbo [iterations], iterations, num_speakers)
    in sorted group order).  `groups` [N] holds one id per row (anything np.unique sorts); a group's rows are taken in input
    order, which must be time order.  `init_labels` [N] are any integers; per recording they are mapped to 0 .. S - 1 by first
    appearance, and more than 64 distinct ones are a ValueError.  The start is gamma = softmax(init_smoothing * onehot),
    pi = 1 / S.  mean / transform / normalize are the front of scoring.prepare before the model.  `model` is a plda.Plda for
    all recordings, or a dict recording -> plda.AdaptedPlda (plda.adapt_groups; every recording needs one), which costs one
    call per recording.  The final labels number the surviving speakers (those some row is assigned to) by their lowest row;
    VbxResult.gamma and pi keep the columns of the start."""
    from . import cluster
    n, _ = scoring._shape2(x, "x")
    labels_in = np.asarray(init_labels).reshape(-1)
    if labels_in.shape[0] != n:
        raise ValueError("init_labels: %d labels for %d rows" % (labels_in.shape[0], n))
    fa, fb, loop_prob, max_iters, epsilon = check_options(fa, fb, loop_prob, max_iters, epsilon)
    names, members = cluster._group_rows(groups, n)
    starts, spk = [], []
    for name, m in zip(names, members):
        if len(m) > MAX_ROWS:
            raise ValueError("recording %s has %d rows: at most %d; split the recording" % (name, len(m), MAX_ROWS))
        lab, s = map_labels(labels_in[m])
        if s > MAX_SPEAKERS:
            raise ValueError("recording %s has %d distinct initial labels: at most %d" % (name, s, MAX_SPEAKERS))
        starts.append(init_gamma(lab, s, init_smoothing))
        spk.append(s)
    per_model = isinstance(model, dict)
    if per_model:
        missing = [k for k in names if model.get(k) is None]
        if missing:
            raise ValueError("%d recordings have no adapted model (first: %s)" % (len(missing), missing[0]))
    torch = scoring._need_device()
    front = mean is not None or transform is not None or normalize
    rows = scoring.prepare(x, mean=mean, transform=transform, normalize=normalize, device=device, as_tensor=True) if front else x
    opts = dict(fa=fa, fb=fb, loop_prob=loop_prob, max_iters=max_iters, epsilon=epsilon, lda_dim=lda_dim, device=device)
    sizes = [len(m) for m in members]
    with torch.cuda.device(device):
        rows = scoring._rows(rows, device, "x")
        order = np.concatenate(members) if members else np.zeros(0, np.int64)
        xs = rows[torch.from_numpy(order).to(rows.device)].contiguous()
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if per_model:
        runs = [[g] for g in range(len(names))]
    else:
        r = model_operands(model, lda_dim)[0].shape[0]
        runs = _chunks(sizes, spk, r, max_iters, BUDGET_BYTES if budget is None else int(budget))
    labels = np.zeros(n, np.int32)
    out = [None] * len(names)
    for run in runs:
        g0, g1 = run[0], run[-1] + 1
        raw = vb_hmm(model[names[g0]] if per_model else model, xs, bounds[g0:g1 + 1], [starts[g][0] for g in run],
                     [starts[g][1] for g in run], **opts)
        go = po = ro = 0
        for i, g in enumerate(run):
            t, s = sizes[g], spk[g]
            lab, kept = map_labels(raw.labels[ro:ro + t])
            it = int(raw.iters[i])
            out[g] = VbxResult(lab.astype(np.int32), raw.gamma[go:go + t * s].reshape(t, s).copy(), raw.pi[po:po + s].copy(),
                               raw.elbo[i, :it].copy(), it, kept if t else 0)
            labels[members[g]] = out[g].labels
            go, po, ro = go + t * s, po + s, ro + t
    return labels, collections.OrderedDict(zip(names, out))
