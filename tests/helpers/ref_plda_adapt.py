"""ORACLE (test infrastructure only) of the per-recording PCA adaptation of a PLDA model (include/xvec_hip.h, xv_plda_adapt),
numpy, float64 throughout, in two forms: the chain the GPU runs (covariance, eigendecomposition, energy rule, projection,
simultaneous diagonalisation: `adapt`), with numpy.linalg.eigh / cholesky in place of the Jacobi iteration, and the log
likelihood ratio of the projected Gaussian model (P m, P W P^T, P B P^T) written without any diagonalisation (`llr_direct`).
Kaldi is absent from the reference tree: the steps follow ivector-plda-scoring-dense.cc and Plda::ApplyTransform as published
(**parity unpinned**, as tests/helpers/ref_plda.py)."""
import collections

import numpy as np

Adapted = collections.namedtuple("Adapted", ["dim", "eigenvalues", "pca", "affine", "psi", "cov", "w_proj", "b_proj"])


def covariance(x):
    """Rows x [n, D] (the float32 values) -> (mu, C = (1/n) sum (x - mu)(x - mu)^T), double; mu is the sum in row order / n."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    mu = np.add.accumulate(x, axis=0)[-1] / n               # one addition per row, in row order
    y = x - mu[None, :]
    return mu, (y.T @ y) / n


def energy_dim(lam, target_energy):
    """lam descending -> r: the least k >= 1 whose leading sum exceeds target_energy * trace, plus one, at most D; D when no
    k does.  Sums run in descending order, one addition per eigenvalue."""
    lam = np.asarray(lam, np.float64)
    d = lam.shape[0]
    trace = 0.0
    for v in lam:
        trace += float(v)
    cum = 0.0
    for k in range(1, d + 1):
        cum += float(lam[k - 1])
        if cum > target_energy * trace:
            return min(k + 1, d)
    return d


def energy_fractions(lam):
    """Cumulative energy fractions of the descending spectrum (what the test keeps away from target_energy)."""
    lam = np.asarray(lam, np.float64)
    return np.cumsum(lam) / np.sum(lam)


def fix_signs(rows):
    """Every row scaled by +-1 so that its entry of largest magnitude (the lowest column among equals) is positive."""
    rows = np.array(rows, np.float64)
    for r in rows:
        j = int(np.argmax(np.abs(r)))
        if r[j] < 0.0:
            r *= -1.0
    return rows


def sorted_eigh(c):
    """eigh with the spectrum descending -> (lam [D], vectors as ROWS [D, D])."""
    lam, v = np.linalg.eigh(c)
    order = np.argsort(-lam, kind="stable")
    return lam[order], v[:, order].T.copy()


def model_from_p(mean, transform, psi, p):
    """Steps 5-8 for a given P [r, D] (rows with their signs fixed) -> (affine [r, D + 1], psi' [r], W', B'), or None when the
    Cholesky of W' fails."""
    mean, transform, psi, p = (np.asarray(a, np.float64) for a in (mean, transform, psi, p))
    m = p @ np.linalg.inv(transform)
    w = m @ m.T
    b = (m * psi[None, :]) @ m.T
    try:
        low = np.linalg.cholesky(w)
    except np.linalg.LinAlgError:
        return None
    linv = np.linalg.inv(low)
    k = linv @ b @ linv.T
    psi2, urows = sorted_eigh(0.5 * (k + k.T))
    ap = (urows @ linv) @ p
    affine = fix_signs(np.concatenate([ap, -(ap @ mean)[:, None]], axis=1))
    return affine, np.maximum(psi2, 0.0), w, b


def adapt(mean, transform, psi, x, target_energy):
    """Chain 1-8 for one group -> Adapted, or None for a fallback group (n < 2, trace not > 0, a Cholesky that fails)."""
    mean, transform, psi = (np.asarray(a, np.float64) for a in (mean, transform, psi))
    x = np.asarray(x, np.float64)
    if x.shape[0] < 2:
        return None
    d = x.shape[1]
    _, c = covariance(x)
    lam, vrows = sorted_eigh(c)
    if not np.sum(lam) > 0.0:
        return None
    r = energy_dim(lam, target_energy)
    p = fix_signs(vrows[:r])
    model = model_from_p(mean, transform, psi, p)
    if model is None:
        return None
    affine, psi2, w, b = model
    assert affine.shape == (r, d + 1)
    return Adapted(r, lam, p, affine, psi2, c, w, b)


def llr_adapted(ad, x, normalize_length=True):
    """Step 9 on the rows x [n, D] of the group, both sides one utterance -> [n, n]: u = T [x; 1], TransformIvector and
    LogLikelihoodRatio of tests/helpers/ref_plda.py with psi' and dimension r."""
    import ref_plda
    x = np.asarray(x, np.float64)
    u = x @ ad.affine[:, :-1].T + ad.affine[:, -1][None, :]
    ident = np.eye(ad.dim)
    y = ref_plda.transform_ivector(np.zeros(ad.dim), ident, ad.psi, u, 1, normalize_length=normalize_length)
    return ref_plda.llr(ad.psi, y, 1, y)


def llr_direct(mean, transform, psi, p, x, normalize_length=True):
    """The same scores from the projected Gaussian model with no diagonalisation: z = P (x - m) has within-class covariance
    W = P A^-1 A^-T P^T and between-class covariance B = P A^-1 diag(psi) A^-T P^T.  Length normalisation (what
    TransformIvector does with one utterance): q = z^T (B + W)^-1 z, z <- z sqrt(r / q).  Two rows of one speaker are jointly
    Gaussian with covariance [[B + W, B], [B, B + W]], of different speakers independent with covariance B + W each:
    LLR = log N([e; t]; joint) - log N(e) - log N(t)."""
    mean, transform, psi, p = (np.asarray(a, np.float64) for a in (mean, transform, psi, p))
    x = np.asarray(x, np.float64)
    r = p.shape[0]
    m = p @ np.linalg.inv(transform)
    w = m @ m.T
    b = (m * psi[None, :]) @ m.T
    tot = b + w
    z = (x - mean[None, :]) @ p.T
    tot_inv = np.linalg.inv(tot)
    if normalize_length:
        q = np.einsum("ni,ij,nj->n", z, tot_inv, z)
        z = z * np.where(q > 0.0, np.sqrt(r / np.where(q > 0.0, q, 1.0)), 0.0)[:, None]
    joint = np.block([[tot, b], [b, tot]])
    joint_inv = np.linalg.inv(joint)
    _, logdet_joint = np.linalg.slogdet(joint)
    _, logdet_tot = np.linalg.slogdet(tot)
    jaa, jab, jbb = joint_inv[:r, :r], joint_inv[:r, r:], joint_inv[r:, r:]
    qa = np.einsum("ni,ij,nj->n", z, jaa, z)
    qb = np.einsum("ni,ij,nj->n", z, jbb, z)
    qab = z @ jab @ z.T
    marg = np.einsum("ni,ij,nj->n", z, tot_inv, z)
    log_joint = -0.5 * (logdet_joint + qa[:, None] + 2.0 * qab + qb[None, :])
    log_marg = -0.5 * (logdet_tot + marg)
    return log_joint - log_marg[:, None] - log_marg[None, :]


# ---------------------------------------------------------------------------------------------------- shared test inputs
# One batch of recordings per D: sizes at the edges (no rows, one row, fewer rows than dimensions, one more than D, many).
CASES = collections.OrderedDict([(7, (0, 1, 2, 3, 5, 40)), (33, (20, 33, 34, 100)), (128, (90, 300)), (150, (120, 400)),
                                 (256, (300,)), (1, (4,))])
TARGET_ENERGIES = (0.1, 0.5, 0.9, 1.0)


def case(d, seed=3):
    """(mean, transform, psi, list of float32 recordings [n, D]) of the batch of dimension d: a ref_plda.random_model and,
    per recording, n rows of 3 speakers drawn from it (ref_plda.draw), shuffled and rounded to float32.  The seed is one whose
    spectra stay clear of every target energy and have a gap behind the kept directions (margins below: 2.1e-6 and 1.0e-4 at
    the least; a recording of D + 1 rows has a smallest eigenvalue of ~1e-6 of the trace, which target_energy = 1 has to tell
    from 0); tests/test_gpu_plda_adapt.py asserts both, so another seed that does not have them fails there."""
    import ref_plda
    rng = np.random.default_rng(1000 * seed + d)
    mean, transform, psi = ref_plda.random_model(rng, d)
    recs = []
    for n in CASES[d]:
        x, _ = ref_plda.draw(rng, mean, transform, psi, 3, (n + 2) // 3 if n else 1)
        recs.append(np.ascontiguousarray(x[rng.permutation(x.shape[0])[:n]], dtype=np.float32))
    return mean, transform, psi, recs


def margins(lam, target_energy):
    """How well the rule determines its own outcome on the descending spectrum `lam` -> (r, energy margin, gap margin).
    energy margin: the least distance of a cumulative energy fraction from target_energy (with target_energy = 1 the last
    fraction, which is 1 by construction, is left out); r is the same for every computation whose eigenvalues are accurate to
    well below it.  gap margin: (lam_{r-1} - lam_r) / lam_0, inf when r = D; the kept subspace is determined to about
    2^-53 / gap margin."""
    lam = np.asarray(lam, np.float64)
    d = lam.shape[0]
    r = energy_dim(lam, target_energy)
    frac = energy_fractions(lam)
    if target_energy >= 1.0:
        frac = frac[:-1]
    energy = float(np.min(np.abs(frac - target_energy))) if frac.size else np.inf
    gap = float((lam[r - 1] - lam[r]) / lam[0]) if r < d else np.inf
    return r, energy, gap
