"""The rule of xv_bn_batch_forward / xv_bn_batch_backward (include/xvec_hip.h) in float64 numpy: batch norm in training mode on a
stored product z [n, N], the moving-average update (in float64 and as the float32 replay of its three operations), and the
per-element error bound derived in the header of csrc/bn_batch.hip restated as bounds().

The rule is checked against torch.autograd in float64 (tests/test_bn_batch_host.py)."""
import numpy as np

U = 2.0 ** -24
EPS = 1e-3
NONE, RELU, LRELU = 0, 1, 2
F = np.float32
SLOPE = float(F(0.2))                      # the kernel multiplies by float32(0.2)


def decay(momentum):
    """d = float(1.0 - double(momentum)) as a float64 value."""
    return float(F(1.0 - float(momentum)))


def bessel_factor(n):
    """f = float(double(n) / double(max(n - 1, 1))) as a float64 value."""
    return float(F(float(n) / float(max(n - 1, 1))))


def forward(z, gamma, beta, act=NONE, slope=SLOPE):
    """z [n, N], gamma, beta [N] -> dict(z, gamma, beta, act, mu, v, r, s, h, y), float64."""
    z, gamma, beta = (np.asarray(v, dtype=np.float64) for v in (z, gamma, beta))
    mu = z.mean(axis=0)
    v = ((z - mu[None, :]) ** 2).mean(axis=0)
    r = 1.0 / np.sqrt(v + EPS)
    s = gamma * r
    h = s[None, :] * (z - mu[None, :]) + beta[None, :]
    y = h if act == NONE else np.where(h > 0, h, 0.0 if act == RELU else slope * h)
    return dict(z=z, gamma=gamma, beta=beta, act=act, slope=slope, mu=mu, v=v, r=r, s=s, h=h, y=y)


def backward(fwd, gy):
    """-> dict(a, xh, A, G, p, gz [n, N], ggamma, gbeta [N]), float64."""
    gy = np.asarray(gy, dtype=np.float64)
    act, h, z = fwd["act"], fwd["h"], fwd["z"]
    n = z.shape[0]
    if act == NONE:
        a = gy.copy()
    else:
        a = gy * np.where(h > 0, 1.0, 0.0 if act == RELU else fwd["slope"])     # zero belongs to the lower branch
    xh = fwd["r"][None, :] * (z - fwd["mu"][None, :])
    A = a.sum(axis=0)
    G = (a * xh).sum(axis=0)
    p = a - A[None, :] / n - xh * (G[None, :] / n)
    return dict(gy=gy, a=a, xh=xh, A=A, G=G, p=p, gz=fwd["s"][None, :] * p, ggamma=G, gbeta=A)


def moving(mm, mv, mu, v, n, momentum, bessel):
    """The update in float64 with the kernel's float32 d and f -> (moving_mean', moving_variance', v')."""
    mm, mv, mu, v = (np.asarray(x, dtype=np.float64) for x in (mm, mv, mu, v))
    d = decay(momentum)
    vb = v * bessel_factor(n) if bessel else v
    return mm - (mm - mu) * d, mv - (mv - vb) * d, vb


def moving_f32(mm, mv, mu, v, n, momentum, bessel):
    """The three operations of the update replayed in float32 from float32 mu and v: the bits the kernel writes."""
    mm, mv, mu, v = (np.asarray(x, dtype=F) for x in (mm, mv, mu, v))
    d = F(1.0 - float(momentum))
    f = F(float(n) / float(max(n - 1, 1)))
    vb = (v * f).astype(F) if bessel else v
    return (mm - ((mm - mu).astype(F) * d).astype(F)).astype(F), (mv - ((mv - vb).astype(F) * d).astype(F)).astype(F)


def bounds(fwd, bwd=None, bz=None, mm=None, mv=None, momentum=0.99, bessel=False):
    """The header of csrc/bn_batch.hip -> dict of per-element bounds: mu, v, r, s, h, y; with mm and mv moving_mean and
    moving_variance; with `bwd` gbeta, ggamma, gz.  bz [n, N] is the caller's bound of z (None: the oracle has the device's z)."""
    z, gamma, mu, v, r, s, h = (fwd[k] for k in ("z", "gamma", "mu", "v", "r", "s", "h"))
    n = z.shape[0]
    t = 2.0 ** -53 * (n + 64)
    bz = np.zeros_like(z) if bz is None else np.asarray(bz, dtype=np.float64)
    dev = np.abs(z - mu[None, :])
    bmu = bz.mean(axis=0) + t * np.abs(z).mean(axis=0) + U * np.abs(mu)
    q = (2.0 * dev * bz + (bz + bmu[None, :]) ** 2).mean(axis=0)
    bv = q + (U + t) * (v + q)
    br = 0.5 * (np.maximum(v - bv, 0.0) + EPS) ** -1.5 * bv + 1.01 * U * r
    bs = np.abs(gamma) * br + U * (np.abs(s) + np.abs(gamma) * br)
    bd = bz + bmu[None, :] + U * (dev + bz + bmu[None, :])
    e = np.abs(s)[None, :] * bd + bs[None, :] * (dev + bd)
    bh = e + U * (np.abs(h) + e)
    out = dict(mu=bmu, v=bv, r=br, s=bs, h=bh, y=bh + 2.0 * U * np.abs(fwd["y"]))
    if mm is not None:
        d = decay(momentum)
        mm1, mv1, vb = moving(mm, mv, mu, v, n, momentum, bessel)
        bvb = bessel_factor(n) * bv + 1.01 * U * vb if bessel else bv
        out["moving_mean"] = 1.01 * d * bmu + 2.01 * U * d * np.abs(np.asarray(mm, dtype=np.float64) - mu) + U * np.abs(mm1)
        out["moving_variance"] = 1.01 * d * bvb + 2.01 * U * d * np.abs(np.asarray(mv, dtype=np.float64) - vb) + U * np.abs(mv1)
    if bwd is None:
        return out
    a, xh, A, G, p = np.abs(bwd["a"]), np.abs(bwd["xh"]), np.abs(bwd["A"]), np.abs(bwd["G"]), np.abs(bwd["p"])
    ba = 2.0 * U * a if fwd["act"] == LRELU else np.zeros_like(a)
    bx = br[None, :] * (dev + bz + bmu[None, :]) + r[None, :] * (bz + bmu[None, :])
    bA = ba.sum(axis=0) + t * a.sum(axis=0)
    bG = (ba * (xh + bx) + a * bx).sum(axis=0) + 1.01 * t * (a * (xh + bx)).sum(axis=0)
    out["gbeta"] = bA + U * A
    out["ggamma"] = bG + U * G
    bp = (ba + bA[None, :] / n + (bx * (G + bG)[None, :] + xh * bG[None, :]) / n
          + t * (a + A[None, :] / n + xh * G[None, :] / n))
    eg = np.abs(s)[None, :] * bp + bs[None, :] * (p + bp)
    out["gz"] = eg + U * (np.abs(bwd["gz"]) + eg)
    return out
