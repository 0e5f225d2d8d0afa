"""NumPy restatement of the CG data-consistency step (include/dpsx.h, dpsx_cg_step_f32) over the oracle's
Operator.forward / adjoint -- the reference the device step is compared with.  Vectors in `dtype`, sums and scalars in
float64, the same guards.  The oracle's operators take and return fp32, so each application rounds its input once."""
import numpy as np


def sumsq(v):
    """one float64 sum of squares per particle"""
    return (np.asarray(v, dtype=np.float64).reshape(v.shape[0], -1) ** 2).sum(axis=1)


def _col(s, dtype):
    return np.asarray(s, dtype=dtype).reshape(-1, 1, 1, 1)


def rows(y, n):
    """y [y_n, ...] with y_n dividing n -> [n, ...]: particle p reads row p // (n // y_n)"""
    return np.repeat(np.asarray(y), n // y.shape[0], axis=0)


def solve(op, x0_hat, y, rho, iters, dtype=np.float64):
    """-> (d [N, C, H, W], dist [N] = ||y - A x0_hat||_2) after `iters` CG iterations on (A^T A + rho I) from d = 0"""
    x0 = np.asarray(x0_hat, dtype=dtype)
    hw = x0.shape[-2:]
    A = lambda v: op.forward(v.astype(np.float32)).astype(dtype)
    At = lambda u: op.adjoint(u.astype(np.float32), hw).astype(dtype)
    r_y = rows(y, x0.shape[0]).astype(dtype) - A(x0)
    dist = np.sqrt(sumsq(r_y))
    r = At(r_y)
    p, rs, d = r.copy(), sumsq(r), np.zeros_like(x0)
    with np.errstate(all="ignore"):
        for _ in range(iters):
            t = A(p)
            s = At(t)
            pq = sumsq(t) + float(rho) * sumsq(p)
            alpha = np.where(pq > 0, rs / pq, 0.0)
            d = d + _col(alpha, dtype) * p
            r = r - _col(alpha, dtype) * (s + dtype(rho) * p)
            rs_new = sumsq(r)
            beta = np.where(rs > 0, rs_new / rs, 0.0)
            rs = rs_new
            p = r + _col(beta, dtype) * p
    return d, dist


def objective(op, x0_hat, y, d, rho):
    """J = ||y - A (x0_hat + d)||^2 + rho ||d||^2 per particle, float64"""
    x = np.asarray(x0_hat, dtype=np.float64) + np.asarray(d, dtype=np.float64)
    ax = op.forward(x.astype(np.float32)).astype(np.float64)
    return sumsq(rows(y, x.shape[0]).astype(np.float64) - ax) + float(rho) * sumsq(d)


def kappa(c):
    """the slope of the sampler's `sample` in x0_hat from an oracle.tables record (fp32, in this order)"""
    c1, c2, b = np.float32(c["c1"]), np.float32(c["c2"]), np.float32(c["b"])
    return np.float32(c1 - c2 / b) if int(c["add_noise"]) & 2 else c1
