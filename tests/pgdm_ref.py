"""NumPy float64 restatement of pseudoinverse guidance on the CG solve (include/dpsx.h, dpsx_cg_pullback_f32) -- the
reference of the `pgdm` suites.  Four parts:

* the step's records and host scalars from a beta schedule (records, scalars);
* dense linear algebra for the push-through identity (dense_matrix, pinv_form, normal_form, cg_dense);
* the launch's output from tests/cg_ref.py's solve over the oracle's operators (pullback);
* the analytic model: a Gaussian prior, whose denoiser, Jacobian and exact posterior are closed forms (analytic_error).
"""
import numpy as np

import cg_ref


# ------------------------------------------------------------------ records and host scalars
def tables(betas):
    """float64 tables of a (possibly respaced) schedule -> dict of abar, abar_prev, a, b"""
    betas = np.asarray(betas, dtype=np.float64)
    abar = np.cumprod(1.0 - betas)
    return dict(betas=betas, abar=abar, abar_prev=np.append(1.0, abar[:-1]), a=np.sqrt(1.0 / abar),
                b=np.sqrt(1.0 / abar - 1.0))


def record(tb, idx, eta=None):
    """the step's record in float64 -> dict(a, b, c1, c2, ddim).  eta=None: the DDPM record (the posterior mean's
    coefficients); else the DDIM record with that eta (c1 = sqrt(abar_prev), c2 = sqrt(1 - abar_prev - sigma^2))"""
    abar, abar_prev, beta = tb["abar"][idx], tb["abar_prev"][idx], tb["betas"][idx]
    if eta is None:
        c1 = beta * np.sqrt(abar_prev) / (1.0 - abar)
        c2 = (1.0 - abar_prev) * np.sqrt(1.0 - beta) / (1.0 - abar)
        return dict(a=tb["a"][idx], b=tb["b"][idx], c1=c1, c2=c2, ddim=False)
    sigma = float(eta) * np.sqrt((1.0 - abar_prev) / (1.0 - abar)) * np.sqrt(1.0 - abar / abar_prev)
    return dict(a=tb["a"][idx], b=tb["b"][idx], c1=np.sqrt(abar_prev), c2=np.sqrt(max(1.0 - abar_prev - sigma ** 2, 0.0)),
                ddim=True)


def kappa(rec):
    """the slope of the sampler's `sample` in x0_hat: c1 (DDPM), c1 - c2 / b (DDIM: eps is re-derived from x0_hat)"""
    return rec["c1"] - rec["c2"] / rec["b"] if rec["ddim"] else rec["c1"]


def weight_of(tb, idx, rec, weighting):
    """w_t: "score" = kappa a; "paper" = sqrt(abar_prev) / a"""
    if weighting == "score":
        return kappa(rec) * rec["a"]
    if weighting == "paper":
        return np.sqrt(tb["abar_prev"][idx]) / rec["a"]
    raise ValueError(weighting)


def scalars(tb, idx, rec, sigma_y, weighting="score", weight=1.0):
    """(rho_t, gain_t) in float64: rho_t = sigma_y^2 / (1 - abar_t), gain_t = weight w_t b"""
    return float(sigma_y) ** 2 / (1.0 - tb["abar"][idx]), float(weight) * weight_of(tb, idx, rec, weighting) * rec["b"]


# ------------------------------------------------------------------ the push-through identity, dense
def dense_matrix(op, shape):
    """A as a dense float64 matrix [m, e] from an oracle operator's forward on the unit vectors of `shape` (c, h, w)"""
    e = int(np.prod(shape))
    cols = op.forward(np.eye(e, dtype=np.float32).reshape((e,) + tuple(shape)))
    return cols.reshape(e, -1).T.astype(np.float64)


def pinv_form(A, r, r2, sigma_y):
    """r_t^2 A^T (r_t^2 A A^T + sigma_y^2 I)^-1 r"""
    m = A.shape[0]
    return r2 * A.T @ np.linalg.solve(r2 * (A @ A.T) + sigma_y ** 2 * np.eye(m), r)


def normal_form(A, r, rho):
    """(A^T A + rho I)^-1 A^T r"""
    e = A.shape[1]
    return np.linalg.solve(A.T @ A + rho * np.eye(e), A.T @ r)


def cg_dense(A, r, rho, iters):
    """dpsx_cg_step_f32's recurrence on (A^T A + rho I) d = A^T r from d = 0, one vector, float64, the same guards"""
    g = A.T @ r
    d, p, rs = np.zeros_like(g), g.copy(), float(g @ g)
    for _ in range(iters):
        t = A @ p
        pq = float(t @ t) + rho * float(p @ p)
        alpha = rs / pq if pq > 0 else 0.0
        d = d + alpha * p
        g = g - alpha * (A.T @ t + rho * p)
        rs_new = float(g @ g)
        beta = rs_new / rs if rs > 0 else 0.0
        rs = rs_new
        p = g + beta * p
    return d


# ------------------------------------------------------------------ the launch
def solve_at(op, x0_hat, y, rho, counts):
    """cg_ref.solve's recurrence (float64 vectors, the same guards), run once to max(counts) iterations
    -> ({k: d after k iterations for k in counts}, dist [N])"""
    x0 = np.asarray(x0_hat, dtype=np.float64)
    hw, col = x0.shape[-2:], lambda s: np.asarray(s, dtype=np.float64).reshape(-1, 1, 1, 1)
    A = lambda v: op.forward(v.astype(np.float32)).astype(np.float64)
    At = lambda u: op.adjoint(u.astype(np.float32), hw).astype(np.float64)
    r_y = cg_ref.rows(y, x0.shape[0]).astype(np.float64) - A(x0)
    dist = np.sqrt(cg_ref.sumsq(r_y))
    r = At(r_y)
    p, rs, d = r.copy(), cg_ref.sumsq(r), np.zeros_like(x0)
    out = {0: d.copy()}
    with np.errstate(all="ignore"):
        for k in range(1, max(counts) + 1):
            t = A(p)
            s = At(t)
            pq = cg_ref.sumsq(t) + float(rho) * cg_ref.sumsq(p)
            alpha = np.where(pq > 0, rs / pq, 0.0)
            d = d + col(alpha) * p
            r = r - col(alpha) * (s + float(rho) * p)
            rs_new = cg_ref.sumsq(r)
            beta = np.where(rs > 0, rs_new / rs, 0.0)
            rs = rs_new
            p = r + col(beta) * p
            out[k] = d.copy()
    return {k: out[k] for k in counts}, dist


def pullback(op, x0_hat, y, inside, rho, iters, gain):
    """-> (g_eps [N, C, H, W] = inside ? gain d : 0, d, dist [N]) in float64 over the oracle operator `op`"""
    d, dist = cg_ref.solve(op, x0_hat, y, rho, iters)
    return np.where(np.asarray(inside) != 0, float(gain) * d, 0.0), d, dist


# ------------------------------------------------------------------ the analytic model
def uniform_steps(n, T=1000):
    """n base timesteps of T, uniformly spaced, the first and the last included"""
    return np.unique(np.round(np.linspace(0, T - 1, n)).astype(np.int64))


def analytic_error(n, weighting="score", elems=4096, mu0=0.2, sigma_y=0.5, T=1000, seed=0, weight=1.0):
    """DDIM (eta = 0) with the pgdm step on the model whose every quantity is a closed form: prior N(mu0, 1) per element,
    A = I, y = x* + sigma_y noise.  The marginal of x_t is N(sqrt(abar_t) mu0, 1), so
        eps(x_t) = sqrt(1 - abar_t) (x_t - sqrt(abar_t) mu0) ,  x0_hat = a x_t - b eps ,  J = a - b sqrt(1 - abar_t)
    (no clamp: the gate is 1), and d = (y - x0_hat) / (1 + rho_t).  The loop starts from the exact marginal
    x_T = sqrt(abar_T) mu0 + z and steps x_next = sqrt(abar_s) x0_hat + sqrt(1 - abar_s) eps + weight w_t J d.
    -> (RMS of x_final - (mu_post(y) + s_post z), RMS of x_final - y): the probability-flow map of the exact posterior
    N(mu_post, s_post^2), mu_post = (mu0 sigma_y^2 + y) / (1 + sigma_y^2), s_post^2 = sigma_y^2 / (1 + sigma_y^2)."""
    rng = np.random.RandomState(seed)
    x_star = mu0 + rng.randn(elems)
    y = x_star + sigma_y * rng.randn(elems)
    z = rng.randn(elems)
    base_abar = np.cumprod(1.0 - np.linspace(1e-4, 0.02, T, dtype=np.float64))
    kept = uniform_steps(n, T)
    abar_kept = base_abar[kept]
    tb = tables(1.0 - abar_kept / np.append(1.0, abar_kept[:-1]))
    x = np.sqrt(tb["abar"][-1]) * mu0 + z
    for idx in range(len(kept) - 1, -1, -1):
        abar, abar_prev = tb["abar"][idx], tb["abar_prev"][idx]
        rec = record(tb, idx, eta=0.0)
        eps = np.sqrt(1.0 - abar) * (x - np.sqrt(abar) * mu0)
        x0_hat = rec["a"] * x - rec["b"] * eps
        jac = rec["a"] - rec["b"] * np.sqrt(1.0 - abar)
        rho, _ = scalars(tb, idx, rec, sigma_y, weighting, weight)
        d = (y - x0_hat) / (1.0 + rho)
        sample = rec["c1"] * x0_hat + rec["c2"] * eps
        x = sample + weight * weight_of(tb, idx, rec, weighting) * jac * d
    post = (mu0 * sigma_y ** 2 + y) / (1.0 + sigma_y ** 2) + np.sqrt(sigma_y ** 2 / (1.0 + sigma_y ** 2)) * z
    rms = lambda v: float(np.sqrt(np.mean(v ** 2)))
    return rms(x - post), rms(x - y)
