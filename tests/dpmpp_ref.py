"""Restatement of the DPM-Solver++(2M) option of the ddim samplers (Lu et al. 2022), independent of the package:

* table(abar, eta): lambda, h, r and the multistep scalar c per loop index, float64; c32: c rounded to fp32 once
* logsnr_steps(betas, n): the "logsnr{n}" spacing
* update_f32: dpsx_step_update_ms_f32's expression in numpy float32, one rounding per operation (the comparison with the
  kernel is bit for bit)
* update_f64: the same in float64
* loop_f64: the whole sampler in float64 for a given eps function -- S1's DDIM record with the clamp, then the update
* GaussModel: the data model N(m, v) per element, its closed-form eps and its exact probability-flow solution
"""
import numpy as np


def lambdas(abar):
    abar = np.asarray(abar, dtype=np.float64)
    return 0.5 * np.log(abar / (1.0 - abar))


def table(abar, eta):
    """abar [n]: the kept steps' cumulative alphas, loop index order (the loop runs i = n - 1 .. 0 and the step from i lands
    on abar[i - 1]; from 0 on abar = 1) -> dict of float64 arrays lam [n], h [n] (h[0] = nan: lambda of the clean image is
    infinite), r [n] (nan where undefined), c [n] (0 at i = n - 1 and i = 0)"""
    if eta not in (0.0, 1.0):
        raise ValueError("the 2M coefficients are defined for eta = 0 and eta = 1")
    abar = np.asarray(abar, dtype=np.float64)
    n = len(abar)
    lam = lambdas(abar)
    h, r, c = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n)
    h[1:] = lam[:-1] - lam[1:]
    for i in range(1, n - 1):
        r[i] = h[i + 1] / h[i]
        gain = 1.0 - np.exp(-h[i]) if eta == 0.0 else 1.0 - np.exp(-2.0 * h[i])
        c[i] = np.sqrt(abar[i - 1]) * gain / (2.0 * r[i])
    return {"lam": lam, "h": h, "r": r, "c": c}


def c32(abar, eta):
    return table(abar, eta)["c"].astype(np.float32)


def logsnr_steps(betas, n):
    """sorted base indices of "logsnr{n}": n values uniform in lambda from the first to the last base timestep, each mapped
    to the nearest base lambda (tie: the lower index), plus both ends, duplicates dropped"""
    if n < 2:
        raise ValueError("n < 2")
    lam = lambdas(np.cumprod(1.0 - np.asarray(betas, dtype=np.float64)))
    kept = {0, len(lam) - 1}
    for j in range(n):
        v = lam[0] + (lam[-1] - lam[0]) * j / (n - 1)
        best = 0
        for t in range(1, len(lam)):
            if abs(lam[t] - v) < abs(lam[best] - v):          # strict: a tie keeps the lower index
                best = t
        kept.add(best)
    return sorted(kept)


def update_f32(sample, g_eps, g_unet, x0_cur, x0_prev, c, a, b):
    """x_next of dpsx_step_update_ms_f32, float32 arrays in, every operation one fp32 rounding; a, b: the record's"""
    f = np.float32
    ratio = (-f(a)) / f(b)
    s = (ratio * g_eps.astype(f)).astype(f) + (f(0.0) if g_unet is None else g_unet.astype(f))
    u = (sample.astype(f) - s).astype(f)
    if f(c) == 0:
        return u
    d = (x0_cur.astype(f) - x0_prev.astype(f)).astype(f)
    return (u + (f(c) * d).astype(f)).astype(f)


def update_f64(sample, g_eps, g_unet, x0_cur, x0_prev, c, a, b):
    d = np.float64
    ratio = d(np.float32(-np.float32(a) / np.float32(b)))
    s = ratio * g_eps.astype(d) + (0.0 if g_unet is None else g_unet.astype(d))
    u = sample.astype(d) - s
    if np.float32(c) == 0:
        return u
    return u + d(np.float32(c)) * (x0_cur.astype(d) - x0_prev.astype(d))


def ddim_record(abar, i, eta):
    """float64 (a, b, c1, c2, sigma) of the DDIM step at loop index i"""
    ab, abp = abar[i], (abar[i - 1] if i > 0 else 1.0)
    sigma = eta * np.sqrt((1.0 - abp) / (1.0 - ab)) * np.sqrt(1.0 - ab / abp)
    return (np.sqrt(1.0 / ab), np.sqrt(1.0 / ab - 1.0), np.sqrt(abp), np.sqrt(max(1.0 - abp - sigma ** 2, 0.0)), sigma)


def loop_f64(abar, eps_fn, x, order, eta=0.0, noise_fn=None, clamp=True, stop=0):
    """The sampler in float64 with no guidance: for i = n - 1 .. stop
        x0 = clamp(a x - b eps_fn(x, i)) ; eps' = (a x - x0) / b ; sample = c1 x0 + c2 eps' + sigma z   (z: i > 0 only)
        x  = sample + c_i (x0 - x0_prev)                                                              (order 2)
    -> x after the step at index `stop` (stop = 1: the state entering the last step)"""
    abar = np.asarray(abar, dtype=np.float64)
    n = len(abar)
    c = table(abar, eta)["c"] if order == 2 else np.zeros(n)
    x = np.asarray(x, dtype=np.float64)
    x0_prev = None
    for i in range(n - 1, stop - 1, -1):
        a, b, c1, c2, sigma = ddim_record(abar, i, eta)
        x0 = a * x - b * eps_fn(x, i)
        if clamp:
            x0 = np.clip(x0, -1.0, 1.0)
        eps = (a * x - x0) / b
        sample = c1 * x0 + c2 * eps
        if i > 0 and sigma > 0.0:
            sample = sample + sigma * noise_fn(i, x.shape)
        x = sample if c[i] == 0.0 else sample + c[i] * (x0 - x0_prev)
        x0_prev = x0
    return x


class GaussModel:
    """data ~ N(m, v) per element under abar [n]: x_i ~ N(sa m, sa^2 v + 1 - abar)"""

    def __init__(self, abar, m=0.2, v=0.04):
        self.abar, self.m, self.v = np.asarray(abar, dtype=np.float64), m, v

    def var(self, i):
        return self.abar[i] * self.v + 1.0 - self.abar[i]

    def eps(self, x, i):
        """E[eps | x_i = x]"""
        return np.sqrt(1.0 - self.abar[i]) * (x - np.sqrt(self.abar[i]) * self.m) / self.var(i)

    def draw(self, i, size, seed):
        return np.sqrt(self.abar[i]) * self.m + np.sqrt(self.var(i)) * np.random.RandomState(seed).randn(size)

    def flow(self, x, i, j):
        """the exact probability-flow solution: the state at index j of the trajectory through x at index i"""
        return np.sqrt(self.abar[j]) * self.m + np.sqrt(self.var(j) / self.var(i)) * (x - np.sqrt(self.abar[i]) * self.m)
