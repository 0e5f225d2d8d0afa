"""NumPy restatement of spherical-Gaussian guidance (include/dpsx.h "spherical-Gaussian guidance"; the expression in the
header of dps_ttc_amd/csrc/dsg.hip) -- the reference of tests/test_dsg_cpu.py and tests/test_dsg_gpu.py, independent of
the kernels.

From the float32 inputs: s = (-a / b) g_eps + g_unet in float32 with the kernel's two operations (smc_ref.update: numpy
does not fuse, so it has the kernel's bits) and the log-variance in float32 as post_logvar forms it (smc_ref.logvar);
everything after that -- sd, n = sd z, the four sums, alpha, beta, x_next -- is float64."""
import numpy as np

import smc_ref


def restate(sample, g_eps, g_unet, v, z, c, g):
    """particles [n, ...] -> dict:
         S, Nn, C, R        [n] the four sums;   mag: {name: [n]} the summed absolute values of each sum's terms
         alpha, beta, r     [n]
         n                  [n, ...] the noise term sd z K1 added
         D                  [n, ...] x_next - mean = alpha n - beta s  (= r m / ||m||; 0 where the particle keeps `sample`)
         x_next             [n, ...] sample + (alpha - 1) n - beta s;  `sample` itself where the step adds no noise, S is
                            not > 0 or mm is not > 0"""
    c = smc_ref.coefs_dict(c)
    sample = np.asarray(sample, dtype=np.float64)
    p = sample.shape[0]
    zero = np.zeros(p)
    if not int(c["add_noise"]) & 1:
        return {"S": zero, "Nn": zero, "C": zero, "R": zero, "mag": {k: zero for k in ("S", "Nn", "C", "R")},
                "alpha": np.ones(p), "beta": zero, "r": zero, "n": np.zeros_like(sample), "D": np.zeros_like(sample),
                "x_next": sample.copy()}
    s = smc_ref.update(g_eps, g_unet, c).astype(np.float64)
    sd = smc_ref.sd(v, c)
    n = sd * np.asarray(z, dtype=np.float64)
    tot = lambda a: a.reshape(p, -1).sum(axis=1)
    S, Nn, C, R = tot(s * s), tot(n * n), tot(s * n), tot(sd * sd)
    mag = {"S": S, "Nn": Nn, "C": tot(np.abs(s * n)), "R": R}
    g = np.float64(np.float32(g))
    r = np.sqrt(R)
    with np.errstate(divide="ignore", invalid="ignore"):
        mm = (1 - g) ** 2 * Nn + g ** 2 * R - 2 * g * (1 - g) * r * C / np.sqrt(S)
        ok = (S > 0) & (mm > 0)
        alpha = np.where(ok, r * (1 - g) / np.sqrt(mm), 1.0)
        beta = np.where(ok, r * r * g / (np.sqrt(mm) * np.sqrt(S)), 0.0)
    bc = lambda a: a.reshape((p,) + (1,) * (sample.ndim - 1))
    D = np.where(bc(ok), bc(alpha) * n - bc(beta) * s, 0.0)
    x_next = np.where(bc(ok), sample + (bc(alpha) - 1) * n - bc(beta) * s, sample)
    return {"S": S, "Nn": Nn, "C": C, "R": R, "mag": mag, "alpha": alpha, "beta": beta, "r": r, "n": n, "D": D,
            "x_next": x_next}
