"""NumPy restatement of the particle weights (include/dpsx.h, "particle weights") -- the reference of tests/test_smc_cpu.py
and tests/test_smc_gpu.py, independent of the kernels.

The update s = (-a / b) g_eps + g_unet is formed in float32 with the kernel's two operations (numpy does not fuse, so it has
the kernel's bits) and the log-variance in float32 as post_logvar does; sd, q = s / sd, the terms q (z - q / 2) and their
sum are float64.  S = sum |q| (|z| + |q| / 2) is the scale the kernel's rounding errors are measured against.  The
recurrence is restated in float64 with the one final rounding to float32."""
import numpy as np

F = np.float32


def coefs_dict(ck):
    """a kernels.Coefs record (or a dict with its fields) as a dict of Python numbers"""
    if isinstance(ck, dict):
        return ck
    return {k: getattr(ck, k) for k in ("a", "b", "c1", "c2", "min_log", "max_log", "add_noise")}


def update(g_eps, g_unet, c):
    """s of K3 in float32: ratio = -a / b (float32), one product, one sum"""
    c = coefs_dict(c)
    ratio = F(-F(c["a"])) / F(c["b"])
    s = F(ratio) * np.asarray(g_eps, dtype=F)
    return (s + (np.asarray(g_unet, dtype=F) if g_unet is not None else F(0.0))).astype(F)


def logvar(v, c):
    """post_logvar in float32: frac = (v + 1) / 2; frac max_log + (1 - frac) min_log"""
    c = coefs_dict(c)
    frac = (np.asarray(v, dtype=F) + F(1.0)) * F(0.5)
    return (frac * F(c["max_log"]) + (F(1.0) - frac) * F(c["min_log"])).astype(F)


def sd(v, c):
    """the per-element standard deviation of the step's noise term, float64: exp(logvar / 2); a DDIM record: sigma"""
    c = coefs_dict(c)
    if int(c["add_noise"]) & 2:
        return np.full(np.shape(v), np.float64(F(c["min_log"])))
    return np.exp(0.5 * logvar(v, c).astype(np.float64))


def correction(g_eps, g_unet, v, z, c):
    """-> (corr [n], S [n]) of particles [n, ...]: corr = sum q (z - q / 2), S = sum |q| (|z| + |q| / 2), q = s / sd;
    both 0 on a step that adds no noise"""
    c = coefs_dict(c)
    n = np.shape(g_eps)[0]
    if not int(c["add_noise"]) & 1:
        return np.zeros(n), np.zeros(n)
    q = update(g_eps, g_unet, c).astype(np.float64) / sd(v, c)
    z = np.asarray(z, dtype=np.float64)
    corr = (q * (z - 0.5 * q)).reshape(n, -1).sum(axis=1)
    scale = (np.abs(q) * (np.abs(z) + 0.5 * np.abs(q))).reshape(n, -1).sum(axis=1)
    return corr, scale


def density_difference(x_next, mean_u, s, sd_):
    """log N(x_next; mean_u, sd^2) - log N(x_next; mean_u - s, sd^2) per particle, float64 (the normalisers cancel)"""
    x, m, s, d = (np.asarray(a, dtype=np.float64) for a in (x_next, mean_u, s, sd_))
    n = x.shape[0]
    return (-(x - m) ** 2 / (2 * d ** 2) + (x - m + s) ** 2 / (2 * d ** 2)).reshape(n, -1).sum(axis=1)


def accum(E, d_prev, d_cur, partials, reset, segments, twist_scale, power, proposal_weight):
    """one dpsx_smc_accum_f32 call -> (E' float32 [n], d_prev' float32 [n], magnitude float64 [n]).  partials [n, slots]
    float32 or None; reset [segments] or None.  magnitude = the summed absolute values of the terms of E'."""
    E, d_prev, d_cur = (np.asarray(a, dtype=F) for a in (E, d_prev, d_cur))
    n = E.shape[0]
    seg = np.arange(n) // (n // int(segments))
    base = E.astype(np.float64)
    if reset is not None:
        base = np.where(np.asarray(reset)[seg] != 0, 0.0, base)
    dc, dp = d_cur.astype(np.float64), d_prev.astype(np.float64)
    ts, pw = np.float64(F(twist_scale)), np.float64(F(proposal_weight))
    a, b = (dc * dc, dp * dp) if int(power) == 2 else (dc, dp)
    out = base + ts * (a - b)
    mag = np.abs(base) + np.abs(ts * a) + np.abs(ts * b)
    if partials is not None:
        corr = np.asarray(partials, dtype=F).astype(np.float64).reshape(n, -1).sum(axis=1)
        out = out - pw * corr
        mag = mag + np.abs(pw * corr)
    return out.astype(F), d_cur.copy(), mag
