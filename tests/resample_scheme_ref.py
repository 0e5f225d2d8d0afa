"""Restatement of the library's resampling schemes and ESS trigger (include/dpsx.h, "resampling schemes and the ESS
trigger") over tests/resample_ref.py -- Python integers from the weights q on, so ids and flags reproduce the kernels'
exactly from (q, u)."""
import numpy as np

import resample_ref as R

MULTINOMIAL, STRATIFIED, SYSTEMATIC = 0, 1, 2
SCHEMES = {"multinomial": MULTINOMIAL, "stratified": STRATIFIED, "systematic": SYSTEMATIC}
ONE_Q16 = 1 << 16


def ess_q16_of(tau):
    """tau in [0, 1] -> tau * 65536 rounded to nearest"""
    return int(float(tau) * 65536.0 + 0.5)


def _ints(q):
    return [int(v) for v in np.asarray(q).reshape(-1)]


def need(q, ess_q16):
    """the trigger: T^2 * 65536 < ess_q16 * K * S2"""
    q = _ints(q)
    t, s2 = sum(q), sum(v * v for v in q)
    return t * t * ONE_Q16 < int(ess_q16) * len(q) * s2


def ess(q):
    """the reported effective sample size: (double) T * (double) T / (double) S2 as fp32; 0 when S2 = 0"""
    q = _ints(q)
    t, s2 = sum(q), sum(v * v for v in q)
    return np.float32(float(t) * float(t) / float(s2)) if s2 else np.float32(0)


def min_trigger(q):
    """the smallest ess_q16 at which the segment resamples (may exceed 65536: then it never does)"""
    q = _ints(q)
    t, s2 = sum(q), sum(v * v for v in q)
    return None if s2 == 0 else (t * t * ONE_Q16) // (len(q) * s2) + 1


def targets(q, u, scheme):
    """target_j of every slot (Python integers)"""
    q = _ints(q)
    k, t = len(q), sum(q)
    ui = [int(v) for v in R.uniform_ints(u)]
    if scheme == MULTINOMIAL:
        return [(t * ui[j]) >> 24 for j in range(k)]
    return [((t * ((j << 24) + (ui[0] if scheme == SYSTEMATIC else ui[j]))) >> 24) // k for j in range(k)]


def draw(q, u, scheme, ess_q16=ONE_Q16):
    """local ids [K] of one segment: the identity unless the trigger fires, else the smallest i with cdf_i > target_j,
    clamped to K - 1"""
    qi = _ints(q)
    k = len(qi)
    if not need(qi, ess_q16):
        return np.arange(k, dtype=np.int64)
    cdf, acc = [], 0
    for v in qi:
        acc += v
        cdf.append(acc)
    out = np.empty(k, dtype=np.int64)
    for j, tg in enumerate(targets(qi, u, scheme)):
        lo, hi = 0, k - 1
        while lo < hi:
            mid = (lo + hi) >> 1
            if cdf[mid] > tg:
                hi = mid
            else:
                lo = mid + 1
        out[j] = lo
    return out


def draw_segments(q, u, segments, scheme, ess_q16=ONE_Q16):
    """(global ids [N], flags [segments] uint8, ess [segments] fp32) for q, u [N] split into equal segments"""
    q, u = np.asarray(q).reshape(segments, -1), np.asarray(u, dtype=np.float32).reshape(segments, -1)
    k = q.shape[1]
    ids = np.concatenate([m * k + draw(q[m], u[m], scheme, ess_q16) for m in range(segments)])
    flags = np.array([need(q[m], ess_q16) for m in range(segments)], dtype=np.uint8)
    return ids, flags, np.array([ess(q[m]) for m in range(segments)], dtype=np.float32)


def counts(ids_local, k):
    return np.bincount(np.asarray(ids_local), minlength=k)


def count_bounds(q, scheme):
    """(lower, upper) bounds on the number of slots that draw each particle, from L_i = floor(K q_i / T)"""
    qi = _ints(q)
    k, t = len(qi), sum(qi)
    L = np.array([k * v // t for v in qi], dtype=np.int64)
    if scheme == SYSTEMATIC:
        return L, L + 1
    return np.maximum(L - 1, 0), L + 2


# the mean-count check (unbiasedness): M identical segments of K = 8 particles, uniforms torch.manual_seed(0);
# torch.rand(M * K) on the CPU.  The bound is 6 sigma of the mean of M counts of variance at most v: a systematic n_i takes
# two adjacent values (v <= 1/4), a stratified one has at most two partially covered strata, independent (v <= 1/2).
MEAN_D = [0.0, 10.0, 20.0, 40.0, 80.0, 160.0, 320.0, float("nan")]
MEAN_M, MEAN_K = 1024, 8
MEAN_BOUND = {SYSTEMATIC: 6 * (0.25 / MEAN_M) ** 0.5, STRATIFIED: 6 * (0.5 / MEAN_M) ** 0.5}


def mean_count_error(ids, q, M, K):
    """max_i |mean_m n_i - K q_i / T| over M identical segments (global ids, q of the first segment)"""
    ids = np.asarray(ids)
    n = np.stack([counts(ids[m * K:(m + 1) * K] - m * K, K) for m in range(M)])
    q = np.asarray(q[:K], dtype=np.float64)
    return float(np.abs(n.mean(axis=0) - K * q / q.sum()).max())
