"""NumPy restatement of the library's counter-based normals (include/dpsx.h, "counter-based normals") -- the reference the
device fill and the in-kernel draws are compared with.  Philox4x32-10 in uint64 arithmetic (its words reproduce the
device's exactly); the uniforms and Box-Muller in float64 (the device evaluates them in fp32 on the transcendental unit)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
TAG_STEP, TAG_X_START = 0, 1


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two -> the four output words as uint64 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def counters(seed, step, tag, particle, units):
    """-> (counter words (c0, c1, c2, c3), key (k0, k1)) of the first `units` float4 units of one particle"""
    seed = int(seed)
    key = (seed & MASK, (seed >> 32) & MASK)
    return (np.arange(units, dtype=np.uint64), int(particle), int(step), int(tag)), key


def particle_ids(n, particle_base=0, per_image=0):
    p = np.arange(n, dtype=np.int64)
    ids = int(particle_base) + (p % per_image if per_image > 0 else p)
    assert ids.max(initial=0) <= MASK, "the particle id must fit 32 bits"
    return ids


def bits(n, chw, seed, step, tag=0, particle_base=0, per_image=0):
    """the Philox words of every unit: uint32 [n, 4 * ceil(chw / 4)]"""
    units = (chw + 3) // 4
    out = np.empty((n, units, 4), dtype=np.uint32)
    for p, pid in enumerate(particle_ids(n, particle_base, per_image)):
        ctr, key = counters(seed, step, tag, pid, units)
        out[p] = np.stack(philox4x32_10(ctr, key), axis=-1).astype(np.uint32)
    return out.reshape(n, 4 * units)


def normals_from_bits(words, chw):
    """float64 [n, chw] from the words [n, 4 * units]: (r0, r1) -> elements 0, 1 of the unit, (r2, r3) -> 2, 3"""
    w = np.asarray(words).astype(np.uint64).reshape(words.shape[0], -1, 2, 2)
    u1 = ((w[..., 0] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24      # (0, 1]
    u2 = (w[..., 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24              # [0, 1)
    rad = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)], axis=-1)
    return z.reshape(words.shape[0], -1)[:, :chw]


def randn(n, chw, seed, step, tag=0, particle_base=0, per_image=0):
    return normals_from_bits(bits(n, chw, seed, step, tag, particle_base, per_image), chw)
