"""Blur kernels that are degenerate on purpose, shared by the host check of the tap tables (test_blur_tables_cpu.py) and
the device tests (test_blur_kernels_gpu.py): the named families F1-F7, each member chosen for the route it takes through
csrc/blur.hip, and a seeded fuzz set for the host check alone.  numpy only; everything is float32 and deterministic."""
import numpy as np

AUTO, FORCE_TAPS = 0, 1          # include/dpsx.h: DPSX_BLUR_AUTO, DPSX_BLUR_FORCE_TAPS
FUZZ_SIZES = (1, 3, 5, 7, 9, 31, 61, 65)
FUZZ_PER_SIZE = 200


def reach_of(k):
    """largest |offset| from the centre of a non-zero tap"""
    r = k.shape[0] // 2
    i, j = np.nonzero(k)
    return int(max(np.abs(i - r).max(), np.abs(j - r).max())) if i.size else 0


def radius4_of(k):
    """the halo the separable kernels stage: the reach rounded up to a multiple of 4, at least 4"""
    return max(4, (reach_of(k) + 3) // 4 * 4)


def image_shapes(k):
    """the smallest shapes that differ in route: the smallest image the reflection pad admits, one no larger than the
    staged halo, one whole tile, two tiles per axis, a tile plus slivers on the 16-byte path, the scalar loaders with
    folds from both borders"""
    r, r4 = k.shape[0] // 2, radius4_of(k)
    return [(r + 1, r + 1), (r4, r4 + 4), (64, 64), (128, 128), (66, 68), (50, 46)]


def admits(k, hw):
    """ReflectionPad2d(ks // 2) needs pad < side: what the library's geometry check accepts"""
    return hw[0] > k.shape[0] // 2 and hw[1] > k.shape[0] // 2


def pedestal_kernel():
    """the shipped 61 x 61 sigma = 3 Gaussian on a uniform pedestal of 0.9e-6 * peak: every element of (col x row - K)
    is below 1e-6 * peak, the L1 distance is 4.6e-5 of the kernel's mass"""
    from oracle.tables import gaussian_kernel2d
    g = gaussian_kernel2d(61, 3.0)
    return (g + 0.9e-6 * g.max()).astype(np.float32)


def _single(ks, i, j):
    k = np.zeros((ks, ks), dtype=np.float32)
    k[i, j] = 1.0
    return k


def named_families():
    """-> list of (family, name, kernel [ks, ks] float32, rank1): rank1 says that the kernel is an exact outer product,
    so DPSX_BLUR_AUTO must classify it separable and FORCE_TAPS is a second, different route; every other member
    must come back as a tap list in either mode"""
    out = []
    rng = np.random.RandomState(20240611)
    pos = lambda n: (0.25 + rng.rand(n)).astype(np.float32)          # random positive weights, none near zero

    # F1 single taps of weight 1
    out.append(("F1", "ks1", _single(1, 0, 0), True))
    for ks in (3, 61, 65):
        r, e = ks // 2, ks - 1
        for tag, (i, j) in {"centre": (r, r), "tl": (0, 0), "tr": (0, e), "bl": (e, 0), "br": (e, e),
                            "top": (0, r), "bottom": (e, r), "left": (r, 0), "right": (r, e)}.items():
            out.append(("F1", f"ks{ks}.{tag}", _single(ks, i, j), True))
    # F2 lines with random positive weights
    for ks in (5, 61):
        r, e = ks // 2, ks - 1
        for tag, row in (("row.centre", r), ("row.first", 0), ("row.last", e)):
            k = np.zeros((ks, ks), dtype=np.float32)
            k[row, :] = pos(ks)
            out.append(("F2", f"ks{ks}.{tag}", k, True))
        for tag, col in (("col.centre", r), ("col.first", 0), ("col.last", e)):
            k = np.zeros((ks, ks), dtype=np.float32)
            k[:, col] = pos(ks)
            out.append(("F2", f"ks{ks}.{tag}", k, True))
    # F3 diagonals: runs of two taps only (one tap and a padding zero), both parities of dx
    for ks in (5, 61):
        d = np.arange(ks)
        for tag, cols in (("diag", d), ("antidiag", ks - 1 - d)):
            k = np.zeros((ks, ks), dtype=np.float32)
            k[d, cols] = pos(ks)
            out.append(("F3", f"ks{ks}.{tag}", k, False))
    # F4 column segments of 4 and 8 rows on one parity of dx only: whole run classes stay empty
    for par in (0, 1):
        for seg in (4, 8):
            ks, r = 31, 15
            k = np.zeros((ks, ks), dtype=np.float32)
            for n, dx in enumerate(range(-12 + par, 13, 6)):          # even: -12 .. 12, odd: -11 .. 7
                top = 2 + 4 * n
                k[top:top + seg, r + dx] = pos(seg)
            out.append(("F4", f"ks31.{'odd' if par else 'even'}.seg{seg}", k, False))
    # F5 columns whose taps occupy the last / first 1, 2, 3 and 5 kernel rows: the run windows that must be shifted up
    for where in ("last", "first"):
        for rows in (1, 2, 3, 5):
            ks, r = 9, 4
            k = np.zeros((ks, ks), dtype=np.float32)
            for dx in (-3, 0, 2):
                if where == "last":
                    k[ks - rows:, r + dx] = pos(rows)
                else:
                    k[:rows, r + dx] = pos(rows)
            out.append(("F5", f"ks9.{where}{rows}", k, rows == 1))       # one row of taps is an outer product
    # F6 dense signed kernels
    for ks in (3, 5, 9):
        k = rng.randn(ks, ks).astype(np.float32)
        out.append(("F6", f"ks{ks}.dense_signed", k, False))
    # F7 the pedestal kernel: inside the element-wise rank-1 test, outside the operator bound
    out.append(("F7", "ks61.pedestal", pedestal_kernel(), False))
    return out


def asymmetric_rank1_kernels():
    """the asymmetric rank-1 products of test_hip_parity.py's test_blur_other_radii and test_blur_regular_non_square:
    both assert the separable kind"""
    from oracle.tables import gaussian_kernel2d
    out = []
    for ks, sigma in ((9, 1.0), (31, 0.5), (61, 5.0), (61, 7.5), (65, 8.0)):
        k = gaussian_kernel2d(ks, sigma)
        k = k * (1.0 + 0.3 * np.linspace(-1, 1, ks))[None, :] * (1.0 - 0.2 * np.linspace(-1, 1, ks))[:, None]
        out.append((f"other_radii.ks{ks}.s{sigma}", k.astype(np.float32)))
    for ks, sigma in ((9, 1.0), (25, 2.0), (61, 3.0), (61, 7.5)):
        k = gaussian_kernel2d(ks, sigma) * (1.0 + 0.3 * np.linspace(-1, 1, ks))[None, :]
        out.append((f"non_square.ks{ks}.s{sigma}", k.astype(np.float32)))
    return out


def fuzz_kernels(seed=7):
    """FUZZ_PER_SIZE kernels per size of FUZZ_SIZES: signed weights at densities from 2 % to 100 %, and in rotation
    taps forced into the four corners, single taps, full single columns, full single rows, sparse outer products
    (the separable branch) and the all-zero kernel"""
    rng = np.random.RandomState(seed)
    out = []
    for ks in FUZZ_SIZES:
        for n in range(FUZZ_PER_SIZE):
            kind = n % 8
            k = np.zeros((ks, ks), dtype=np.float32)
            density = 0.02 * (50.0 ** rng.rand())                    # log-uniform in [0.02, 1]
            if kind in (0, 1, 2):
                k = (rng.randn(ks, ks) * (rng.rand(ks, ks) < density)).astype(np.float32)
                if n % 16 == 0:
                    k = rng.randn(ks, ks).astype(np.float32)          # fully dense
            elif kind == 3:
                k = (rng.randn(ks, ks) * (rng.rand(ks, ks) < density)).astype(np.float32)
                for i, j in ((0, 0), (0, ks - 1), (ks - 1, 0), (ks - 1, ks - 1)):
                    if rng.rand() < 0.7:
                        k[i, j] = rng.randn()
            elif kind == 4:
                k[rng.randint(ks), rng.randint(ks)] = rng.randn()
            elif kind == 5:
                k[:, rng.randint(ks)] = rng.randn(ks)
            elif kind == 6:
                k[rng.randint(ks), :] = rng.randn(ks)
            elif n % 64 != 7:
                u = rng.randn(ks) * (rng.rand(ks) < max(density, 0.3))
                v = rng.randn(ks) * (rng.rand(ks) < max(density, 0.3))
                k = np.outer(u.astype(np.float32), v.astype(np.float32)).astype(np.float32)
            out.append(k)
    return out


def write_records(path, records):
    """records: iterable of (kernel, mode) -> the checker's input file: int32 ks, int32 mode, ks * ks float32 each"""
    with open(path, "wb") as f:
        for k, mode in records:
            k = np.ascontiguousarray(k, dtype=np.float32)
            np.array([k.shape[0], mode], dtype=np.int32).tofile(f)
            k.tofile(f)
