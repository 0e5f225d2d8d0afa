"""CPU suite of what the analysis entries share (image metrics, particle repulsion, ensemble statistics, order statistics,
principal components): the byte totals of the five size queries, pinned to the numbers the library returned before the
layouts were moved onto one carver (csrc/common.h: Carver); the refusals of the one shape rule (particle_set_shape) as
every family applies it; and the same rule in the Python front ends (kernels._particle_shape).  No GPU: the size queries
are host functions and the shape rule of the front ends is separate from their device check.

The labels helper (kernels._label_rows with `images`) asks for the device first and is covered on the GPU: its texts by
test_pca_gpu.py::test_the_labels_of_the_images, its refusals through a front end by
test_quantile_gpu.py::test_refusals_come_as_value_errors_before_any_launch."""
import pytest

FAMILIES = ("repulse", "ensemble", "quantiles", "pca")
MAX_K = {"repulse": 512, "ensemble": 4096, "quantiles": 512, "pca": 128}
EINVAL, EUNSUPPORTED = -1, -2

# (n, d, images) -> dpsx_{repulse, ensemble, quantiles, pca}_workspace_bytes, recorded from the library built from the
# commit before the carver.  Up to about (8, 256, 2) every region is one 256-byte unit, so the rows that pin the formulas
# are the large ones: full slot counts, K across the tile and batch sizes, several images, d % 4 != 0.
SET_BYTES = {
    (64, 196608, 1): (493056, 51456, 211968, 509440),
    (64, 196608, 4): (377344, 56064, 258048, 381440),
    (128, 12288, 1): (521728, 7680, 102144, 587264),
    (130, 768, 2): (88832, 2304, 7168, 122880),
    (512, 48, 1): (2620928, 5120, 2816, EUNSUPPORTED),
    (7, 5, 1): (1280, 1280, 768, 1536),
    (1, 1, 1): (1280, 1280, 768, 1536),
    (8, 256, 2): (1280, 1280, 768, 1536),
    (6, 768, 1): (1280, 1280, 768, 1536),
    (6, 3072, 2): (1280, 1280, 1280, 1536),
    (96, 3072, 3): (43008, 2560, 5632, 55296),
    (256, 196608, 2): (1303040, 201216, 1089536, 1434112),
    (4096, 1024, 1): (EUNSUPPORTED, 33792, EUNSUPPORTED, EUNSUPPORTED),
    (1024, 100000, 2): (5241344, 408064, 4235264, EUNSUPPORTED),
    (33, 1000003, 3): (173312, 40704, 196608, 174848),
    (12, 786432, 12): (1536, 37632, 294912, 1792),
}
# (n, m, c, h, w) -> dpsx_metrics_workspace_bytes, recorded the same way
METRICS_BYTES = {
    (64, 1, 3, 256, 256): 98816,
    (64, 4, 3, 256, 256): 100352,
    (3, 3, 2, 11, 43): 768,
    (4, 1, 1, 5, 4): 768,
    (6, 2, 3, 16, 16): 768,
    (6, 1, 3, 32, 32): 768,
    (1, 1, 1, 1, 1): 768,
    (0, 1, 3, 64, 64): 512,
    (9, 3, 1, 75, 300): 3072,
    (130, 2, 3, 512, 512): 533504,
}


def _query(family):
    from dps_ttc_amd import _lib
    return getattr(_lib.lib(), f"dpsx_{family}_workspace_bytes")


@pytest.mark.parametrize("shape", list(SET_BYTES), ids=lambda s: "x".join(map(str, s)))
def test_particle_set_size_queries_are_the_recorded_totals(shape):
    got = tuple(int(_query(f)(*shape)) for f in FAMILIES)
    print(f"{shape}: {dict(zip(FAMILIES, got))}")
    assert got == SET_BYTES[shape]


@pytest.mark.parametrize("shape", list(METRICS_BYTES), ids=lambda s: "x".join(map(str, s)))
def test_metrics_size_query_is_the_recorded_total(shape):
    got = int(_query("metrics")(*shape))
    print(f"{shape}: {got}")
    assert got == METRICS_BYTES[shape]


@pytest.mark.parametrize("family", FAMILIES)
def test_the_shape_rule_per_family(family):
    """one rule, the family's K limit and whether an empty set is one: DPSX_EINVAL for a set that is none, DPSX_EUNSUPPORTED
    for one the launches cannot index, the invalid before the unsupported"""
    q, k = _query(family), MAX_K[family]
    assert q(k, 64, 1) > 0 and q(3 * k, 64, 3) > 0 and q(65535, 4, 65535) > 0 and q(2, 2 ** 31 - 1, 1) > 0
    empty = q(0, 64, 1)
    assert empty > 0 if family == "repulse" else empty == EINVAL         # the repulsion entries take an empty set
    for bad in ((-1, 64, 1), (9, 64, 2), (8, 64, 3), (8, 0, 2), (8, -1, 2), (8, 64, 0), (8, 64, -1)):
        assert q(*bad) == EINVAL, bad
    assert q(k + 1, 64, 1) == EUNSUPPORTED and q(2 * (k + 1), 64, 2) == EUNSUPPORTED
    assert q(65536, 64, 65536) == EUNSUPPORTED and q(2, 2 ** 31, 1) == EUNSUPPORTED
    assert q(k + 2, 0, 1) == EINVAL and q(65537, 64, 65536) == EINVAL and q(-1, 2 ** 31, 1) == EINVAL


def test_the_shape_rule_of_the_front_ends():
    """kernels._particle_shape: the rule every front end applies to its particles after the device check, with the texts the
    front ends have always raised"""
    from dps_ttc_amd import kernels
    rule = kernels._particle_shape
    assert rule((6, 3, 16, 16), 2) == (6, 3, 768, 2) and rule((6, 3, 16, 16), 1) == (6, 6, 768, 1)
    assert rule((8, 5), 4, nchw=False) == (8, 2, 5, 4) and rule((4, 2, 3, 5, 7), 2, nchw=False) == (4, 2, 210, 2)
    assert rule((0, 3, 16, 16), 1, nchw=False, allow_empty=True) == (0, 0, 768, 1)
    assert rule((0, 3, 16, 16), 3, allow_empty=True) == (0, 0, 768, 3)
    assert rule((2, 1, 65536, 32768), 1)[2] == 2 ** 31                   # D is not a 32-bit product
    for shape in ((6, 3, 16), (6, 3, 16, 16, 1), (6,), ()):
        with pytest.raises(ValueError, match=r"^particles must be \[N, C, H, W\] \(got \(.*\)\)$"):
            rule(shape, 1)
    for shape in ((6,), ()):
        with pytest.raises(ValueError, match=r"^particles must be \[N, \.\.\.\] \(got \(.*\)\)$"):
            rule(shape, 1, nchw=False)
    for n, images, kw in ((6, 4, {}), (6, 0, {}), (6, -1, {}), (0, 1, {}), (0, 2, {}), (7, 2, dict(allow_empty=True)),
                          (0, 0, dict(allow_empty=True))):
        with pytest.raises(ValueError, match=rf"^{n} particles do not split into {images} images$"):
            rule((n, 3, 16, 16), images, **kw)
    with pytest.raises(ValueError, match="particles must be"):           # the dimensions before the split
        rule((6, 3, 16), 4)
