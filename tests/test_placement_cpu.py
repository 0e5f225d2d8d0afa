"""The placement harness (tests/placement.py) proved on CPU tensors: a fake "entry" written in numpy computes
out = 2 x and a byte gate inside its buffers; each planted violation must be reported by the check meant for it, and by no
other, and the clean call must pass at every placement."""
import numpy as np
import pytest
import torch

import placement
from placement import GUARD, Arena, Buf

OK, REFUSED = 0, -2
N = 24          # a multiple of 4: only the address decides the form
BUFS = [Buf("x", (N,), torch.float32, "in"), Buf("out", (N,), torch.float32, "out"),
        Buf("gate", (N,), torch.uint8, "out"), Buf("idx", (2,), torch.int64, "out"),
        Buf("acc", (N,), torch.float32, "inout"), Buf("ws", (40,), torch.uint8, "ws")]
OUTS = ("out", "gate", "idx")


def _entry(a, plant=None, refuse=False):
    """the fake library call: works on the arena's bytes through the raw positions, like a kernel does"""
    mem = a.mem.numpy()                                   # shares the tensor's memory

    def words(name):
        lo, hi = a.span[name]
        return np.frombuffer(mem[lo:hi].tobytes(), dtype=np.float32)

    def store(name, values):
        lo, hi = a.span[name]
        mem[lo:hi] = np.frombuffer(np.ascontiguousarray(values).tobytes(), dtype=np.uint8)

    if refuse:
        if plant == "write_after_refusal":
            lo, _ = a.span["out"]
            mem[lo + 8] = 0
        return REFUSED
    x = words("x")
    y = (2 * x).astype(np.float32)
    store("out", y)
    store("gate", (np.abs(x) <= 1).astype(np.uint8))
    store("idx", np.array([int(np.argmin(x)), int(np.argmax(x))], dtype=np.int64))
    acc = words("acc").copy()
    acc[: N // 2] = x[: N // 2]                          # half of an inout buffer: the rest keeps the caller's values
    store("acc", acc)
    lo, hi = a.span["out"]
    if plant == "before":
        mem[lo - 4:lo] = np.frombuffer(np.float32(1.0).tobytes(), dtype=np.uint8)
    elif plant == "after":
        mem[hi] = 0
    elif plant == "unwritten":
        mem[lo + 4 * 5:lo + 4 * 6] = placement.FILL
    elif plant == "unwritten_byte":
        glo, _ = a.span["gate"]
        mem[glo + 3] = placement.FILL
    elif plant == "unwritten_i64":
        ilo, _ = a.span["idx"]
        mem[ilo + 8:ilo + 16] = placement.FILL
    elif plant == "far":
        mem[hi + GUARD - 1] = 7                          # the last byte of the band behind `out`
    return OK


def _run(offsets, plant=None, refuse=False):
    a = Arena(BUFS, offsets)
    x = np.linspace(-2, 2, N).astype(np.float32)
    a.put("x", x)
    a.put("acc", np.zeros(N, dtype=np.float32))
    before = a.snapshot()
    rc = _entry(a, plant, refuse)
    return a, x, rc, a.violations(rc == OK, written=OUTS, before=before)


PLACEMENTS = placement.placements(["x", "out", "gate", "acc"], lambda n: 1 if n == "gate" else 4)


def test_the_placements_of_a_case():
    assert [p[0] for p in PLACEMENTS] == ["aligned", "all", "x", "out", "gate", "acc"]
    assert PLACEMENTS[1][1] == {"x": 4, "out": 4, "gate": 1, "acc": 4} and PLACEMENTS[4][1] == {"gate": 1}
    assert placement.placements(["x"], lambda n: 4) == [("aligned", {}), ("x", {"x": 4})]


@pytest.mark.parametrize("tag,offsets", PLACEMENTS)
def test_layout(tag, offsets):
    a = Arena(BUFS, offsets)
    spans = sorted(a.span.values())
    assert spans[0][0] >= GUARD and a.mem.numel() - spans[-1][1] >= GUARD
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert lo - hi >= GUARD                                  # a whole band between any two buffers
    for b in BUFS:
        assert a.addr(b.name) % 16 == offsets.get(b.name, 0)     # the absolute address, not the position
        assert a.nbytes(b.name) == placement.nbytes_of(b)        # exact size: no rounding, no minimum
        assert a.ptr(b.name).value == a.addr(b.name)
    assert a.nbytes("ws") == 40 and a.ptr(None) is None
    assert int(a.guard.sum()) == a.mem.numel() - sum(placement.nbytes_of(b) for b in BUFS)
    assert bool((a.mem == placement.FILL).all())
    assert torch.isnan(a.get("out")).all() and bool((a.get("idx") == -1).all()) and bool((a.get("gate") == 255).all())


@pytest.mark.parametrize("tag,offsets", PLACEMENTS)
def test_clean_call_passes(tag, offsets):
    a, x, rc, v = _run(offsets)
    assert rc == OK and v == []
    assert np.array_equal(a.get("out").numpy(), 2 * x) and np.array_equal(a.get("x").numpy(), x)
    assert a.get("idx").tolist() == [0, N - 1]
    assert np.array_equal(a.get("acc").numpy()[N // 2:], np.zeros(N - N // 2, dtype=np.float32))


@pytest.mark.parametrize("tag,offsets", PLACEMENTS)
@pytest.mark.parametrize("plant,kind,where", [
    ("before", "guard", "4 guard bytes changed, first 4 bytes before out"),
    ("after", "guard", "1 bytes after out"),
    ("far", "guard", ""),
    ("unwritten", "unwritten", "of out still hold the fill, first element 5"),
    ("unwritten_byte", "unwritten", "of gate still hold the fill, first element 3"),
    ("unwritten_i64", "unwritten", "of idx still hold the fill, first element 1"),
])
def test_each_planted_violation_is_reported_by_its_check(tag, offsets, plant, kind, where):
    a, x, rc, v = _run(offsets, plant)
    assert rc == OK
    assert len(v) == 1 and v[0].startswith(kind + ":"), v
    assert where in v[0], v


def test_refusal_that_wrote_nothing_passes():
    a, x, rc, v = _run({}, refuse=True)
    assert rc == REFUSED and v == []
    assert torch.isnan(a.get("out")).all()


@pytest.mark.parametrize("tag,offsets", PLACEMENTS)
def test_write_after_refusal_is_reported(tag, offsets):
    a, x, rc, v = _run(offsets, "write_after_refusal", refuse=True)
    assert rc == REFUSED
    assert v == ["written after refusal: 1 bytes changed, first byte 8 of out"]


def test_refusal_needs_its_snapshot():
    a = Arena(BUFS)
    with pytest.raises(AssertionError, match="snapshot"):
        a.violations(False, written=OUTS)


def test_put_checks_type_and_size_and_unknown_offsets():
    a = Arena(BUFS)
    with pytest.raises(AssertionError):
        a.put("x", np.zeros(N, dtype=np.float64))
    with pytest.raises(AssertionError):
        a.put("x", np.zeros(N + 1, dtype=np.float32))
    with pytest.raises(AssertionError, match="unknown"):
        Arena(BUFS, {"nope": 4})
    with pytest.raises(AssertionError):
        Arena(BUFS, {"x": 2})                             # an fp32 buffer needs 4-byte alignment
