"""The denoiser (dps_ttc_amd/unet.py) against the reference's UNet under shared synthetic weights, on the CPU.

tests/golden/unet.npz holds, per variant of tests/unet_ref.py, what the REFERENCE's architecture computes from
`fill_weights`' numbers: a float64 twin's output and VJP (the truth), the CRC-32 of its own fp32 output and VJP, and
its own fp32 error against the twin (e_ref, 7e-7 .. 1.8e-6).  A layout-compatible but numerically different UNet --
another qkv order, swapped cos / sin, `scale` for `1 + scale`, another skip order, `num_heads_upsample` ignored --
lands at rel-L2 0.1 .. 1; rounding lands at 1e-6.  The gate is the suite's TOL = 1e-5.
"""
import numpy as np
import pytest
import torch

import unet_ref as U
from standin import rel_l2


@pytest.fixture(scope="module")
def ref(golden):
    return golden("unet")


def product(name):
    from dps_ttc_amd.unet import create_model
    return U.fill_weights(create_model(**U.config(name))).eval()


def run(model, name, device="cpu"):
    x, t, w, labels = U.inputs(name)
    to = lambda a: None if a is None else torch.from_numpy(a).to(device)
    y, g = U.forward_and_vjp(model, to(x), to(t), to(w), to(labels))
    return y.cpu().numpy(), g.cpu().numpy()


def same_build(ref):
    """the fixture was written by this torch build on this CPU model: only then can the product's fp32 results be
    expected to equal the reference's bit for bit (the libraries sum in the same order)"""
    return list(ref["env"]) == U.cpu_build()


BIT_EQUAL = ("A", "B", "C", "D", "E")


@pytest.mark.parametrize("name", U.CPU_VARIANTS)
def test_unet_matches_reference_float64(ref, name):
    """output and VJP within TOL of the reference's float64 twin; and where the fixture comes from this torch build,
    bit for bit the reference's own fp32 numbers: the product states the same operations in the same order, except
    attention, where scaled_dot_product_attention rounds like the reference's einsums up to 16 x 16 tokens.  A64
    attends over 32 x 32 and 64 x 64 tokens, where torch's CPU attention kernel sums in blocks: measured 1.01 x e_ref
    on the output, not the same bits, so bit equality is reported there and not asserted."""
    x, _, w, _ = U.inputs(name)
    assert U.crc(x) == ref[f"{name}.x_crc"] and U.crc(w) == ref[f"{name}.w_crc"], "the seeded inputs drifted"
    saved = torch.get_num_threads()
    torch.set_num_threads(int(ref["threads"]))
    try:
        y, g = run(product(name), name)
    finally:
        torch.set_num_threads(saved)
    whole, bad = U.stored_whole(name), []
    for what, a, tag in (("out", y, "y"), ("grad", g, "g")):
        err = rel_l2(U.pick(f"{name}.{tag}", a, whole), ref[f"{name}.{tag}64"])
        e_ref = float(ref[f"{name}.e_ref_{what}"])
        bits = U.crc(a) == ref[f"{name}.{tag}32_crc"]
        line = (f"unet {name} cpu {what}: err {err:.3e}  e_ref {e_ref:.3e}  ratio {err / e_ref:.2f}  "
                f"bit-equal to the reference's fp32: {bool(bits)}")
        print(line)
        if not err <= U.TOL or (same_build(ref) and name in BIT_EQUAL and not bits):
            bad.append(line)
    assert not bad, "; ".join(bad)


def test_unet_shared_timestep_broadcasts(ref):
    """t of shape [1] over two particles (how the loops call the model) = t of shape [2] with equal entries.  Not bit
    for bit: the embedding's Linear layers see one row in one case and two in the other, and the BLAS picks another
    kernel.  Both are fp32 evaluations of the same function, each within e_ref <= TOL / 4 of it, so TOL / 2 holds."""
    m = product("A")
    x, _, w, _ = U.inputs("A")
    x, w = torch.from_numpy(x), torch.from_numpy(w)
    y1, g1 = U.forward_and_vjp(m, x, torch.tensor([250.0]), w)
    y2, g2 = U.forward_and_vjp(m, x, torch.tensor([250.0, 250.0]), w)
    y3, _ = U.forward_and_vjp(m, x, torch.tensor([250.0, 3.0]), w)
    errs = rel_l2(y1.numpy(), y2.numpy()), rel_l2(g1.numpy(), g2.numpy()), rel_l2(y3[0].numpy(), y1[0].numpy())
    print("unet A cpu t [1] against t [2]: out %.3e  grad %.3e  first particle of t = [250, 3] %.3e" % errs)
    assert max(errs) <= U.TOL / 2
    assert rel_l2(y3[1].numpy(), y1[1].numpy()) > 0.1          # the second particle did get its own timestep


def test_unet_complete_checkpoint_loads(tmp_path, capsys):
    """create_model(model_path=...) with a complete checkpoint computes what the in-memory fill computes, bit for
    bit, and not what a fresh random init computes: the reference's `except Exception: print(...)` fallback (kept)
    would otherwise hide a checkpoint that did not load"""
    from dps_ttc_amd.unet import create_model
    filled = product("A")
    path = str(tmp_path / "filled.pt")
    torch.save(filled.state_dict(), path)
    capsys.readouterr()
    loaded = create_model(model_path=path, **U.config("A")).eval()
    assert "Randomly initialize" not in capsys.readouterr().out
    fresh = create_model(**U.config("A")).eval()
    assert "Randomly initialize" in capsys.readouterr().out
    (y0, g0), (y1, g1), (y2, _) = (run(m, "A") for m in (filled, loaded, fresh))
    assert np.array_equal(y0, y1) and np.array_equal(g0, g1)
    assert rel_l2(y2, y0) > 0.1
