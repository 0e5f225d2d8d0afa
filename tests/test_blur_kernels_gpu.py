"""GPU suite (-m gpu): degenerate blur kernels on every route of csrc/blur.hip against the CPU oracle (taps accumulated
in double).  The kernels are the named families of tests/blur_families.py -- the host check (test_blur_tables_cpu.py)
shows that between them they take every route the launchers choose from the tap tables -- on the smallest image shapes
that differ in route.  Gates are the suite's own: rel-L2 < 1e-5 for forward, adjoint, norm and gradient, 1e-6 for sample
and x_{t-1}, bit-exact x0_hat and clamp gate, and <A x, u> = <x, A^T u> as in test_hip_parity.py.  A single tap of weight 1
must reproduce numpy's reflect-pad-and-slice bit for bit (1 * x plus exact zeros): an index error shows per pixel.

Every figure is printed before it is asserted (lines starting with BLURFIG, pytest -s): profiles/blur_kernel_tests.txt."""
import json

import numpy as np
import pytest
import torch

import blur_families as bf
from standin import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"
N, C = 2, 3

FAMILIES = bf.named_families()
# AUTO for every member; FORCE_TAPS as well where AUTO takes the separable route (both are then meaningful)
CASES = [(f, name, k, rank1, mode) for f, name, k, rank1 in FAMILIES for mode in (("auto", "taps") if rank1 else ("auto",))]
# the fused step: one kernel per family
STEP_MEMBERS = ("F1.ks61.tl", "F2.ks61.row.first", "F3.ks61.antidiag", "F4.ks31.odd.seg8", "F5.ks9.last3",
                "F6.ks9.dense_signed", "F7.ks61.pedestal")
STEP_CASES = [c for c in CASES if f"{c[0]}.{c[1]}" in STEP_MEMBERS]
_id = lambda c: f"{c[0]}.{c[1]}-{c[4]}"


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy()


def _handle(K, k, rank1, mode):
    h = K.OpHandle.blur(k, DEV, force_taps=(mode == "taps"))
    assert h.kind == (K._lib.KIND_SEP if rank1 and mode == "auto" else K._lib.KIND_TAPS)
    return h


def _figure(case, route, hw, **figs):
    print("BLURFIG " + json.dumps({"family": case[0], "kernel": case[1], "mode": case[4], "route": route,
                                   "hw": list(hw), **{k: float(v) for k, v in figs.items()}}))


def test_step_members_exist():
    assert sorted(f"{c[0]}.{c[1]}" for c in STEP_CASES if c[4] == "auto") == sorted(STEP_MEMBERS)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_adjoint_score(K, oracle, case):
    fam, name, k, rank1, mode = case
    h = _handle(K, k, rank1, mode)
    r = k.shape[0] // 2
    rng = np.random.RandomState(k.shape[0] + len(name))
    refused = 0
    for hw in dict.fromkeys(bf.image_shapes(k)):
        if not bf.admits(k, hw):         # the reflection pad does not fit: refused before any launch, not skipped
            with pytest.raises(K._lib.DpsxError):
                h.forward(torch.zeros(1, 1, *hw, device=DEV))
            with pytest.raises(K._lib.DpsxError):
                h.adjoint(torch.zeros(1, 1, *hw, device=DEV), in_hw=hw)
            refused += 1
            continue
        if fam == "F7" and hw == (128, 128):
            continue                     # the oracle's time on a dense 61 x 61 list; test_taps_regular_multi_tile has that route
        x = rng.randn(N, C, *hw).astype(np.float32)
        u = rng.randn(N, C, *hw).astype(np.float32)
        ym = rng.randn(1, C, *hw).astype(np.float32)
        y = h.forward(dev(x))
        g = h.adjoint(dev(u), in_hw=hw)
        costs = h.score(dev(x), dev(ym))
        ref_y, ref_g = oracle.blur_fwd(x, k), oracle.blur_adj(u, k)
        ref_c = np.sqrt(((ym.astype(np.float64) - ref_y.astype(np.float64)) ** 2).reshape(N, -1).sum(axis=1))
        lhs = (y.double() * dev(u).double()).sum().item()
        rhs = (dev(x).double() * g.double()).sum().item()
        bound = 2e-5 * max(abs(lhs), np.sqrt(float(y.numel())))
        _figure(case, "fwd_adj_score", hw, forward=rel_l2(host(y), ref_y), adjoint=rel_l2(host(g), ref_g),
                score=rel_l2(host(costs), ref_c), inner=abs(lhs - rhs) / bound)
        if fam == "F1":                  # 1 * x plus exact zeros
            (ti,), (tj,) = np.nonzero(k)
            pad = np.pad(x, ((0, 0), (0, 0), (r, r), (r, r)), mode="reflect")
            np.testing.assert_array_equal(host(y), pad[:, :, ti:ti + hw[0], tj:tj + hw[1]], err_msg=f"{hw}")
        assert rel_l2(host(y), ref_y) < TOL, f"forward {hw}"
        assert rel_l2(host(g), ref_g) < TOL, f"adjoint {hw}"
        assert rel_l2(host(costs), ref_c) < TOL, f"score {hw}"
        assert abs(lhs - rhs) <= bound, f"inner product {hw}"
    # only the shape built from the staged halo can fall below the pad (a tap near the centre of a large grid)
    assert refused == (0 if bf.radius4_of(k) > r else 1)


@pytest.mark.parametrize("case", STEP_CASES, ids=_id)
def test_fused_step(K, oracle, case):
    """step_fwd (norm finished by the launch or by step_bwd), step_bwd (with and without an extra cotangent on x0_hat) and
    step_update on the raw handle against oracle.dps_step; at 64 x 64 also step_fwd with the noise drawn in the kernel"""
    fam, name, k, rank1, mode = case
    h = _handle(K, k, rank1, mode)
    orc = oracle.make_operator("motion_blur", kernel=k)
    t, scale = 500, 0.7
    c = oracle.tables.step_coefs(oracle.tables.schedule(1000), t)
    ck = K.make_coefs(c["a"], c["b"], c["c1"], c["c2"], c["min_log"], c["max_log"], c["add_noise"])
    for hw in ((64, 64), (50, 46)):
        rng = np.random.RandomState(hw[0] + k.shape[0])
        shape = (N, C, *hw)
        x_prev = rng.randn(*shape).astype(np.float32)
        eps = ((c["a"] * x_prev - 1.4 * np.tanh(rng.randn(*shape))) / c["b"]).astype(np.float32)
        mo = np.concatenate([eps, rng.uniform(-1, 1, shape).astype(np.float32)], axis=1)
        y = (orc.forward(rng.uniform(-1, 1, (1, C, *hw)).astype(np.float32)) + 0.05 * rng.randn(1, C, *hw)).astype(np.float32)
        g_unet = (1e-2 * rng.randn(*shape)).astype(np.float32)
        g_extra = (0.05 * rng.randn(*shape)).astype(np.float32)
        draws = [("noise", rng.randn(*shape).astype(np.float32), None)]
        if hw == (64, 64) and h.draws_in_kernel(C, *hw):
            r = K.Rng(41, t, particle_base=3)
            draws.append(("rng", host(K.randn(shape, r, DEV)), r))
        buf = K.StepBuffers(h, N, C, hw[0], hw[1], DEV)
        for draw, noise, r in draws:
            for extra, power in ((False, 1), (True, 2)):
                ref = oracle.dps_step(orc, x_prev, mo, noise, y, c, scale=scale, power=power, g_unet_fn=lambda g: g_unet,
                                      g_x0_extra=g_extra if extra else None)
                for finalize in (False, True):
                    K.step_fwd(h, buf, dev(x_prev), dev(mo), None if r else dev(noise), dev(y), ck, finalize_norm=finalize,
                               rng=r)
                    norm_k1 = host(buf.norm) if finalize else None
                    K.step_bwd(h, buf, dev(y), scale, power, ck, g_x0_extra=dev(g_extra) if extra else None)
                    x_next = host(K.step_update(buf, dev(g_unet), ck))
                    figs = dict(sample=rel_l2(host(buf.sample), ref["sample"]), norm=rel_l2(host(buf.norm), ref["norm"]),
                                gradient=rel_l2(host(buf.g_model_out), ref["g_model_out"]),
                                update=rel_l2(x_next - ref["sample"], ref["x_next"] - ref["sample"]),
                                x_next=rel_l2(x_next, ref["x_next"]))
                    _figure(case, f"step.{draw}.{'extra' if extra else 'plain'}.{'k1norm' if finalize else 'k2norm'}", hw, **figs)
                    what = f"{hw} {draw} extra={extra} finalize={finalize}"
                    np.testing.assert_array_equal(host(buf.x0_hat), ref["x0_hat"], err_msg=what)
                    np.testing.assert_array_equal(buf.inside.cpu().numpy(), ref["inside"], err_msg=what)
                    if finalize:
                        assert rel_l2(norm_k1, ref["norm"]) < TOL, what
                    assert figs["sample"] < 1e-6, what
                    assert figs["norm"] < TOL, what
                    assert figs["gradient"] < TOL, what
                    assert np.all(host(buf.g_model_out)[:, C:] == 0), what
                    assert figs["update"] < TOL, what
                    assert figs["x_next"] < 1e-6, what
