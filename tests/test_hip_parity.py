"""GPU suite (-m gpu): the HIP path through the C ABI against the oracle and the golden fixtures.

Tolerances (rel-L2 = ||a-b||_2 / ||b||_2 over the whole tensor):
  * 1e-5 on operator outputs, adjoints, norms, gradients, x0_hat / x_{t-1}  (gate in BASELINE.json: 1e-4)
  * bit-exact: S1's x0_hat and clamp gate, inpainting A(x) / A^T(u), every argmin / gather index.
"""
import numpy as np
import pytest
import torch

from standin import StandInModel, rel_l2, synthetic_motion_kernel

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy()


def coefs_of(K, oracle, t, sched=None):
    c = oracle.tables.step_coefs(sched or oracle.tables.schedule(1000), t)
    return c, K.make_coefs(c["a"], c["b"], c["c1"], c["c2"], c["min_log"], c["max_log"], c["add_noise"])


# ----------------------------------------------------------------- S1
@pytest.mark.parametrize("t", [999, 500, 1, 0])
def test_posterior_step_golden(K, oracle, golden, t):
    g = golden("posterior")
    c, ck = coefs_of(K, oracle, t)
    x0, sample, inside = K.posterior_fwd(dev(g["x"]), dev(g[f"t{t}.model_out"]), dev(g[f"t{t}.noise"]), ck,
                                         want_inside=True)
    np.testing.assert_array_equal(host(x0), g[f"t{t}.x0_hat"])          # bit-exact vs the reference
    assert rel_l2(host(sample), g[f"t{t}.sample"]) < 1e-6
    o = oracle.posterior_fwd(g["x"], g[f"t{t}.model_out"], g[f"t{t}.noise"], c)
    np.testing.assert_array_equal(inside.cpu().numpy(), o["inside"])
    gx, gmo = K.posterior_bwd(dev(g["w_x0"]), dev(g["w_s"]), dev(g["x"]), dev(g[f"t{t}.model_out"]),
                              dev(g[f"t{t}.noise"]), ck)
    assert rel_l2(host(gx), g[f"t{t}.g_x"]) < TOL
    assert rel_l2(host(gmo), g[f"t{t}.g_model_out"]) < TOL


def ddim_coefs_of(K, oracle, t, eta, sched=None):
    sched = sched or oracle.tables.schedule(1000)
    c = oracle.tables.ddim_step_coefs(sched, t, eta)
    ck = K.make_ddim_coefs(sched["sqrt_recip_alphas_cumprod"][t], sched["sqrt_recipm1_alphas_cumprod"][t],
                           sched["alphas_cumprod"][t], sched["alphas_cumprod_prev"][t], eta, t != 0)
    return c, ck


@pytest.mark.parametrize("t,eta", [(999, 0.0), (500, 0.0), (1, 0.0), (0, 0.0), (500, 0.5), (0, 0.5)])
def test_ddim_step_golden(K, oracle, golden, t, eta):
    """DDIM variant of S1 (reference gaussian_diffusion.py:479-509): HIP forward and VJP against the reference"""
    g = golden("ddim")
    tag = f"t{t}.eta{eta:g}"
    c, ck = ddim_coefs_of(K, oracle, t, eta)
    x0, sample = K.posterior_fwd(dev(g["x"]), dev(g[f"{tag}.model_out"]), dev(g[f"{tag}.noise"]), ck)
    np.testing.assert_array_equal(host(x0), g[f"{tag}.x0_hat"])
    assert rel_l2(host(sample), g[f"{tag}.sample"]) < 1e-6
    o = oracle.posterior_fwd(g["x"], g[f"{tag}.model_out"], g[f"{tag}.noise"], c)
    np.testing.assert_array_equal(host(sample), o["sample"])               # same op order as the oracle: bit-exact
    gx, gmo = K.posterior_bwd(dev(g["w_x0"]), dev(g["w_s"]), dev(g["x"]), dev(g[f"{tag}.model_out"]),
                              dev(g[f"{tag}.noise"]), ck)
    assert rel_l2(host(gx), g[f"{tag}.g_x"]) < TOL
    assert rel_l2(host(gmo), g[f"{tag}.g_model_out"]) < TOL
    # through autograd, as the per-op path uses it
    xx, mo = dev(g["x"]).requires_grad_(), dev(g[f"{tag}.model_out"]).requires_grad_()
    x0a, sa = K.PosteriorStepFn.apply(xx, mo, dev(g[f"{tag}.noise"]), ck)
    ga, gb = torch.autograd.grad((x0a * dev(g["w_x0"])).sum() + (sa * dev(g["w_s"])).sum(), [xx, mo])
    assert rel_l2(host(ga), g[f"{tag}.g_x"]) < TOL and rel_l2(host(gb), g[f"{tag}.g_model_out"]) < TOL


@pytest.mark.parametrize("shape", [(3, 3, 17, 13), (2, 3, 64, 64), (1, 1, 5, 3)])
def test_posterior_step_ragged_vs_oracle(K, oracle, shape):
    rng = np.random.RandomState(0)
    x = rng.randn(*shape).astype(np.float32)
    mo = rng.randn(shape[0], 2 * shape[1], *shape[2:]).astype(np.float32)
    z = rng.randn(*shape).astype(np.float32)
    for t in (700, 0):
        c, ck = coefs_of(K, oracle, t)
        x0, sample, inside = K.posterior_fwd(dev(x), dev(mo), dev(z), ck, want_inside=True)
        o = oracle.posterior_fwd(x, mo, z, c)
        np.testing.assert_array_equal(host(x0), o["x0_hat"])
        np.testing.assert_array_equal(inside.cpu().numpy(), o["inside"])
        assert rel_l2(host(sample), o["sample"]) < 1e-6


def test_posterior_empty_batch(K, oracle):
    _, ck = coefs_of(K, oracle, 10)
    x0, sample = K.posterior_fwd(torch.empty(0, 3, 8, 8, device=DEV), torch.empty(0, 6, 8, 8, device=DEV),
                                 torch.empty(0, 3, 8, 8, device=DEV), ck)
    assert x0.shape == (0, 3, 8, 8) and sample.shape == (0, 3, 8, 8)


# ----------------------------------------------------------------- operators
def _inputs(g, tag):
    if f"{tag}.x" in g.keys():
        return g[f"{tag}.x"], g[f"{tag}.u"]
    gen = torch.Generator().manual_seed(int(g[f"{tag}.seed"]))
    shape = [int(v) for v in g[f"{tag}.shape"]]
    x = torch.rand(*shape, generator=gen) * 2 - 1
    u = torch.randn(*g[f"{tag}.y"].shape, generator=gen)
    return x.numpy(), u.numpy()


def _pair(hw):
    """hw: a side or an (h, w) pair -> (h, w, an int to seed with)"""
    h, w = (hw, hw) if isinstance(hw, int) else hw
    return h, w, h + w if h != w else h


def make_product_op(name, g=None, hw=64, **extra):
    from dps_ttc_amd.measurements import get_operator
    if name == "gauss":
        return get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV), {}
    if name == "motion":
        op = get_operator("motion_blur", kernel_size=61, intensity=0.5, device=DEV)
        op._set_weights(extra["kernel"])         # inject the fixture's kernel exactly as stored in the conv weight
        return op, {}
    if name in ("sr4", "sr8"):
        return get_operator("super_resolution", in_shape=(1, 3, hw, hw), scale_factor=int(name[2:]), device=DEV), {}
    if name == "inpaint":
        return get_operator("inpainting", device=DEV), {"mask": dev(extra["mask"])}
    if name == "phase":
        return get_operator("phase_retrieval", oversample=2.0, device=DEV), {}
    if name == "denoise":
        return get_operator("noise", device=DEV), {}
    raise KeyError(name)


def make_oracle_op(oracle, name, hw=64, **extra):
    if name == "gauss":
        return oracle.make_operator("gaussian_blur", kernel_size=61, intensity=3.0)
    if name == "motion":
        return oracle.make_operator("motion_blur", kernel=extra["kernel"])
    if name in ("sr4", "sr8"):
        return oracle.make_operator("super_resolution", in_shape=(1, 3, hw, hw), scale_factor=int(name[2:]))
    if name == "inpaint":
        return oracle.make_operator("inpainting", mask=extra["mask"])
    if name == "phase":
        return oracle.make_operator("phase_retrieval", oversample=2.0)
    if name == "denoise":
        return oracle.make_operator("noise")
    raise KeyError(name)


@pytest.mark.parametrize("tag", ["gauss.small", "gauss.full", "motion.small", "sr4.small", "sr4.full",
                                 "sr8.full", "inpaint.small", "phase.small", "phase.full"])
def test_operator_forward_adjoint_golden(K, golden, tag):
    g = golden("operators")
    x, u = _inputs(g, tag)
    name = tag.split(".")[0]
    op, fkw = make_product_op(name, hw=x.shape[-1], kernel=g["motion.kernel"], mask=g["inpaint.mask"])
    xt = dev(x).requires_grad_()
    y = op.forward(xt, **fkw)
    (adj,) = torch.autograd.grad((y * dev(u)).sum(), xt)       # the HIP adjoint through autograd
    if name == "inpaint":
        np.testing.assert_array_equal(host(y), g[f"{tag}.y"])
        np.testing.assert_array_equal(host(adj), g[f"{tag}.adj"])
    else:
        assert rel_l2(host(y), g[f"{tag}.y"]) < TOL, "forward"
        assert rel_l2(host(adj), g[f"{tag}.adj"]) < TOL, "adjoint"


@pytest.mark.parametrize("hw", [(64, 64), (50, 46), (33, 96), (130, 72)])
@pytest.mark.parametrize("kind", ["gauss_sep", "gauss_taps", "motion"])
def test_blur_paths_vs_oracle(K, oracle, kind, hw):
    """separable LDS path, tap-list path, ragged sizes (scalar loads, partial tiles, folds on both borders)."""
    rng = np.random.RandomState(1)
    if kind == "motion":
        k2 = synthetic_motion_kernel(61, 9)
    else:
        k2 = oracle.tables.gaussian_kernel2d(61, 3.0).astype(np.float32)
    h = K.OpHandle.blur(k2, DEV, force_taps=(kind == "gauss_taps"))
    assert h.kind == (K._lib.KIND_SEP if kind == "gauss_sep" else K._lib.KIND_TAPS)
    x = rng.randn(2, 3, *hw).astype(np.float32)
    u = rng.randn(2, 3, *hw).astype(np.float32)
    assert rel_l2(host(h.forward(dev(x))), oracle.blur_fwd(x, k2)) < TOL
    assert rel_l2(host(h.adjoint(dev(u), in_hw=hw)), oracle.blur_adj(u, k2)) < TOL


@pytest.mark.parametrize("ks,sigma", [(9, 1.0), (31, 0.5), (61, 5.0), (61, 7.5), (65, 8.0)])
def test_blur_other_radii(K, oracle, ks, sigma):
    """every separable radius bucket (taps reach 4..32) and asymmetric rank-1 kernels"""
    rng = np.random.RandomState(2)
    k2 = oracle.tables.gaussian_kernel2d(ks, sigma)
    k2 = (k2 * (1.0 + 0.3 * np.linspace(-1, 1, ks))[None, :] * (1.0 - 0.2 * np.linspace(-1, 1, ks))[:, None])
    k2 = k2.astype(np.float32)
    h = K.OpHandle.blur(k2, DEV)
    assert h.kind == K._lib.KIND_SEP
    x = rng.randn(1, 2, 80, 72).astype(np.float32)
    assert rel_l2(host(h.forward(dev(x))), oracle.blur_fwd(x, k2)) < TOL
    assert rel_l2(host(h.adjoint(dev(x), in_hw=(80, 72))), oracle.blur_adj(x, k2)) < TOL


@pytest.mark.parametrize("hw", [(128, 192), (192, 64), (64, 128)])
@pytest.mark.parametrize("ks,sigma", [(9, 1.0), (25, 2.0), (61, 3.0), (61, 7.5)])
def test_blur_regular_non_square(K, oracle, hw, ks, sigma):
    """the branch-free loader / in-window folds of the separable kernels on multi-tile non-square images (one, two and
    three tiles per axis), every radius bucket; plus the fused step there (x0_hat halo recomputed from neighbours)"""
    rng = np.random.RandomState(ks + hw[0])
    k2 = oracle.tables.gaussian_kernel2d(ks, sigma)
    k2 = (k2 * (1.0 + 0.3 * np.linspace(-1, 1, ks))[None, :]).astype(np.float32)
    h = K.OpHandle.blur(k2, DEV)
    assert h.kind == K._lib.KIND_SEP
    x = rng.randn(1, 3, *hw).astype(np.float32)
    assert rel_l2(host(h.forward(dev(x))), oracle.blur_fwd(x, k2)) < TOL
    assert rel_l2(host(h.adjoint(dev(x), in_hw=hw)), oracle.blur_adj(x, k2)) < TOL
    # fused forward half against the un-fused composition on the GPU (S1 then the plain operator)
    _, ck = coefs_of(K, oracle, 500)
    xt, mo, z = dev(rng.randn(2, 3, *hw).astype(np.float32)), dev(rng.randn(2, 6, *hw).astype(np.float32) * 0.3), \
        dev(rng.randn(2, 3, *hw).astype(np.float32))
    y = dev(rng.randn(1, 3, *hw).astype(np.float32))
    buf = K.StepBuffers(h, 2, 3, hw[0], hw[1], DEV)
    K.step_fwd(h, buf, xt, mo, z, y, ck, finalize_norm=True)
    x0, sm = K.posterior_fwd(xt, mo, z, ck)
    assert torch.equal(buf.x0_hat, x0) and torch.equal(buf.sample, sm)
    r = (y - h.forward(x0)).reshape(2, -1)
    assert rel_l2(host(buf.norm), host(r.norm(dim=1))) < TOL


def test_blur_rejects_pad_not_smaller_than_image(K, oracle):
    h = K.OpHandle.blur(oracle.tables.gaussian_kernel2d(61, 3.0), DEV)
    with pytest.raises(K._lib.DpsxError):
        h.forward(torch.zeros(1, 1, 30, 64, device=DEV))        # torch's ReflectionPad2d raises here too


@pytest.mark.parametrize("factor,hw", [(4, 64), (4, 256), (8, 256), (2, 96), (4, 36)])
def test_resize_vs_oracle(K, oracle, factor, hw):
    rng = np.random.RandomState(3)
    op, _ = make_product_op(f"sr{factor}" if factor in (4, 8) else "sr4", hw=hw)
    if factor not in (4, 8):
        from dps_ttc_amd.measurements import get_operator
        op = get_operator("super_resolution", in_shape=(1, 3, hw, hw), scale_factor=factor, device=DEV)
    orc = oracle.make_operator("super_resolution", in_shape=(1, 3, hw, hw), scale_factor=factor)
    x = rng.randn(2, 3, hw, hw).astype(np.float32)
    y = op.forward(dev(x))
    assert rel_l2(host(y), orc.forward(x)) < TOL
    u = rng.randn(*y.shape).astype(np.float32)
    assert rel_l2(host(op.hip_handle().adjoint(dev(u), in_hw=(hw, hw))), orc.adjoint(u, (hw, hw))) < TOL


@pytest.mark.parametrize("factor,shape", [(4, (128, 256)), (4, (256, 64)), (8, (64, 256)), (4, (48, 128))])
def test_resize_non_square_vs_oracle(K, oracle, factor, shape):
    """row-streaming forward / register-table adjoint on non-square images (wu = 64, 16, 32: 1, 4, 2 rows per wave-step)"""
    from dps_ttc_amd.measurements import get_operator
    rng = np.random.RandomState(factor + shape[0])
    op = get_operator("super_resolution", in_shape=(1, 3) + shape, scale_factor=factor, device=DEV)
    orc = oracle.make_operator("super_resolution", in_shape=(1, 3) + shape, scale_factor=factor)
    x = rng.randn(2, 3, *shape).astype(np.float32)
    y = op.forward(dev(x))
    assert rel_l2(host(y), orc.forward(x)) < TOL
    u = rng.randn(*y.shape).astype(np.float32)
    assert rel_l2(host(op.hip_handle().adjoint(dev(u), in_hw=shape)), orc.adjoint(u, shape)) < TOL


@pytest.mark.parametrize("in_hw,out_hw,taps", [((40, 48), (12, 10), (6, 5)), ((64, 64), (9, 16), (11, 3)), ((30, 52), (30, 13), (2, 7))])
def test_resize_arbitrary_tables_vs_dense(K, in_hw, out_hw, taps):
    """dpsx_op_create_resize takes ANY (weight, index) tables, not only the bicubic ones of resizer.py:55-74: random weights,
    random indices (repeats inside a column, input rows / columns that nothing reads, rows that more than four outputs read
    -- the CSR form of the adjoint's H pass, the staged-rows forward) against the dense matrices, forward and adjoint."""
    rng = np.random.RandomState(in_hw[0] + taps[0])
    (ih, iw), (oh, ow), (th, tw_) = in_hw, out_hw, taps
    w_h, w_w = rng.randn(th, oh).astype(np.float32), rng.randn(tw_, ow).astype(np.float32)
    i_h, i_w = rng.randint(0, ih, (th, oh)), rng.randint(0, iw, (tw_, ow))
    i_h[:, 0] = 3                                   # one input row read by every tap of an output: repeats
    i_h[i_h == 5] = 6                               # an input row nothing reads
    w_w[rng.rand(tw_, ow) < 0.2] = 0.0              # explicit zero weights
    handle = K.OpHandle.resize(ih, iw, w_h, i_h, w_w, i_w, DEV)
    Ah, Aw = np.zeros((oh, ih)), np.zeros((ow, iw))
    for k in range(th):
        for p in range(oh):
            Ah[p, i_h[k, p]] += w_h[k, p]
    for k in range(tw_):
        for o in range(ow):
            Aw[o, i_w[k, o]] += w_w[k, o]
    x = rng.randn(5, ih, iw).astype(np.float32)
    y = handle.forward(dev(x[:, None]))
    ref = np.einsum("pi,nij,oj->npo", Ah, x.astype(np.float64), Aw)
    assert tuple(y.shape) == (5, 1, oh, ow) and rel_l2(host(y)[:, 0], ref) < TOL
    u = rng.randn(5, oh, ow).astype(np.float32)
    g = handle.adjoint(dev(u[:, None]), in_hw=(ih, iw))
    refg = np.einsum("pi,npo,oj->nij", Ah, u.astype(np.float64), Aw)
    assert tuple(g.shape) == (5, 1, ih, iw) and rel_l2(host(g)[:, 0], refg) < TOL
    assert np.array_equal(host(g)[:, 0, 5, :], np.zeros((5, iw), np.float32))     # the unread row gets an exact zero


def test_inpainting_requires_mask():
    from dps_ttc_amd.measurements import get_operator
    op = get_operator("inpainting", device=DEV)
    with pytest.raises(ValueError, match="Require mask"):
        op.forward(torch.zeros(1, 3, 8, 8, device=DEV))


def test_operator_refuses_cpu_tensors():
    from dps_ttc_amd.measurements import get_operator
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.forward(torch.zeros(1, 3, 64, 64))


# ----------------------------------------------------------------- full-size properties (N = 64, 256 x 256)
@pytest.mark.parametrize("name", ["gauss", "motion", "sr4", "phase"])
def test_full_size_properties(K, name):
    """BASELINE sizes: <A x, u> == <x, A^T u> (VJP identity), linearity of A, and the fused score equals
    ||y - A x|| computed from the materialised forward."""
    n = 64 if name != "phase" else 8
    gen = torch.Generator(device=DEV).manual_seed(5)
    op, fkw = make_product_op(name, hw=256, kernel=synthetic_motion_kernel(61, 2))
    x = torch.randn(n, 3, 256, 256, device=DEV, generator=gen).requires_grad_()
    y = op.forward(x, **fkw)
    u = torch.randn(y.shape, device=DEV, generator=gen)
    (g,) = torch.autograd.grad((y * u).sum(), x)
    lhs = (y.double() * u.double()).sum().item()
    rhs = (x.detach().double() * g.double()).sum().item()
    if name != "phase":        # <A x, u> = <x, A^T u>; for the modulus only Euler homogeneity <x, J^T u> = <A x, u>
        assert abs(lhs - rhs) <= 2e-5 * max(abs(lhs), np.sqrt(float(y.numel())))
        x2 = torch.randn(n, 3, 256, 256, device=DEV, generator=gen)
        lin = op.forward(2.0 * x.detach() - 0.5 * x2, **fkw)
        assert rel_l2(host(lin), host(2.0 * y.detach() - 0.5 * op.forward(x2, **fkw))) < TOL
    else:
        assert abs(lhs - rhs) <= 2e-5 * max(abs(lhs), np.sqrt(float(y.numel())))
    meas = torch.randn(1, *y.shape[1:], device=DEV, generator=gen)
    handle = op.hip_handle(x)
    costs = handle.score(x.detach(), meas)
    ref = torch.linalg.norm((meas - y.detach()).reshape(n, -1).double(), dim=-1)
    assert rel_l2(host(costs), ref.cpu().numpy()) < TOL


# ----------------------------------------------------------------- residual norm
def test_residual_norm_and_vjp(K, oracle):
    rng = np.random.RandomState(4)
    ax = rng.randn(5, 3, 20, 24).astype(np.float32)
    ax[3] = 0
    for y in (rng.randn(1, 3, 20, 24).astype(np.float32), rng.randn(5, 3, 20, 24).astype(np.float32)):
        if y.shape[0] == 5:
            y[3] = 0                       # zero residual -> norm 0 -> zero gradient (torch's convention)
        r, nrm = K.residual_norm(dev(y), dev(ax))
        ro, no = oracle.residual_norm(y, ax)
        np.testing.assert_array_equal(host(r), ro)
        assert rel_l2(host(nrm), no) < 1e-6
        gn = rng.rand(5).astype(np.float32)
        for power in (1, 2):
            assert rel_l2(host(K.norm_bwd(r, nrm, dev(gn), power)), oracle.norm_bwd(ro, no, gn, power)) < 1e-6


# ----------------------------------------------------------------- fused DPS step vs oracle
def _fused_case(K, oracle, name, n, hw, t, scale, power, seed, kernel=None, mask=None, finalize=False, ddim_eta=None,
                extra=False, per_particle_y=False, chw=None):
    """chw: (C, H, W) where the image is not 3 x hw x hw"""
    ch, ih, iw = chw if chw is not None else (3, hw, hw)
    rng = np.random.RandomState(seed)
    sched = oracle.tables.schedule(1000)
    c, ck = coefs_of(K, oracle, t, sched) if ddim_eta is None else ddim_coefs_of(K, oracle, t, ddim_eta, sched)
    op, fkw = make_product_op(name, hw=hw, kernel=kernel, mask=mask)
    orc = make_oracle_op(oracle, name, hw=hw, kernel=kernel, mask=mask)
    x_prev = rng.randn(n, ch, ih, iw).astype(np.float32)
    target = 1.4 * np.tanh(rng.randn(n, ch, ih, iw))
    eps = ((c["a"] * x_prev - target) / c["b"]).astype(np.float32)
    mo = np.concatenate([eps, rng.uniform(-1, 1, eps.shape).astype(np.float32)], axis=1)
    noise = rng.randn(n, ch, ih, iw).astype(np.float32)
    truth = rng.uniform(-1, 1, (1, ch, ih, iw)).astype(np.float32)
    y = orc.forward(truth)
    if per_particle_y:          # one measurement per particle ([N, ...] instead of the broadcast [1, ...])
        y = np.repeat(y, n, axis=0)
    y = (y + 0.05 * rng.randn(*y.shape)).astype(np.float32)
    g_unet = (1e-2 * rng.randn(n, ch, ih, iw)).astype(np.float32)
    g_extra = (0.05 * rng.randn(n, ch, ih, iw)).astype(np.float32) if extra else None
    ref = oracle.dps_step(orc, x_prev, mo, noise, y, c, scale=scale, power=power, g_unet_fn=lambda g: g_unet,
                          g_x0_extra=g_extra)
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(dev(x_prev))
    buf = K.StepBuffers(handle, n, ch, ih, iw, DEV)
    K.step_fwd(handle, buf, dev(x_prev), dev(mo), dev(noise), dev(y), ck, finalize_norm=finalize)
    if finalize:        # norms already final after K1 (the stand-alone finalisation kernel)
        assert rel_l2(host(buf.norm), ref["norm"]) < TOL
    K.step_bwd(handle, buf, dev(y), scale, power, ck, g_x0_extra=None if g_extra is None else dev(g_extra))
    x_next = K.step_update(buf, dev(g_unet), ck)
    np.testing.assert_array_equal(host(buf.x0_hat), ref["x0_hat"])
    np.testing.assert_array_equal(buf.inside.cpu().numpy(), ref["inside"])
    assert rel_l2(host(buf.sample), ref["sample"]) < 1e-6
    assert rel_l2(host(buf.norm), ref["norm"]) < TOL
    assert rel_l2(host(buf.g_model_out), ref["g_model_out"]) < TOL
    assert np.all(host(buf.g_model_out)[:, ch:] == 0)
    assert rel_l2(host(x_next) - ref["sample"], ref["x_next"] - ref["sample"]) < TOL      # the update itself
    assert rel_l2(host(x_next), ref["x_next"]) < 1e-6
    if name == "inpaint":      # gradient support = mask AND clamp gate, bit-exact pattern
        pat = (host(buf.g_model_out)[:, :ch] != 0)
        expect = (ref["g_model_out"][:, :ch] != 0)
        np.testing.assert_array_equal(pat, expect)


@pytest.mark.parametrize("name,hw", [("gauss", 64), ("gauss", 128), ("motion", 64), ("sr4", 64), ("sr4", 128),
                                     ("inpaint", 64), ("phase", 32), ("gauss", 46)])
@pytest.mark.parametrize("t,power", [(900, 1), (400, 2), (0, 1)])
def test_fused_step_vs_oracle(K, oracle, golden, name, hw, t, power):
    g = golden("operators")
    mask = (np.random.RandomState(7).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    _fused_case(K, oracle, name, 3, hw, t, 0.7, power, seed=hw + t, kernel=g["motion.kernel"], mask=mask)


@pytest.mark.parametrize("name,hw", [("gauss", 64), ("sr4", 64), ("inpaint", 64), ("motion", 64), ("phase", 32)])
@pytest.mark.parametrize("t,eta", [(900, 0.0), (400, 0.7), (0, 0.0)])
def test_fused_step_ddim_vs_oracle(K, oracle, golden, name, hw, t, eta):
    """the same three launches with the DDIM variant of S1 (scope row f2)"""
    g = golden("operators")
    mask = (np.random.RandomState(7).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    _fused_case(K, oracle, name, 3, hw, t, 0.7, 1, seed=hw + t + 1, kernel=g["motion.kernel"], mask=mask, ddim_eta=eta)


@pytest.mark.parametrize("name,hw", [("gauss", 64), ("gauss", 46), ("motion", 64), ("sr4", 64), ("sr4", 36), ("inpaint", 64),
                                     ("phase", 32)])
def test_fused_step_extra_cotangent_vs_oracle(K, oracle, golden, name, hw):
    """dpsx_step_bwd_extra_f32: a further cotangent on x0_hat (the semantic term's) joins coef * A^T r before the gate"""
    g = golden("operators")
    mask = (np.random.RandomState(7).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    _fused_case(K, oracle, name, 3, hw, 600, 0.7, 1, seed=hw + 3, kernel=g["motion.kernel"], mask=mask, extra=True)
    _fused_case(K, oracle, name, 2, hw, 0, 0.4, 2, seed=hw + 4, kernel=g["motion.kernel"], mask=mask, extra=True,
                finalize=True)


class _ToyEmbedder(torch.nn.Module):
    """Stand-in for the face-embedding network (the reference's InceptionResnetV1 weights are not available
    offline): a fixed random conv + pooling, differentiable, batch-independent."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(9)
        self.w = torch.nn.Parameter(torch.randn(8, 3, 5, 5, generator=g) * 0.2, requires_grad=False)

    def forward(self, x):
        h = torch.nn.functional.conv2d(x, self.w, stride=2, padding=2)
        return torch.tanh(h).mean(dim=(2, 3)) * 4.0


@pytest.mark.parametrize("oname", ["gauss", "motion", "sr4", "inpaint"])
def test_semantic_guidance_fused_matches_per_op(K, golden, oname):
    """ps_semantic with an ACTIVE semantic term (pluggable embedder; parity with the reference's networks is unpinned):
    the fused route (embedder VJP -> dpsx_step_bwd_extra_f32) and the per-op autograd route give the same loop."""
    import functools
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    g, gops = golden("loop"), golden("operators")
    op, fkw = make_product_op(oname, hw=64, kernel=gops["motion.kernel"], mask=gops["inpaint.mask"])
    emb = _ToyEmbedder().to(DEV)
    ref_emb = emb(dev(g["gauss.r20.x_start"][:1]).tanh()).unsqueeze(0)
    res = []
    for fused in (True, False):
        cm = get_conditioning_method("ps_semantic", op, get_noise("gaussian", sigma=0.05), scale=0.5,
                                     sem_guid_scale=0.3, anneal_factor=4.0, norm_exp=2, embedder=emb,
                                     guid_image_emb=ref_emb, guid_images=[0])
        smp = _sampler("ddpm", "20")
        if fused:
            cond = functools.partial(cm.conditioning, **fkw) if fkw else cm.conditioning
        else:
            cond = lambda **kw: cm.conditioning(**kw, **fkw)          # foreign callable -> per-op autograd path
        assert (smp._fusion_plan(cond, dev(g["gauss.r20.x_start"])) is not None) == fused
        torch.manual_seed(3)
        y = op.forward(dev(g["gauss.r20.x_start"][:1]).tanh(), **fkw).detach().contiguous()
        img, dist, sem = smp.p_sample_loop(model=StandInModel().to(DEV), x_start=dev(g["gauss.r20.x_start"]).requires_grad_(),
                                           measurement=y, measurement_cond_fn=cond, record=False, save_root=None)
        res.append((host(img), host(dist), host(sem)))
    assert res[0][2].shape == (4,) and np.all(res[0][2] > 0)
    assert rel_l2(res[0][0], res[1][0]) < 1e-4
    assert rel_l2(res[0][1], res[1][1]) < 1e-4 and rel_l2(res[0][2], res[1][2]) < 1e-4


@pytest.mark.parametrize("t,power,extra", [(700, 1, False), (300, 2, True), (0, 1, False)])
def test_phase_spectral_step_full_size(K, oracle, t, power, extra):
    """256 x 256, oversample 2.0 takes the hand-written three-pass spectral step (csrc/phase_fft.h: row FFTs fused with
    S1, column FFT + pointwise + inverse in LDS, row inverse fused with the gate epilogue) instead of the library
    transforms: same gates as every other fused step, against the oracle's numpy-free C DFT path."""
    _fused_case(K, oracle, "phase", 2, 256, t, 0.6, power, seed=40 + t, extra=extra)
    _fused_case(K, oracle, "phase", 1, 256, t, 0.6, power, seed=41 + t, extra=extra, finalize=True)


@pytest.mark.parametrize("name,hw", [("gauss", 128), ("motion", 64), ("sr4", 64), ("inpaint", 64), ("phase", 32), ("phase", 256),
                                     ("denoise", 17)])
def test_fused_step_per_particle_measurement(K, golden, name, hw):
    """y given once ([1, ...], broadcast) or per particle ([N, ...]): the same launches, bit-identical results"""
    g = golden("operators")
    rng = np.random.RandomState(hw)
    n = 3
    mask = (np.random.RandomState(7).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=g["motion.kernel"], mask=mask)
    x = dev(rng.randn(n, 3, hw, hw).astype(np.float32))
    mo = dev(rng.randn(n, 6, hw, hw).astype(np.float32) * 0.4)
    z = dev(rng.randn(n, 3, hw, hw).astype(np.float32))
    y1 = op.forward(dev(rng.uniform(-1, 1, (1, 3, hw, hw)).astype(np.float32)), **fkw).detach().contiguous()
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(x)
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    ck = _sampler("ddpm", "").step_coefs[400]
    out = []
    for y in (y1, y1.expand(n, *y1.shape[1:]).contiguous()):
        buf = K.StepBuffers(handle, n, 3, hw, hw, DEV)
        K.step_fwd(handle, buf, x, mo, z, y, ck)
        K.step_bwd(handle, buf, y, 0.5, 1, ck)
        out.append((buf.norm.clone(), buf.g_model_out.clone(), buf.x0_hat.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert float(out[0][1].abs().max()) > 0


@pytest.mark.parametrize("name,hw", [("gauss", 128), ("sr4", 64), ("inpaint", 64), ("motion", 64), ("denoise", 64)])
def test_fused_step_is_graph_capturable(K, golden, name, hw):
    """The three launches allocate nothing and never synchronise: captured once in a HIP graph on a
    side stream and replayed on new inputs, they give the eager results bit for bit."""
    g = golden("operators")
    rng = np.random.RandomState(hw + 1)
    n = 4
    mask = (np.random.RandomState(7).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=g["motion.kernel"], mask=mask)
    mk = lambda *shape: dev(rng.randn(*shape).astype(np.float32))
    x, mo, z, gu = mk(n, 3, hw, hw), mk(n, 6, hw, hw) * 0.4, mk(n, 3, hw, hw), mk(n, 3, hw, hw) * 1e-2
    y = op.forward(dev(rng.uniform(-1, 1, (1, 3, hw, hw)).astype(np.float32)), **fkw).detach().contiguous()
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(x)
    ck = _sampler("ddpm", "").step_coefs[300]
    buf = K.StepBuffers(handle, n, 3, hw, hw, DEV)

    def step():
        K.step_fwd(handle, buf, x, mo, z, y, ck)
        K.step_bwd(handle, buf, y, 0.5, 1, ck)
        return K.step_update(buf, gu, ck)

    ref = step().clone()                       # eager (also the warm-up: kernel attributes, workspace)
    ref_norm = buf.norm.clone()
    step()                                     # leave the ping-pong output index where the capture will start
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = step()
    torch.cuda.current_stream().wait_stream(side)
    buf.norm.fill_(-1.0)
    out.fill_(0.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and torch.equal(buf.norm, ref_norm)
    x.mul_(0.5)                                # new inputs in the same buffers, same graph
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out, ref)
    replayed = out.clone()
    assert torch.equal(step(), replayed)       # eager on the new inputs


@pytest.mark.parametrize("name", ["gauss", "sr4", "sr8", "inpaint", "motion"])
@pytest.mark.parametrize("t,power,finalize", [(500, 1, False), (0, 2, True), (500, 2, True), (0, 1, False)])
def test_fused_step_full_size(K, oracle, name, t, power, finalize):
    """The launches the BASELINE configs run -- every operator at 256 x 256 (Gaussian 64x64-tile kernel, the wu = 64
    row-streaming POST,RESID resize kernel for x4 and x8, the 256^2 tap-list and mask kernels) -- against the oracle on
    a particle subset it finishes fast: both norm-finalisation modes, t in {500, 0}, power in {1, 2}.
    (reference: resizer.py:55-74, measurements.py:84,108,142,158; phase retrieval at 256^2: test_phase_spectral_step_full_size)"""
    mask = (np.random.RandomState(3).rand(1, 1, 256, 256) < 0.5).astype(np.float32)
    _fused_case(K, oracle, name, 2, 256, t, 0.3 if power == 1 else 0.05, power, seed=11 + t + power, finalize=finalize,
                kernel=synthetic_motion_kernel(61, 4), mask=mask)


@pytest.mark.parametrize("name", ["sr4", "sr8", "gauss", "motion", "inpaint"])
def test_fused_step_full_size_per_particle_measurement(K, oracle, name):
    """256 x 256 with one measurement per particle (y [N, ...]) against the oracle"""
    mask = (np.random.RandomState(5).rand(1, 1, 256, 256) < 0.5).astype(np.float32)
    _fused_case(K, oracle, name, 3, 256, 300, 0.4, 1, seed=77, kernel=synthetic_motion_kernel(61, 6), mask=mask,
                per_particle_y=True)
    _fused_case(K, oracle, name, 2, 256, 700, 0.4, 1, seed=78, kernel=synthetic_motion_kernel(61, 6), mask=mask,
                per_particle_y=True, extra=True, finalize=True)


@pytest.mark.parametrize("name,n", [("gauss", 512), ("phase", 512), ("motion", 256), ("sr4", 64), ("sr8", 64), ("inpaint", 64)])
def test_fused_step_full_batch_is_batch_independent(K, name, n):
    """BASELINE's full particle counts (configs[2]: 64, configs[3]: 256, configs[4]: 512 -- here on ONE GPU, the
    largest shard any configuration can hand a rank) through the size-independent property the domain offers: particles
    are independent, so particle i of the N-particle launches equals, BIT FOR BIT, the same particle run alone or in a
    small batch (x_{t-1}, norm, sample and clamp gate).  The small batches are what `test_fused_step_full_size` pins
    against the oracle; this test carries that pin to the large grids (plane offsets beyond 2^31 bytes, thousands of
    workgroups per launch, several generations of tiles)."""
    hw = 256
    gen = torch.Generator(device=DEV).manual_seed(100 + n)
    mk = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)
    mask = (np.random.RandomState(9).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=synthetic_motion_kernel(61, 4), mask=mask)
    x, mo, z, gu = mk(n, 3, hw, hw), mk(n, 6, hw, hw) * 0.4, mk(n, 3, hw, hw), mk(n, 3, hw, hw) * 1e-2
    y = op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1, **fkw).detach().contiguous()
    ck = _sampler("ddpm", "").step_coefs[400]

    def run(sl):
        xs, ms, zs, gs = (t[sl].contiguous() for t in (x, mo, z, gu))
        k = xs.shape[0]
        handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(xs)
        buf = K.StepBuffers(handle, k, 3, hw, hw, DEV)
        K.step_fwd(handle, buf, xs, ms, zs, y, ck)
        K.step_bwd(handle, buf, y, 0.3, 1, ck)
        out = K.step_update(buf, gs, ck)
        return out.clone(), buf.norm.clone(), buf.sample.clone(), buf.inside.clone()

    full = run(slice(0, n))
    assert bool(torch.isfinite(full[0]).all()) and bool((full[1] > 0).all())
    for sl in (slice(0, 1), slice(n - 1, n), slice(n // 2 - 1, n // 2 + 2), slice(n - 5, n)):
        part = run(sl)
        for a, b, what in zip(full, part, ("x_prev", "norm", "sample", "gate")):
            assert torch.equal(a[sl], b), f"{name} N={n}: {what} of particles {sl} depends on the batch"


# ----------------------------------------------------------------- conditioning per call (registry API, autograd path)
@pytest.mark.parametrize("oname", ["gauss", "motion", "sr4", "inpaint", "phase"])
@pytest.mark.parametrize("t", [900, 500, 0])
def test_conditioning_per_call_golden(K, golden, oname, t):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    from dps_ttc_amd.measurements import get_noise
    g, gops = golden("conditioning"), golden("operators")
    op, fkw = make_product_op(oname, hw=32, kernel=gops["motion.kernel"], mask=g["inpaint.mask"])
    noiser = get_noise("gaussian", sigma=0.05)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    model = StandInModel().to(DEV)
    y = dev(g[f"{oname}.y"])
    for method, params in (("ps", {"scale": 0.3}), ("ps_semantic", {"scale": 0.7, "sem_guid_scale": 0.0}),
                           ("ps_anneal", {"scale": 0.3})):
        cm = get_conditioning_method(method, op, noiser, **params)
        x_prev = dev(g[f"{oname}.t{t}.x_prev"]).requires_grad_()
        out = smp.p_sample(model=model, x=x_prev, t=torch.tensor([t]), noise=dev(g[f"{oname}.t{t}.noise"]))
        np.testing.assert_array_equal(host(out["pred_xstart"]), g[f"{oname}.t{t}.x0_hat"])
        assert rel_l2(host(out["sample"]), g[f"{oname}.t{t}.sample"]) < 1e-6
        ret = cm.conditioning(x_prev=x_prev, x_t=out["sample"], x_0_hat=out["pred_xstart"], measurement=y,
                              noisy_measurement=y, beta_scale=float(smp.betas[t]), t=t / 1000.0, **fkw)
        assert rel_l2(host(ret[1]), g[f"{oname}.t{t}.{method}.ret1"]) < TOL, method
        tol0 = 2e-5 if method == "ps_semantic" else TOL
        assert rel_l2(host(ret[0]), g[f"{oname}.t{t}.{method}.ret0"]) < tol0, method
        assert rel_l2(host(torch.as_tensor(ret[2])), g[f"{oname}.t{t}.{method}.ret2"]) < TOL, method


# ----------------------------------------------------------------- free-running loops vs the reference
def _sampler(name, respacing):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    s = create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                       model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                       rescale_timesteps=True, timestep_respacing=respacing)
    s.rng_parity = True
    return s


LOOPS = [("gauss.r20", "gauss", "20", 0.5, 1), ("sr4.r20", "sr4", "20", 1.0, 1), ("inpaint.r20", "inpaint", "20", 0.5, 1),
         ("motion.r20", "motion", "20", 0.5, 2), ("sr4.full1000", "sr4", "", 1.0, 1)]


@pytest.mark.parametrize("tag,oname,resp,scale,norm_exp", LOOPS)
@pytest.mark.parametrize("fused", [True, False])
def test_base_loop_golden(K, golden, tag, oname, resp, scale, norm_exp, fused):
    """Whole p_sample_loop (ps_semantic, sem_guid_scale=0) with the stand-in UNet, same host RNG stream as the
    reference run: final image within 1e-4 rel-L2 (BASELINE gate), per-step norms within 1e-4."""
    import functools
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    if not fused and tag == "sr4.full1000":
        pytest.skip("1000 steps once (fused) is enough")
    g, gops, gc = golden("loop"), golden("operators"), golden("operators")
    op, fkw = make_product_op(oname, hw=64, kernel=gops["motion.kernel"], mask=gc["inpaint.mask"])
    cm = get_conditioning_method("ps_semantic", op, get_noise("gaussian", sigma=0.05), scale=scale,
                                 sem_guid_scale=0.0, norm_exp=norm_exp)
    smp = _sampler("ddpm", resp)
    norms = []
    if fused:
        cond = functools.partial(cm.conditioning, **fkw) if fkw else cm.conditioning
        orig = smp.dps_step

        def spy(*a, **k):
            r = orig(*a, **k)
            norms.append(host(r[1]).copy())
            return r
        smp.dps_step = spy
    else:
        def cond(**kw):                      # a foreign callable: forces the per-op autograd path
            r = cm.conditioning(**kw, **fkw)
            norms.append(host(r[1]).copy())
            return r
    model = StandInModel().to(DEV)
    smp.parity_measurement_stride = tuple(int(v) for v in g[f"{tag}.y_stride"])
    torch.manual_seed(int(g[f"{tag}.rng_seed"]))
    img, dist, sem = smp.p_sample_loop(model=model, x_start=dev(g[f"{tag}.x_start"]).requires_grad_(),
                                       measurement=dev(g[f"{tag}.y"]), measurement_cond_fn=cond, record=False,
                                       save_root=None)
    assert (smp._fusion_plan(cond, img) is not None) == fused
    assert rel_l2(np.stack(norms), g[f"{tag}.norms"]) < 1e-4
    assert rel_l2(host(img), g[f"{tag}.final"]) < 1e-4
    assert rel_l2(host(dist), g[f"{tag}.norms"][-1]) < 1e-4


@pytest.mark.parametrize("tag,resp,scale", [("gauss.r20", "20", 0.5), ("gauss.r50", "ddim50", 0.3)])
def test_ttc_ddim_loop_golden(K, golden, tag, resp, scale):
    """ttc_ddim (reference gaussian_diffusion.py:644-707) with 'mcg', the shipped method whose two return values
    fit the loop: DDIM S1 in HIP, per-op HIP operator calls under autograd, multinomial resampling on the replayed
    host RNG stream, HIP gather.  Resampled ids bit-exact; images and norms within the 1e-4 gate."""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    g = golden("ddim")
    op, _ = make_product_op("gauss", hw=64)
    cm = get_conditioning_method("mcg", op, get_noise("gaussian", sigma=0.05), scale=scale)
    smp = _sampler("ttc_ddim", resp)
    norms, picks = [], []

    def cond(**kw):
        r = cm.conditioning(**kw)
        norms.append(host(r[1]).copy())
        return r
    orig = K.gather

    def spy(x, ids, **kw):
        if x.dim() == 4:                     # the particle gather (the distances are gathered with the same ids)
            picks.append(ids.cpu().numpy().copy())
        return orig(x, ids, **kw)
    K.gather = spy
    try:
        torch.manual_seed(int(g[f"{tag}.rng_seed"]))
        img, dist = smp.p_sample_loop(model=StandInModel().to(DEV), x_start=dev(g[f"{tag}.x_start"]).requires_grad_(),
                                      measurement=dev(g[f"{tag}.y"]), measurement_cond_fn=cond, record=False,
                                      save_root=None)
    finally:
        K.gather = orig
    np.testing.assert_array_equal(np.stack(picks), g[f"{tag}.resample_ids"])
    assert rel_l2(np.stack(norms), g[f"{tag}.norms"]) < 1e-4
    assert rel_l2(host(img), g[f"{tag}.final"]) < 1e-4
    assert rel_l2(host(dist), g[f"{tag}.distance"]) < 1e-4


def test_ttc_ddim_fused_matches_per_op(K, golden):
    """'ps' under ttc_ddim (the reference's own loop cannot unpack its three return values): the fused three-launch
    DDIM step and the per-op autograd path are two HIP routes to the same numbers."""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    g = golden("ddim")
    op, _ = make_product_op("gauss", hw=64)
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.5)
    res = []
    for fused in (True, False):
        smp = _sampler("ttc_ddim", "20")
        cond = cm.conditioning if fused else (lambda **kw: cm.conditioning(**kw))
        assert (smp._fusion_plan(cond, dev(g["gauss.r20.x_start"])) is not None) == fused
        torch.manual_seed(5)
        img, dist = smp.p_sample_loop(model=StandInModel().to(DEV), x_start=dev(g["gauss.r20.x_start"]).requires_grad_(),
                                      measurement=dev(g["gauss.r20.y"]), measurement_cond_fn=cond, record=False,
                                      save_root=None)
        res.append((host(img), host(dist), smp.last_resample_ids.cpu().numpy()))
    np.testing.assert_array_equal(res[0][2], res[1][2])
    assert rel_l2(res[0][0], res[1][0]) < 1e-5 and rel_l2(res[0][1], res[1][1]) < 1e-5


@pytest.mark.parametrize("tag", ["gauss.n1.p5", "gauss.n2.p4"])
def test_base_loop_diffstategrad_golden(K, golden, tag):
    """base loop with project=True (reference gaussian_diffusion.py:203-204, 240-251): fused launches on ordinary
    steps, per-op path + rocSOLVER SVD projection every `period` steps; final image within the 1e-4 gate"""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    g = golden("project")
    op, _ = make_product_op("gauss", hw=64)
    cm = get_conditioning_method("ps_semantic", op, get_noise("gaussian", sigma=0.05), scale=0.5, sem_guid_scale=0.0)
    smp = _sampler("ddpm", "20")
    torch.manual_seed(int(g[f"{tag}.rng_seed"]))
    img, dist, _ = smp.p_sample_loop(model=StandInModel().to(DEV), x_start=dev(g[f"{tag}.x_start"]).requires_grad_(),
                                     measurement=dev(g[f"{tag}.y"]), measurement_cond_fn=cm.conditioning, record=False,
                                     save_root=None, project=True, period=int(g[f"{tag}.period"]))
    assert rel_l2(host(img), g[f"{tag}.final"]) < 1e-4
    assert rel_l2(host(dist), g[f"{tag}.distance"]) < 1e-4


@pytest.mark.parametrize("tag,oname", [("sr4", "sr4"), ("gauss", "gauss")])
@pytest.mark.parametrize("single", [True, False])
def test_search_ddpm_golden(K, golden, tag, oname, single):
    """per-step best-of-N: winner indices bit-exact, costs and final image within 1e-5 / 1e-4 -- with the loop's state
    held as one particle after the first select (the default) and as N copies (the reference's form)"""
    g = golden("search")
    op, _ = make_product_op(oname, hw=64)
    smp = _sampler("search_ddpm", "20")
    smp.single_state = single
    model = StandInModel().to(DEV)
    best, calls = [], {"n": 0, "one": 0}

    def spy_on(name):                      # the select is fused into the scoring launch: read its device-side index
        orig = getattr(smp, name)

        def spy(*a, **kw):
            r = orig(*a, **kw)
            best.append(int(smp.last_best))
            calls["one" if name == "search_step_one" else "n"] += 1
            return r
        setattr(smp, name, spy)
    spy_on("search_step")
    spy_on("search_step_one")
    torch.manual_seed(int(g[f"{tag}.rng_seed"]))
    img = smp.p_sample_loop(model=model, x_start=dev(g[f"{tag}.x_start"]), measurement=dev(g[f"{tag}.y"]),
                            measurement_cond_fn=None, record=False, save_root=None, operator=op, trace=True)
    np.testing.assert_array_equal(np.array(best), g[f"{tag}.best"])
    costs = np.array([host(c)[b] for c, b in zip(smp.best_costs, best)])
    assert rel_l2(costs, g[f"{tag}.cost"]) < 1e-5
    assert rel_l2(host(img), g[f"{tag}.final"]) < 1e-4
    assert img.shape == (5, 3, 64, 64) and torch.equal(img[0], img[4])
    assert calls == ({"n": 1, "one": 19} if single else {"n": 20, "one": 0})


def test_ttc_driver_call_returns_bare_tensor(K, golden):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    g = golden("loop")
    op, _ = make_product_op("sr4", hw=64)
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=1.0)
    smp = _sampler("ddpm", "20")
    smp.parity_measurement_stride = tuple(int(v) for v in g["sr4.r20.y_stride"])
    torch.manual_seed(int(g["sr4.r20.rng_seed"]))
    out = smp.p_sample_loop(model=StandInModel().to(DEV), x_start=dev(g["sr4.r20.x_start"]).requires_grad_(),
                            measurement=dev(g["sr4.r20.y"]), measurement_cond_fn=cm.conditioning, record=False,
                            save_root=None, operator=op, resample_every_steps=10, potential_type="curr",
                            rs_temp=0.1, anneal_scale=10, anneal_loc=0.5, anneal_amp=1)
    assert isinstance(out, torch.Tensor) and out.shape == (4, 3, 64, 64)
    # 'ps' with scale s equals 'ps_semantic' with scale s and no semantic term: same fixture
    assert rel_l2(host(out), g["sr4.r20.final"]) < 1e-4


# ----------------------------------------------------------------- select
def test_argmin_gather_replicate(K, oracle, golden):
    v = torch.tensor([3.0, 1.0, 1.0, 7.0], device=DEV)
    assert int(K.argmin(v)) == 1
    v2 = v.clone()
    v2[2] = float("nan")
    assert int(K.argmin(v2)) == 2 == oracle.argmin(host(v2))
    big = torch.rand(5000, device=DEV)
    big[4097] = -1.0
    big[4999] = -1.0
    assert int(K.argmin(big)) == 4097 == int(torch.argmin(big))
    nn = torch.full((300,), float("nan"), device=DEV)
    assert int(K.argmin(nn)) == 0
    v3 = torch.rand(300, device=DEV)
    v3[[77, 200, 299]] = float("nan")
    assert int(K.argmin(v3)) == 77                                # first NaN wins, as torch.argmin
    assert int(K.argmin(torch.tensor([5.0], device=DEV))) == 0
    for n in (2, 63, 64, 65, 256, 257, 1000):
        r = torch.randn(n, device=DEV).round(decimals=1)          # plenty of ties
        assert int(K.argmin(r)) == int(torch.argmin(r))
    src = torch.randn(6, 3, 10, 7, device=DEV)                   # chw not a multiple of 4 -> scalar kernel
    ids = torch.tensor([5, 5, 0, 3], device=DEV)
    assert torch.equal(K.gather(src, ids), src[ids])
    src4 = torch.randn(6, 3, 8, 8, device=DEV)
    assert torch.equal(K.gather(src4, ids), src4[ids])
    assert K.gather(src4, ids[:0]).shape == (0, 3, 8, 8)
    assert torch.equal(K.replicate(src4, torch.tensor(2, device=DEV)), src4[2:3].repeat(6, 1, 1, 1))
    with pytest.raises(IndexError):
        K.gather(src4, torch.tensor([6], device=DEV))                  # the public default validates (torch's IndexError)
    with pytest.raises(IndexError):
        K.gather(src4, torch.tensor([-1], device=DEV))
    bad = K.gather(src4, torch.tensor([1, 6, -1], device=DEV), validate=False)   # the loops' own ids: no host check; a bad id poisons its particle only
    assert torch.equal(bad[0], src4[1]) and bool(torch.isnan(bad[1:]).all())
    idx, val = K.argmin(v, want_value=True)
    assert int(idx) == 1 and val.shape == (1,) and float(val) == 1.0
    g = golden("search")
    w = torch.exp(-torch.from_numpy(g["resample.dist"]) / 100.0)
    torch.manual_seed(int(g["resample.seed"]))
    ids = torch.multinomial(w, 8, replacement=True)
    np.testing.assert_array_equal(ids.numpy(), g["resample.ids"])


def test_pack_and_select_champion(K):
    """The two launches around the champion all-gather (distributed._champion_table / GlobalSelect on the device) against
    their torch restatement: record = [particles[argmin] | cost, index, 0, 0]; select = first minimum over the records'
    costs (lowest rank wins ties, NaN counts as the minimum), n_out copies, winner rank and local index on the device."""
    torch.manual_seed(5)
    for n, shape in ((1, (3, 8, 8)), (7, (3, 16, 12)), (64, (3, 64, 64)), (300, (1, 4, 4))):
        x = torch.randn((n,) + shape, device=DEV)
        c = torch.randn(n, device=DEV).round(decimals=1)
        chw = x[0].numel()
        rec = K.pack_champion(x, c)
        b = int(torch.argmin(c))
        assert rec.shape == (chw + 4,)
        assert torch.equal(rec[:chw], x[b].reshape(-1)) and float(rec[chw]) == float(c[b]) and int(rec[chw + 1]) == b
        assert float(rec[chw + 2]) == 0.0 and float(rec[chw + 3]) == 0.0
        # the select already done by the caller (index [+ value] on the device)
        rec2 = K.pack_champion(x, c, best=torch.tensor(n - 1, device=DEV))
        assert torch.equal(rec2[:chw], x[n - 1].reshape(-1)) and float(rec2[chw]) == float(c[n - 1]) and int(rec2[chw + 1]) == n - 1
        rec3 = K.pack_champion(x, None, best=torch.tensor(0, device=DEV), best_val=torch.tensor([2.5], device=DEV))
        assert torch.equal(rec3[:chw], x[0].reshape(-1)) and float(rec3[chw]) == 2.5
    cn = torch.tensor([3.0, float("nan"), 1.0, float("nan")], device=DEV)
    xs = torch.randn(4, 3, 8, 8, device=DEV)
    assert int(K.pack_champion(xs, cn)[3 * 64 + 1]) == 1                      # first NaN wins, as torch.argmin
    # select over a gathered table
    for world, shape, n_out in ((1, (3, 8, 8), 1), (2, (3, 16, 12), 5), (8, (3, 64, 64), 64), (70, (1, 4, 4), 9)):
        chw = int(np.prod(shape))
        table = torch.randn(world, chw + 4, device=DEV)
        table[:, chw] = torch.randn(world, device=DEV).round(decimals=0)      # ties across ranks
        table[:, chw + 1] = torch.randint(0, 1000, (world,), device=DEV).float()
        w = int(torch.argmin(table[:, chw]))
        dst, wr, wl = K.select_champion(table, shape, n_out=n_out, want_index=True)
        assert int(wr) == w and int(wl) == int(table[w, chw + 1])
        assert torch.equal(dst, table[w, :chw].reshape((1,) + shape).repeat(n_out, 1, 1, 1))
        assert torch.equal(K.select_champion(table, shape, n_out=n_out), dst)
    table = torch.randn(3, 3 * 64 + 4, device=DEV)
    table[:, 192] = torch.tensor([float("inf"), float("nan"), -5.0])
    _, wr, _ = K.select_champion(table, (3, 8, 8), want_index=True)
    assert int(wr) == 1
    table[:, 192] = float("inf")                                              # all shards empty / all +inf: rank 0
    _, wr, _ = K.select_champion(table, (3, 8, 8), want_index=True)
    assert int(wr) == 0
    with pytest.raises(ValueError):
        K.select_champion(table, (3, 8, 9))


# ----------------------------------------------------------------- resample_update (reference :515-587) and fused selects
@pytest.mark.parametrize("tag,oname", [("gauss", "gauss"), ("sr4", "sr4")])
def test_resample_update_golden(K, golden, tag, oname):
    """SearchDDPM.resample_update against the reference's own outputs: multinomial ids bit-exact on the replayed host
    RNG stream, net costs within 1e-5, for every potential type x {first call, update, resample + update};
    gathers and the L1^2 / CHW cost + combine are HIP (dpsx_gather_f32, dpsx_resample_cost_f32)."""
    g = golden("resample")
    op, _ = make_product_op(oname, hw=64)
    smp = _sampler("search_ddpm", "20")
    cands, den, y, prev = dev(g[f"{tag}.candidates"]), dev(g[f"{tag}.denoised"]), dev(g[f"{tag}.y"]), dev(g[f"{tag}.prev_costs"])
    for pot in ("mean", "min", "diff", "curr"):
        cases = (("first", dict(prev_costs=None, resample=True)),
                 ("noresample", dict(prev_costs=prev.clone(), resample=False)),
                 ("resample", dict(prev_costs=prev.clone(), resample=True, rs_temp=0.05, steps_done=3)))
        for cname, kw in cases:
            torch.manual_seed(int(g[f"{tag}.rng_seed"]))
            c2, net = smp.resample_update(cands.clone(), den.clone(), op, y, potential_type=pot, **kw)
            np.testing.assert_array_equal(host(c2)[:, 0, 0, 0].round().astype(np.int64), g[f"{tag}.{pot}.{cname}.ids"])
            assert rel_l2(host(net), g[f"{tag}.{pot}.{cname}.net"]) < TOL, (pot, cname)
    # equal potentials: no draw, particles untouched (:545)
    c2, _ = smp.resample_update(cands.clone(), den.clone(), op, y, prev_costs=torch.full((6,), 7.0, device=DEV),
                                resample=True, potential_type="min")
    assert torch.equal(c2, cands)
    with pytest.raises(NotImplementedError):
        smp.resample_update(cands, den, op, y, potential_type="median")


@pytest.mark.parametrize("name,hw,n", [("gauss", 256, 5), ("motion", 256, 3), ("sr4", 256, 5), ("sr8", 256, 3),
                                       ("inpaint", 256, 4), ("phase", 256, 2), ("gauss", 46, 3), ("sr4", 36, 3),
                                       ("inpaint", 30, 3), ("denoise", 17, 3), ("phase", 34, 2), ("phase", 36, 2),
                                       ("inpaint", 63, 3), ("inpaint", (62, 63), 3)])
def test_resample_cost_vs_oracle(K, oracle, name, hw, n):
    """curr = ||y - A x||_1^2 / CHW and the four combines for every operator (full size and ragged), against the oracle;
    NaN in either cost propagates through 'min' as torch.min does"""
    ih, iw, hw = _pair(hw)
    rng = np.random.RandomState(hw + n)
    kernel = synthetic_motion_kernel(61, 5)
    mask = (np.random.RandomState(3).rand(1, 1, ih, iw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=kernel, mask=mask)
    orc = make_oracle_op(oracle, name, hw=hw, kernel=kernel, mask=mask)
    x = rng.uniform(-1, 1, (n, 3, ih, iw)).astype(np.float32)
    y = orc.forward(rng.uniform(-1, 1, (1, 3, ih, iw)).astype(np.float32))
    y = (y + 0.05 * rng.randn(*y.shape)).astype(np.float32)
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(dev(x))
    prev = (rng.rand(n) * 50).astype(np.float32)
    for pot in ("mean", "min", "diff", "curr"):
        for pv in (None, prev):
            curr, net = handle.resample_cost(dev(x), dev(y), None if pv is None else dev(pv), pot)
            oc, on = oracle.resample_cost(orc, x, y, pv, pot)
            assert rel_l2(host(curr), oc) < TOL and rel_l2(host(net), on) < TOL, (pot, pv is None)
    pn = prev.copy()
    pn[1] = np.nan
    _, net = handle.resample_cost(dev(x), dev(y), dev(pn), "min")
    assert np.isnan(host(net)[1]) and not np.isnan(host(net)[0])
    # per-particle measurements
    yn = np.repeat(y, n, axis=0) + 0.01 * rng.randn(n, *y.shape[1:]).astype(np.float32)
    curr, _ = handle.resample_cost(dev(x), dev(yn.astype(np.float32)), None, "curr")
    assert rel_l2(host(curr), oracle.resample_cost(orc, x, yn.astype(np.float32), None, "curr")[0]) < TOL


@pytest.mark.parametrize("name,hw,n", [("gauss", 256, 64), ("motion", 128, 9), ("sr4", 256, 64), ("inpaint", 256, 33),
                                       ("phase", 256, 3), ("gauss", 46, 7), ("sr4", 64, 300), ("denoise", 17, 7),
                                       ("phase", 34, 2), ("phase", 36, 2), ("inpaint", 63, 3), ("inpaint", (62, 63), 3)])
def test_score_argmin_fused(K, name, hw, n):
    """dpsx_score_argmin_f32: the scoring launch's own tail finishes the norms and the select -- same costs bit for bit
    as dpsx_score_f32, same index as torch.argmin (first minimum; NaN wins), repeatable (counters reset themselves)"""
    ih, iw, hw = _pair(hw)
    gen = torch.Generator(device=DEV).manual_seed(n)
    mask = (np.random.RandomState(3).rand(1, 1, ih, iw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=synthetic_motion_kernel(61, 5), mask=mask)
    x = torch.randn(n, 3, ih, iw, device=DEV, generator=gen)
    x[n // 2] = x[1]                                         # an exact tie: the first one must win
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(x)
    y = op.forward(x[1:2] * 0.9, **fkw).detach().contiguous()
    for rep in range(3):
        costs, best, val = handle.score_argmin(x, y)
        ref = handle.score(x, y)
        assert torch.equal(costs, ref)
        assert int(best) == int(torch.argmin(ref)) == 1 and float(val) == float(ref[1])
    xn = x.clone()
    xn[n - 1, 0, 3, 3] = float("nan")
    costs, best, val = handle.score_argmin(xn, y)
    assert int(best) == n - 1 and bool(torch.isnan(val).all())


def _norm_modes_bit_identical(K, name, hw, n, draw=None):
    """the body of test_step_fwd_norm_modes_bit_identical*.  draw: a kernels.Rng record -- the noise is drawn inside K1
    (the handle must have that form) instead of read from a tensor"""
    rng = np.random.RandomState(hw)
    mask = (np.random.RandomState(7).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=synthetic_motion_kernel(61, 5), mask=mask)
    x, mo, z = dev(rng.randn(n, 3, hw, hw).astype(np.float32)), dev(rng.randn(n, 6, hw, hw).astype(np.float32) * 0.4), \
        dev(rng.randn(n, 3, hw, hw).astype(np.float32))
    y = op.forward(dev(rng.uniform(-1, 1, (1, 3, hw, hw)).astype(np.float32)), **fkw).detach().contiguous()
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(x)
    noise = dict(noise=z)
    if draw is not None:
        assert handle.draws_in_kernel(3, hw, hw)
        noise = dict(rng=draw)
    ck = _sampler("ddpm", "").step_coefs[400]
    outs = []
    for finalize in (True, False, True, True):
        buf = K.StepBuffers(handle, n, 3, hw, hw, DEV)
        buf.norm.fill_(-1.0)
        K.step_fwd(handle, buf, x, mo, y=y, coefs=ck, finalize_norm=finalize, **noise)
        if finalize:
            first = buf.norm.clone()
            assert float(first.min()) > 0
        K.step_bwd(handle, buf, y, 0.5, 1, ck)
        if finalize:
            assert torch.equal(first, buf.norm)
        outs.append((buf.norm.clone(), buf.g_model_out.clone()))
    for a, b in outs[1:]:
        assert torch.equal(a, outs[0][0]) and torch.equal(b, outs[0][1])
    r = (y - op.forward(buf.x0_hat, **fkw)).reshape(n, -1)
    assert rel_l2(host(outs[0][0]), host(r.norm(dim=1))) < TOL


@pytest.mark.parametrize("name,hw", [("gauss", 256), ("motion", 128), ("sr4", 256), ("inpaint", 256), ("gauss", 46),
                                     ("denoise", 17)])
def test_step_fwd_norm_modes_bit_identical(K, name, hw):
    """K1 finishing the norm itself (last block of each particle) == the stand-alone finalisation kernel of r01 ==
    K2's prologue finalisation: the same bits, and repeatable over launches (self-resetting counters)"""
    _norm_modes_bit_identical(K, name, hw, 5)


@pytest.mark.parametrize("name,hw", [("gauss", 128), ("motion", 128), ("sr4", 256), ("inpaint", 64)])
def test_step_fwd_norm_modes_bit_identical_in_kernel_draw(K, name, hw):
    """the same with the noise drawn inside K1 (the RNG instantiations carry the in-launch norm too): the smallest
    whole-tile shapes with several arriving blocks per particle (128^2: 4 tiles x 3 planes)"""
    _norm_modes_bit_identical(K, name, hw, 3, draw=K.Rng(29, 400))


def test_step_fwd_norm_modes_bit_identical_coarse_blocking(K):
    """the same under the resize kernel's coarse blocking, where one block publishes several partials and arrives once:
    96 planes x out_h / tp workgroups is past the threshold up to which the launch takes the fine blocking (n = 5 above)"""
    _norm_modes_bit_identical(K, "sr4", 256, 32)


@pytest.mark.parametrize("name,hw,n", [("gauss", 256, 64), ("sr4", 256, 64), ("inpaint", 256, 64), ("motion", 128, 16),
                                       ("denoise", 64, 8)])
def test_in_launch_reduction_sees_fresh_partials(K, name, hw, n):
    """the tail of a launch re-reads partial sums other XCDs wrote a moment ago, in buffers earlier launches filled with
    other values: every launch of a sequence with CHANGING inputs must reproduce the norms of the materialised residual
    (a stale line would surface as the previous launch's value)"""
    gen = torch.Generator(device=DEV).manual_seed(hw + n)
    mask = (np.random.RandomState(7).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=synthetic_motion_kernel(61, 5), mask=mask)
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(torch.empty(n, 3, hw, hw, device=DEV))
    y = op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1, **fkw).detach().contiguous()
    ck = _sampler("ddpm", "").step_coefs[300]
    buf = K.StepBuffers(handle, n, 3, hw, hw, DEV)
    for it in range(6):
        amp = 0.2 + 0.6 * it
        x = torch.randn(n, 3, hw, hw, device=DEV, generator=gen) * amp
        costs, best, val = handle.score_argmin(x, y)
        ref = torch.linalg.norm((y - op.forward(x, **fkw)).reshape(n, -1).double(), dim=-1)
        assert rel_l2(host(costs), ref.cpu().numpy()) < TOL and int(best) == int(torch.argmin(costs))
        mo = torch.randn(n, 6, hw, hw, device=DEV, generator=gen) * 0.4 * amp
        z = torch.randn(n, 3, hw, hw, device=DEV, generator=gen)
        K.step_fwd(handle, buf, x, mo, z, y, ck, finalize_norm=True)      # norm finished by the launch itself
        got = buf.norm.clone()
        ref = torch.linalg.norm((y - op.forward(buf.x0_hat, **fkw)).reshape(n, -1).double(), dim=-1)
        assert rel_l2(host(got), ref.cpu().numpy()) < TOL


@pytest.mark.parametrize("hw", [(128, 192), (192, 128), (256, 256), (128, 128)])
@pytest.mark.parametrize("kind,seed", [("motion", 2), ("motion", 7), ("gauss_taps", 0), ("mid", 1), ("wide", 0), ("widest", 0),
                                       ("onesided", 3)])
def test_taps_regular_multi_tile(K, oracle, kind, seed, hw):
    """tap-list operator on regular multi-tile images (loads-first stage; the one-launch adjoint: plain + mirrored-row
    windows, mirrored-column / corner strips in one scan of the run table) for kernels of different reach -- a short
    path and the 25 x 25 Gaussian as a tap list (reach <= 12: 16-column strips), a kernel reaching 20 columns (32-column
    strips), one that reaches 29 px on every side (beyond the strips once rounded to 32: the multi-pass fallback), a
    65 x 65 kernel that reaches 32 px (beyond the strips: the multi-pass fallback) and a kernel whose taps all lie on one
    side of the centre (empty strip ranges) -- against the oracle, plus <A x, u> = <x, A^T u>"""
    rng = np.random.RandomState(seed + hw[0])
    if kind == "motion":
        k2 = synthetic_motion_kernel(61, seed)
    elif kind == "gauss_taps":
        k2 = oracle.tables.gaussian_kernel2d(61, 3.0).astype(np.float32)
    elif kind == "mid":          # reach 18-20 columns: the 32-column strips (4 rows per lane) of the one-scan adjoint
        k2 = np.zeros((61, 61), dtype=np.float32)
        idx = np.stack([rng.randint(20, 41, size=36), rng.randint(10, 51, size=36)], axis=1)
        k2[idx[:, 0], idx[:, 1]] = rng.rand(36).astype(np.float32)
        k2[30, 10] = k2[30, 50] = 0.2
        k2 /= k2.sum()
    elif kind == "widest":
        k2 = np.zeros((65, 65), dtype=np.float32)
        idx = rng.randint(0, 65, size=(48, 2))
        k2[idx[:, 0], idx[:, 1]] = rng.rand(48).astype(np.float32)
        k2[0, 0] = k2[64, 64] = k2[0, 64] = k2[64, 0] = 0.3
        k2[32, 0] = k2[0, 31] = 0.2
        k2 /= k2.sum()
    elif kind == "onesided":
        k2 = np.zeros((61, 61), dtype=np.float32)
        idx = np.stack([rng.randint(31, 50, size=30), rng.randint(8, 30, size=30)], axis=1)     # dy > 0, dx < 0 only
        k2[idx[:, 0], idx[:, 1]] = rng.rand(30).astype(np.float32)
        k2 /= k2.sum()
    else:
        k2 = np.zeros((61, 61), dtype=np.float32)
        idx = rng.randint(1, 60, size=(40, 2))
        k2[idx[:, 0], idx[:, 1]] = rng.rand(40).astype(np.float32)
        k2[1, 1] = k2[59, 59] = k2[1, 59] = k2[59, 1] = 0.3
        k2 /= k2.sum()
    h = K.OpHandle.blur(k2, DEV, force_taps=True)
    assert h.kind == K._lib.KIND_TAPS
    x = rng.randn(2, 3, *hw).astype(np.float32)
    u = rng.randn(2, 3, *hw).astype(np.float32)
    y = h.forward(dev(x))
    g = h.adjoint(dev(u), in_hw=hw)
    assert rel_l2(host(y), oracle.blur_fwd(x, k2)) < TOL
    assert rel_l2(host(g), oracle.blur_adj(u, k2)) < TOL
    lhs = (y.double() * dev(u).double()).sum().item()
    rhs = (dev(x).double() * g.double()).sum().item()
    assert abs(lhs - rhs) <= 2e-5 * max(abs(lhs), np.sqrt(float(y.numel())))


@pytest.mark.parametrize("name,hw,n", [("gauss", 256, 9), ("gauss", 64, 5), ("gauss", 128, 3), ("gauss", 46, 4), ("sr4", 256, 5),
                                       ("inpaint", 64, 4), ("motion", 128, 3), ("phase", 32, 2), ("denoise", 64, 5),
                                       ("denoise", 17, 4), ("inpaint", 63, 3), ("inpaint", (62, 63), 3)])
@pytest.mark.parametrize("t", [700, 0])
def test_search_step_fused_equals_separate(K, oracle, name, hw, n, t):
    """dpsx_search_step_f32 (S1, scoring launch, one launch for costs + select + replication) ==
    dpsx_posterior_fwd_f32 + dpsx_score_argmin_f32 + dpsx_replicate_f32, bit for bit: sample, costs, winner, x_next.
    The segmented forms (segments = 1, 2; below 256 x 256, n made even for two segments by one more particle) against the
    same separate launches scored with each particle's own measurement row, the select being torch.argmin on the host
    per segment: best[m] = m k + argmin(costs[m k : (m + 1) k]), val[m] = costs[best[m]], x_next[m k : (m + 1) k] =
    sample[best[m]]"""
    ih, iw, hw = _pair(hw)
    rng = np.random.RandomState(hw + n + t)
    mask = (np.random.RandomState(3).rand(1, 1, ih, iw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=synthetic_motion_kernel(61, 5), mask=mask)
    _, ck = coefs_of(K, oracle, t)
    x = dev(rng.randn(n, 3, ih, iw).astype(np.float32))
    mo = dev(rng.randn(n, 6, ih, iw).astype(np.float32) * 0.5)
    z = dev(rng.randn(n, 3, ih, iw).astype(np.float32))
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(x)
    y = op.forward(dev(rng.uniform(-1, 1, (1, 3, ih, iw)).astype(np.float32)), **fkw).detach().contiguous()
    for yy in (y, y.expand(n, *y.shape[1:]).contiguous()):
        _, ref_sample = K.posterior_fwd(x, mo, z, ck, want_x0=False)
        ref_costs, ref_best, ref_val = handle.score_argmin(ref_sample, yy)
        for replicate in (True, False):
            x_next, sample, costs, best, val = handle.search_step(x, mo, z, yy, ck, replicate=replicate)
            assert torch.equal(sample, ref_sample) and torch.equal(costs, ref_costs)
            assert int(best) == int(ref_best) == int(torch.argmin(ref_costs)) and torch.equal(val, ref_val)
            if replicate:
                assert torch.equal(x_next, ref_sample[int(ref_best)].unsqueeze(0).expand_as(x_next))
            else:
                assert x_next is None
    if hw == 256:
        return
    y_b = op.forward(dev(rng.uniform(-1, 1, (1, 3, ih, iw)).astype(np.float32)), **fkw).detach().contiguous()
    for segments in (1, 2):
        pad = n % segments
        xs, mos, zs = (torch.cat([a, a[:pad]]) for a in (x, mo, z))
        k = (n + pad) // segments
        for yy in ((y,) if segments == 1 else (y, torch.cat([y, y_b]))):       # one row for all, or one per segment
            _, ref_sample = K.posterior_fwd(xs, mos, zs, ck, want_x0=False)
            ref_costs = handle.score(ref_sample, yy.repeat_interleave((n + pad) // yy.shape[0], dim=0))
            for replicate in (True, False):
                x_next, sample, costs, best, val = handle.search_step(xs, mos, zs, yy, ck, replicate=replicate,
                                                                      segments=segments)
                assert torch.equal(sample, ref_sample) and torch.equal(costs, ref_costs)
                assert best.shape == (segments,) and val.shape == (segments,)
                assert (x_next is None) == (not replicate)
                for m in range(segments):
                    sl = slice(m * k, (m + 1) * k)
                    assert int(best[m]) == m * k + int(torch.argmin(ref_costs[sl])), (segments, m)
                    assert torch.equal(val[m], ref_costs[int(best[m])])
                    if replicate:
                        assert torch.equal(x_next[sl], ref_sample[int(best[m])].unsqueeze(0).expand(k, -1, -1, -1))


@pytest.mark.parametrize("name,hw,n", [("gauss", 256, 9), ("gauss", 64, 5), ("sr4", 256, 5), ("inpaint", 64, 4), ("motion", 128, 3),
                                       ("denoise", 17, 4)])
@pytest.mark.parametrize("t", [700, 0])
def test_search_step_one_state_equals_replicated(K, oracle, name, hw, n, t):
    """dpsx_search_step_one_f32 (one state particle feeds all N proposals, the winner is copied out once) ==
    dpsx_search_step_f32 on N copies of that state, bit for bit: proposals, costs, winner index, winner.
    The segmented forms (segments = 1, 2; below 256 x 256) with one state per segment against the segmented replicated
    step on each state's copies, and the winners against the proposals themselves"""
    rng = np.random.RandomState(hw + n + t + 1)
    mask = (np.random.RandomState(3).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=synthetic_motion_kernel(61, 5), mask=mask)
    _, ck = coefs_of(K, oracle, t)
    x1 = dev(rng.randn(1, 3, hw, hw).astype(np.float32))
    mo1 = dev(rng.randn(1, 6, hw, hw).astype(np.float32) * 0.5)
    z = dev(rng.randn(n, 3, hw, hw).astype(np.float32))
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(x1)
    y = op.forward(dev(rng.uniform(-1, 1, (1, 3, hw, hw)).astype(np.float32)), **fkw).detach().contiguous()
    x_rep, s_rep, c_rep, b_rep, v_rep = handle.search_step(x1.repeat(n, 1, 1, 1), mo1.repeat(n, 1, 1, 1), z, y, ck)
    w_one, s_one, c_one, b_one, v_one = handle.search_step_one(x1, mo1, z, y, ck)
    assert torch.equal(s_one, s_rep) and torch.equal(c_one, c_rep)
    assert int(b_one) == int(b_rep) and torch.equal(v_one, v_rep)
    assert torch.equal(w_one, x_rep[:1]) and torch.equal(w_one, s_rep[int(b_rep)].unsqueeze(0))
    w_none = handle.search_step_one(x1, mo1, z, y, ck, want_winner=False)[0]
    assert w_none is None
    if hw == 256:
        return
    x2 = torch.cat([x1, dev(rng.randn(1, 3, hw, hw).astype(np.float32))])
    mo2 = torch.cat([mo1, dev(rng.randn(1, 6, hw, hw).astype(np.float32) * 0.5)])
    y2 = torch.cat([y, op.forward(dev(rng.uniform(-1, 1, (1, 3, hw, hw)).astype(np.float32)), **fkw).detach()]).contiguous()
    for segments in (1, 2):
        zs = torch.cat([z, z[:n % segments]])
        k = zs.shape[0] // segments
        xs, mos, yy = x2[:segments].contiguous(), mo2[:segments].contiguous(), y2[:segments].contiguous()
        x_rep, s_rep, c_rep, b_rep, v_rep = handle.search_step(xs.repeat_interleave(k, dim=0), mos.repeat_interleave(k, dim=0),
                                                                zs, yy, ck, segments=segments)
        w_one, s_one, c_one, b_one, v_one = handle.search_step_one(xs, mos, zs, yy, ck, segments=segments)
        assert torch.equal(s_one, s_rep) and torch.equal(c_one, c_rep)
        assert b_one.shape == (segments,) and torch.equal(b_one, b_rep) and torch.equal(v_one, v_rep)
        assert torch.equal(w_one, x_rep[::k]) and torch.equal(w_one, s_rep[b_rep])
        assert handle.search_step_one(xs, mos, zs, yy, ck, want_winner=False, segments=segments)[0] is None


@pytest.mark.parametrize("name", ["gauss", "motion", "sr4", "phase"])
def test_fused_step_without_x0_store(K, oracle, name):
    """dpsx_step_fwd_f32 with x0_hat == NULL (blur, resize): the x0_hat image is consumed inside the launch and not written;
    everything downstream -- sample, clamp gate, residual, norm, gradient, x_{t-1} -- is bit for bit the same"""
    rng = np.random.RandomState(11)
    hw, n = (256, 2) if name == "phase" else (128, 3)      # the hand-written spectral step is the 256 -> 384 geometry
    op, fkw = make_product_op(name, hw=hw, kernel=synthetic_motion_kernel(61, 5))
    _, ck = coefs_of(K, oracle, 400)
    x = dev(rng.randn(n, 3, hw, hw).astype(np.float32))
    mo = dev(rng.randn(n, 6, hw, hw).astype(np.float32) * 0.5)
    z = dev(rng.randn(n, 3, hw, hw).astype(np.float32))
    gu = dev(rng.randn(n, 3, hw, hw).astype(np.float32) * 1e-2)
    handle = op.hip_handle(x)
    y = op.forward(dev(rng.uniform(-1, 1, (1, 3, hw, hw)).astype(np.float32)), **fkw).detach().contiguous()
    outs = []
    for want in (True, False):
        buf = K.StepBuffers(handle, n, 3, hw, hw, DEV)
        buf.x0_hat.fill_(123.0)
        K.step_fwd(handle, buf, x, mo, z, y, ck, want_x0=want)
        K.step_bwd(handle, buf, y, 0.5, 1, ck)
        xn = K.step_update(buf, gu, ck)
        outs.append((buf.sample.clone(), buf.inside.clone(), buf.norm.clone(), buf.g_model_out.clone(), xn.clone(),
                     buf.x0_hat.clone()))
    for a, b in zip(outs[0][:5], outs[1][:5]):
        assert torch.equal(a, b)
    assert bool((outs[1][5] == 123.0).all()) and not bool((outs[0][5] == 123.0).all())


# ----------------------------------------------------------------- the denoising operator (get_operator("noise"), OP_IDENT)
@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (3, 3, 17, 13), (1, 1, 5, 3)])
def test_identity_handle_copies_bit_exact(K, shape):
    """OpHandle.identity: A and A^T are device-to-device copies, out_hw is the identity; its scoring launch always uses
    64 partial slots per particle, more than the 15 elements of the smallest shape here (empty chunks sum to zero)"""
    gen = torch.Generator(device=DEV).manual_seed(shape[-1])
    h = K.OpHandle.identity(DEV)
    assert h.kind == K._lib.KIND_IDENT and h.out_hw(*shape[-2:]) == tuple(shape[-2:]) and h.fuses_step(*shape[1:])
    x, u = torch.randn(*shape, device=DEV, generator=gen), torch.randn(*shape, device=DEV, generator=gen)
    y, g = h.forward(x), h.adjoint(u, in_hw=shape[-2:])
    assert y.data_ptr() != x.data_ptr() and torch.equal(y, x)
    assert g.data_ptr() != u.data_ptr() and torch.equal(g, u)
    meas = torch.randn(1, *shape[1:], device=DEV, generator=gen)
    ref = torch.linalg.norm((meas - x).reshape(shape[0], -1).double(), dim=-1).cpu().numpy()
    assert rel_l2(host(h.score(x, meas)), ref) < TOL
    costs, best, val = h.score_argmin(x, meas)
    assert torch.equal(costs, h.score(x, meas)) and int(best) == int(torch.argmin(costs)) and float(val) == float(costs[int(best)])
    op, _ = make_product_op("denoise")
    xt = x.clone().requires_grad_()
    (adj,) = torch.autograd.grad((op.forward(xt) * u).sum(), xt)
    assert torch.equal(adj, u) and op.hip_handle(x).kind == K._lib.KIND_IDENT


@pytest.mark.parametrize("hw", [64, 17])          # 17: 867 floats per particle, the scalar kernels
@pytest.mark.parametrize("t", [900, 400, 0])
@pytest.mark.parametrize("power", [1, 2])
def test_denoise_fused_step_vs_oracle(K, oracle, hw, t, power):
    """S1 + residual_partials, [finalize_norm] + clamp_scale_to_eps against the oracle, both norm-finalisation modes"""
    for finalize in (False, True):
        _fused_case(K, oracle, "denoise", 3, hw, t, 0.7, power, seed=hw + t + power, finalize=finalize)


@pytest.mark.parametrize("hw", [64, 17])
@pytest.mark.parametrize("t,eta", [(900, 0.0), (400, 0.7), (0, 0.0)])
def test_denoise_fused_step_ddim_vs_oracle(K, oracle, hw, t, eta):
    _fused_case(K, oracle, "denoise", 3, hw, t, 0.7, 1, seed=hw + t + 1, ddim_eta=eta)


@pytest.mark.parametrize("hw", [64, 17])
def test_denoise_fused_step_extra_cotangent_and_per_particle_y(K, oracle, hw):
    _fused_case(K, oracle, "denoise", 3, hw, 600, 0.7, 1, seed=hw + 3, extra=True)
    _fused_case(K, oracle, "denoise", 2, hw, 0, 0.4, 2, seed=hw + 4, extra=True, finalize=True)
    _fused_case(K, oracle, "denoise", 3, hw, 300, 0.4, 1, seed=hw + 5, per_particle_y=True)
    _fused_case(K, oracle, "denoise", 2, hw, 700, 0.4, 2, seed=hw + 6, per_particle_y=True, extra=True, finalize=True)


@pytest.mark.parametrize("chw", [(3, 160, 160), (1, 5, 3)])
def test_denoise_fused_step_partial_slot_counts(K, oracle, chw):
    """the identity launches write and re-sum 64 partial slots per particle whatever the size, while the workspace holds
    max(ceil(CHW / 1024), 64): 3 x 160 x 160 is where the first count (75) exceeds 64; 1 x 5 x 3 has fewer elements (15)
    than slots"""
    for finalize in (False, True):
        _fused_case(K, oracle, "denoise", 2, chw[1], 500, 0.5, 1, seed=chw[1], finalize=finalize, chw=chw)
        _fused_case(K, oracle, "denoise", 2, chw[1], 0, 0.5, 2, seed=chw[1] + 1, finalize=finalize, chw=chw, extra=True)


def test_denoise_loop_fused_matches_per_op(K, golden):
    """`ps` on the denoising task, as test_ttc_ddim_fused_matches_per_op: _fusion_plan takes the identity handle (three
    fused launches per step), a foreign callable takes the per-op autograd path; two HIP routes to the same 20-step loop,
    within the loop gate.  (ttc_ddim: the loop whose unpacking fits what `ps` returns on the per-op route.)"""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    g = golden("loop")
    op, _ = make_product_op("denoise")
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.5)
    x_start = dev(g["gauss.r20.x_start"])
    gen = torch.Generator(device=DEV).manual_seed(2)
    y = (x_start[:1].tanh() + 0.05 * torch.randn(1, *x_start.shape[1:], device=DEV, generator=gen)).contiguous()
    res = []
    for fused in (True, False):
        smp = _sampler("ttc_ddim", "20")
        cond = cm.conditioning if fused else (lambda **kw: cm.conditioning(**kw))
        plan = smp._fusion_plan(cond, x_start)
        assert (plan is not None) == fused and (not fused or plan[2].kind == K._lib.KIND_IDENT)
        torch.manual_seed(5)
        img, dist = smp.p_sample_loop(model=StandInModel().to(DEV), x_start=x_start.clone().requires_grad_(),
                                      measurement=y, measurement_cond_fn=cond, record=False, save_root=None)
        res.append((host(img), host(dist), smp.last_resample_ids.cpu().numpy()))
    assert np.isfinite(res[0][0]).all() and np.all(res[0][1] > 0)
    np.testing.assert_array_equal(res[0][2], res[1][2])
    assert rel_l2(res[0][0], res[1][0]) < 1e-4 and rel_l2(res[0][1], res[1][1]) < 1e-4


# ----------------------------------------------------------------- shapes off the float4 grid
@pytest.mark.parametrize("side", [34, 36])
def test_phase_off_vector_grid_forward_adjoint(K, oracle, side):
    """sides 34 and 36 with pad 64 (padded 162 / 164): h % 4 or (h + 2 pad) / 2 % 4 is non-zero, so nothing takes a
    float4 form -- A and its autograd adjoint against the oracle's direct DFT"""
    rng = np.random.RandomState(side)
    op, _ = make_product_op("phase")
    orc = make_oracle_op(oracle, "phase")
    x = rng.uniform(-1, 1, (2, 3, side, side)).astype(np.float32)
    u = rng.randn(2, 3, side + 128, side + 128).astype(np.float32)
    xt = dev(x).requires_grad_()
    y = op.forward(xt)
    (adj,) = torch.autograd.grad((y * dev(u)).sum(), xt)
    assert tuple(y.shape) == (2, 3, side + 128, side + 128)
    assert rel_l2(host(y), orc.forward(x)) < TOL, "forward"
    assert rel_l2(host(adj), orc.adjoint(u, (side, side))) < TOL, "adjoint"


@pytest.mark.parametrize("side", [34, 36])
@pytest.mark.parametrize("t", [900, 0])
@pytest.mark.parametrize("power", [1, 2])
def test_phase_off_vector_grid_fused_step_vs_oracle(K, oracle, side, t, power):
    """the scalar staging kernel of phase_step_fwd and the un-fused backward (C2R, crop, clamp_scale_to_eps): both
    norm-finalisation modes, with and without the extra cotangent"""
    for finalize in (False, True):
        for extra in (False, True):
            _fused_case(K, oracle, "phase", 2, side, t, 0.6, power, seed=side + t + power, finalize=finalize, extra=extra)


def test_phase_odd_padded_size_is_refused(K):
    with pytest.raises(K._lib.DpsxError) as e:
        K.OpHandle.phase(33, 64, 6, DEV)            # 33 + 2 x 64 = 161: no Hermitian half of an odd transform
    assert e.value.code == K._lib.EINVAL


@pytest.mark.parametrize("hw", [(63, 63), (62, 63)])         # H W = 1 and 2 (mod 4)
def test_inpainting_off_grid_per_op_and_refusal(K, oracle, hw):
    """H W not a multiple of 4: A and A^T (scalar k_mask_mul) stay bit-exact; the fused step has no such form, and the
    library says so (DPSX_EUNSUPPORTED) before it launches anything -- OpHandle.fuses_step is the question to ask first"""
    rng = np.random.RandomState(hw[0])
    n = 3
    mask = (np.random.RandomState(7).rand(1, 1, *hw) < 0.5).astype(np.float32)
    op, fkw = make_product_op("inpaint", mask=mask)
    orc = make_oracle_op(oracle, "inpaint", mask=mask)
    x, u = rng.randn(n, 3, *hw).astype(np.float32), rng.randn(n, 3, *hw).astype(np.float32)
    xt = dev(x).requires_grad_()
    y = op.forward(xt, **fkw)
    (adj,) = torch.autograd.grad((y * dev(u)).sum(), xt)
    np.testing.assert_array_equal(host(y), orc.forward(x))
    np.testing.assert_array_equal(host(adj), orc.adjoint(u, hw))
    handle = op.hip_handle_for(fkw["mask"])
    assert not handle.fuses_step(3, *hw) and handle.fuses_step(3, 64, 64)
    _, ck = coefs_of(K, oracle, 500)
    buf = K.StepBuffers(handle, n, 3, *hw, DEV)
    mo, z = dev(rng.randn(n, 6, *hw).astype(np.float32)), dev(rng.randn(n, 3, *hw).astype(np.float32))
    with pytest.raises(K._lib.DpsxError) as e:
        K.step_fwd(handle, buf, dev(x), mo, z, y.detach().contiguous()[:1], ck)
    assert e.value.code == K._lib.EUNSUPPORTED
    with pytest.raises(K._lib.DpsxError) as e:
        K.step_bwd(handle, buf, y.detach().contiguous()[:1], 0.5, 1, ck)
    assert e.value.code == K._lib.EUNSUPPORTED


def test_inpainting_off_grid_loop_takes_the_per_op_path(K):
    """`ps` on a 63 x 63 mask: _fusion_plan answers None from the shape, before the first step, and the loop runs per op.
    Base loop: sampler.particle_groups = 2 changes nothing (no plan, no groups: same bits); a multi-image batch, which
    only the fused step serves, is refused up front.  ttc_ddim (whose per-op unpacking fits a foreign `ps` callable): the
    bound method and the foreign callable now take the same route, bit for bit."""
    import functools
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    hw, n = 63, 3
    gen = torch.Generator(device=DEV).manual_seed(63)
    mask = dev((np.random.RandomState(7).rand(1, 1, hw, hw) < 0.5).astype(np.float32))
    op, _ = make_product_op("inpaint", mask=host(mask))
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.5)
    bound = functools.partial(cm.conditioning, mask=mask)
    x_start = torch.randn(n, 3, hw, hw, device=DEV, generator=gen)
    y = op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1, mask=mask).detach().contiguous()
    model = StandInModel().to(DEV)
    res = []
    for groups in (1, 2):
        smp = _sampler("ddpm", "20")
        smp.particle_groups = groups
        assert smp._fusion_plan(bound, x_start) is None
        torch.manual_seed(7)
        img, dist, _ = smp.p_sample_loop(model=model, x_start=x_start.clone().requires_grad_(), measurement=y,
                                         measurement_cond_fn=bound, record=False, save_root=None)
        assert smp._pgroups is None and smp._bufs is None
        res.append((img, dist))
        with pytest.raises(NotImplementedError, match="multi-image"):
            smp.p_sample_loop(model=model, x_start=torch.cat([x_start, x_start[:1]]).requires_grad_(),
                              measurement=torch.cat([y, y]), measurement_cond_fn=bound, record=False, save_root=None)
    assert bool(torch.isfinite(res[0][0]).all()) and bool((res[0][1] > 0).all())
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    res = []
    for cond in (bound, lambda **kw: cm.conditioning(**kw, mask=mask)):
        smp = _sampler("ttc_ddim", "20")
        assert smp._fusion_plan(cond, x_start) is None
        torch.manual_seed(7)
        img, dist = smp.p_sample_loop(model=model, x_start=x_start.clone().requires_grad_(), measurement=y,
                                      measurement_cond_fn=cond, record=False, save_root=None)
        assert smp._bufs is None
        res.append((img, dist, smp.last_resample_ids))
    assert bool(torch.isfinite(res[0][0]).all()) and bool((res[0][1] > 0).all())
    assert all(torch.equal(u, v) for u, v in zip(res[0], res[1]))
    # the same mask family on the float4 grid keeps its plan
    mask64 = dev((np.random.RandomState(7).rand(1, 1, 64, 64) < 0.5).astype(np.float32))
    assert _sampler("ddpm", "20")._fusion_plan(functools.partial(cm.conditioning, mask=mask64),
                                               torch.zeros(n, 3, 64, 64, device=DEV)) is not None


@pytest.mark.parametrize("name,hw", [("gauss", 47), ("motion", 47), ("denoise", 47), ("phase", 34)])
def test_particle_groups_on_unaligned_slices_match_one_chain(K, oracle, name, hw):
    """kernels.ParticleGroups hands group j a slice of one full-batch buffer set: with C H W = 3 x 47 x 47 = 6627 floats the
    second group's sample / x0_hat / g_model_out / x_next start 8 or 12 bytes past a 16-byte boundary and its clamp gate at
    an odd byte: the scalar kernels on slices.  (A slice is unaligned only where C H W is no multiple of 4, where the size
    test alone already picks the scalar kernel, so this does not show that a launcher also tests its pointers.)  34 x 34
    phase retrieval is the scalar staging + un-fused backward on slices.  Per-particle results equal one chain bit for bit."""
    n, steps = 3, 3
    gen = torch.Generator(device=DEV).manual_seed(hw)
    mk = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)
    op, fkw = make_product_op(name, hw=hw, kernel=synthetic_motion_kernel(61, 5))
    x_t = mk(n, 3, hw, hw)
    ring = [dict(model_out=mk(n, 6, hw, hw) * 0.4, noise=mk(n, 3, hw, hw), g_unet=mk(n, 3, hw, hw) * 1e-2)
            for _ in range(steps)]
    y = op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1, **fkw).detach().contiguous()
    cks = [coefs_of(K, oracle, t)[1] for t in (900, 400, 0)]
    handle = op.hip_handle(x_t)
    buf = K.StepBuffers(handle, n, 3, hw, hw, DEV)
    x = x_t
    for s, ck in zip(ring, cks):
        K.step_fwd(handle, buf, x, s["model_out"], s["noise"], y, ck)
        K.step_bwd(handle, buf, y, 0.3, 1, ck)
        x = K.step_update(buf, s["g_unet"], ck)
    ref, ref_norm, ref_x0 = x.clone(), buf.norm.clone(), buf.x0_hat.clone()
    assert bool(torch.isfinite(ref).all()) and bool((ref_norm > 0).all())
    for groups in (2, 3):
        pg = K.ParticleGroups(op, n, 3, hw, hw, torch.device(DEV), groups, like=x_t)
        assert sum(pg.sizes) == n and len(pg) == groups
        if (3 * hw * hw) % 4:
            assert any(b.sample.data_ptr() % 16 for b in pg.bufs) and any(b.inside.data_ptr() % 4 for b in pg.bufs)
        pg.fork()
        xs = [x_t[sl] for sl in pg.slices]
        for s, ck in zip(ring, cks):
            for j in range(len(pg)):
                pg.step_fwd(j, xs[j], s["model_out"], s["noise"], y, ck)
                pg.step_bwd(j, y, 0.3, 1, ck)
                xs[j] = pg.step_update(j, s["g_unet"], ck)
        pg.join()
        torch.cuda.synchronize()
        assert torch.equal(pg.x_next(), ref), groups
        assert torch.equal(pg.full.norm, ref_norm) and torch.equal(pg.full.x0_hat, ref_x0), groups
