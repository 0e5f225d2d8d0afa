"""CPU suite: the resampling schemes and the ESS trigger -- the integer restatement's own properties
(tests/resample_scheme_ref.py), the host-side validation of the sampler attributes and the driver flags, and the two new
C ABI entry points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import resample_ref as R
import resample_scheme_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = np.float32(0.01)
ONE_BELOW = np.float32(1) - np.float32(2.0 ** -24)


def _cases():
    """seeded (q, u) segments, K = 2 ... 512: spread-out and nearly flat weights, zero weights, ties, extreme uniforms"""
    rng = np.random.RandomState(5)
    out = []
    for c in range(120):
        k = int(rng.choice([2, 3, 5, 8, 16, 17, 64, 257, 512]))
        spread = float(rng.choice([0.01, 1.0, 30.0, 300.0]))
        d = (50.0 + spread * rng.randn(k)).astype(np.float32)
        if c % 3 == 0:
            d[rng.randint(k)] = np.nan
        if c % 4 == 0 and k > 2:
            d[1] = d[0]
        u = rng.rand(k).astype(np.float32)
        if c % 5 == 0:
            u[0], u[-1] = 0.0, ONE_BELOW
        out.append((R.weights(d, INV), u))
    out.append((np.array([R.TWO24, 0, 0, 0]), np.array([ONE_BELOW] * 4, dtype=np.float32)))
    out.append((np.array([0, 0, R.TWO24, 1]), np.array([0.0, 0.5, 0.75, ONE_BELOW], dtype=np.float32)))
    return out


CASES = _cases()


@pytest.mark.parametrize("scheme", [S.STRATIFIED, S.SYSTEMATIC])
def test_count_bounds_sortedness_and_zero_weights(scheme):
    moved = 0
    for q, u in CASES:
        k, t = len(q), int(q.sum())
        assert all(tg < t for tg in S.targets(q, u, scheme))
        ids = S.draw(q, u, scheme)
        if not S.need(q, S.ONE_Q16):
            assert ids.tolist() == list(range(k))
            continue
        moved += 1
        assert ids.min() >= 0 and ids.max() <= k - 1
        assert (np.diff(ids) >= 0).all()                                     # non-decreasing in the slot index
        assert (np.asarray(q)[ids] > 0).all()                                # a zero weight is never drawn
        n = S.counts(ids, k)
        lo, hi = S.count_bounds(q, scheme)
        assert (n >= lo).all() and (n <= hi).all(), (scheme, k, (n - lo).min(), (hi - n).min())
        if scheme == S.SYSTEMATIC:                                           # the best particle(s) survive
            assert (n[np.asarray(q) == np.asarray(q).max()] >= 1).all()
    assert moved > 100


def test_trigger_rules():
    for q, u in CASES:
        flat = bool((np.asarray(q) == np.asarray(q)[0]).all())
        assert S.need(q, S.ONE_Q16) == (not flat)                            # tau = 1: exactly the flat rule
        assert not S.need(q, 0)                                              # tau = 0: never
        for scheme in (S.MULTINOMIAL, S.STRATIFIED, S.SYSTEMATIC):
            assert S.draw(q, u, scheme, 0).tolist() == list(range(len(q)))
        assert np.array_equal(S.draw(q, u, S.MULTINOMIAL), R.draw(q, u))     # scheme 0, tau = 1: the existing draw
        m = S.min_trigger(q)
        if m is not None and m <= S.ONE_Q16:
            assert S.need(q, m) and not S.need(q, m - 1)
        # the reported ESS is (sum q)^2 / sum q^2, in [1, K] for a segment with a finite distance
        e = float(S.ess(q))
        assert 1.0 - 1e-6 <= e <= len(q) * (1 + 1e-6)
        # the trigger is the ESS test: ESS < tau K, away from the rounding of the threshold
        for tau in (0.25, 0.5, 0.9):
            if abs(e - tau * len(q)) > 1e-3 * len(q):
                assert S.need(q, S.ess_q16_of(tau)) == (e < tau * len(q))
    assert not S.need([0, 0, 0], S.ONE_Q16) and float(S.ess([0, 0, 0])) == 0.0
    assert S.draw([7], np.float32([0.3]), S.SYSTEMATIC).tolist() == [0]
    assert [S.ess_q16_of(t) for t in (0.0, 0.5, 0.999, 1.0)] == [0, 32768, 65470, 65536]


def test_segments_and_bad_uniforms():
    q = np.concatenate([R.weights([5.0, 1.0, 9.0, 2.0], INV), R.weights([2.0] * 4, INV),
                        R.weights([np.nan, np.inf, -np.inf, np.nan], INV)])
    u = np.array([np.nan, -3.0, 1.0, np.inf] * 3, dtype=np.float32)
    for scheme in (S.MULTINOMIAL, S.STRATIFIED, S.SYSTEMATIC):
        ids, flags, e = S.draw_segments(q, u, 3, scheme)
        assert (ids // 4 == np.repeat(np.arange(3), 4)).all()
        assert flags.tolist() == [1, 0, 0] and ids[4:].tolist() == list(range(4, 12))
        assert e[2] == 0 and abs(e[1] - 4.0) < 1e-6


@pytest.mark.parametrize("scheme", [S.STRATIFIED, S.SYSTEMATIC])
def test_mean_counts_are_unbiased(scheme):
    import torch
    torch.manual_seed(0)
    u = torch.rand(S.MEAN_M * S.MEAN_K).numpy()
    q = np.tile(R.weights(S.MEAN_D, INV), S.MEAN_M)
    ids, flags, _ = S.draw_segments(q, u, S.MEAN_M, scheme)
    assert flags.all()
    err = S.mean_count_error(ids, q, S.MEAN_M, S.MEAN_K)
    print(f"scheme {scheme}: max |mean n_i - K q_i / T| = {err:.4f} (bound {S.MEAN_BOUND[scheme]:.4f})")
    assert err <= S.MEAN_BOUND[scheme]


# ----------------------------------------------------------------- C ABI
def test_header_library_and_bindings_agree_on_the_new_entry_points():
    from dps_ttc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dpsx.h")).read()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in ("dpsx_resample_draw_seg_ex_f32", "dpsx_resample_seg_ex_f32"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    p, i64, f, i, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int, ctypes.c_int32
    # d, u, segments, k, inv_scale, ids_out, q_out, scheme, ess_q16, resampled_out, ess_out, stream
    assert _lib.SIGNATURES["dpsx_resample_draw_seg_ex_f32"] == (i, [p, p, i64, i64, f, p, p, i, i32, p, p, p])
    # d, u, segments, k, inv_scale, src, dst, d_out, ids_out, q_out, n, chw, scheme, ess_q16, resampled_out, ess_out, stream
    assert _lib.SIGNATURES["dpsx_resample_seg_ex_f32"] == (i, [p, p, i64, i64, f, p, p, p, p, p, i64, i64, i, i32, p, p, p])
    tail = r"int scheme, int32_t ess_q16,\s*uint8_t \*resampled_out,\s*float \*ess_out, void \*stream\)"
    assert re.search(r"dpsx_resample_draw_seg_ex_f32\([^)]*int32_t \*q_out, " + tail, hdr)
    assert re.search(r"dpsx_resample_seg_ex_f32\([^)]*int64_t n, int64_t chw, " + tail, hdr)
    for name, value in (("MULTINOMIAL", 0), ("STRATIFIED", 1), ("SYSTEMATIC", 2)):
        assert re.search(r"DPSX_RESAMPLE_%s = %d\b" % (name, value), hdr)
    assert _lib.ABI_VERSION == 3 and raw.dpsx_abi_version() == 3            # an additive change


def test_wrapper_argument_validation():
    from dps_ttc_amd import kernels
    assert kernels.RESAMPLE_SCHEMES == S.SCHEMES
    assert kernels.resample_scheme_args("multinomial", None) == (0, 65536)
    assert kernels.resample_scheme_args("systematic", 0.5) == (2, 32768)
    assert kernels.resample_scheme_args("stratified", 0.0) == (1, 0)
    for tau in (0.0, 0.3, 0.5, 0.999, 1.0):
        assert kernels.resample_scheme_args("stratified", tau)[1] == S.ess_q16_of(tau)
    with pytest.raises(ValueError, match="scheme"):
        kernels.resample_scheme_args("residual", None)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ESS"):
            kernels.resample_scheme_args("systematic", bad)


# ----------------------------------------------------------------- sampler attributes
def _sampler(name):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing="20")


def test_sampler_attributes_defaults_and_refusals():
    for name in ("ttc_ddim", "search_ddpm"):
        smp = _sampler(name)
        assert smp.resample_scheme == "multinomial" and smp.resample_ess is None
        assert smp.last_resample_flags is None and smp.last_resample_ess is None
        assert smp._check_resample_scheme("multinomial") is None and smp._check_resample_scheme("device") is None
        smp.resample_scheme = "systematic"
        with pytest.raises(ValueError, match=r"resample_scheme.*resample_draw"):      # not the device draw
            smp._check_resample_scheme("multinomial")
        assert smp._check_resample_scheme("device") == ("systematic", None)
        smp.resample_scheme, smp.resample_ess = "multinomial", 0.5
        with pytest.raises(ValueError, match=r"resample_ess.*resample_draw"):
            smp._check_resample_scheme("multinomial")
        assert smp._check_resample_scheme("device") == ("multinomial", 0.5)
        assert smp._check_resample_scheme("device", "stratified", 1.0) == ("stratified", 1.0)     # per-call overrides
        smp.resample_ess = 1.5
        with pytest.raises(ValueError, match="ESS"):
            smp._check_resample_scheme("device")
        smp.resample_scheme, smp.resample_ess = "residual", None
        with pytest.raises(ValueError, match="scheme"):
            smp._check_resample_scheme("device")
    smp = _sampler("ttc_ddim")
    assert smp.resample_every == 10
    smp.resample_draw, smp.resample_scheme, smp.global_resample = "device", "systematic", True
    with pytest.raises(NotImplementedError, match=r"resample_scheme.*global"):        # several ranks
        smp._check_resample_scheme("device")


# ----------------------------------------------------------------- driver
def _driver():
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    return drv


def test_driver_flags(capsys):
    drv = _driver()
    args = drv.parse_args([])
    assert (args.resample_scheme, args.resample_ess, args.ttc_resample_every) == ("multinomial", None, 10)
    assert args.resample_every_steps == 10                                   # the existing flag keeps its meaning
    assert drv.check_resample_scheme(args) is None
    args = drv.parse_args(["--resample_draw", "device", "--resample_scheme", "systematic", "--resample_ess", "0.5",
                           "--ttc_resample_every", "1"])
    assert (args.resample_scheme, args.resample_ess, args.ttc_resample_every) == ("systematic", 0.5, 1)
    assert drv.check_resample_scheme(args) is None
    for flags, word in ((["--resample_scheme", "stratified"], "--resample_scheme"),
                        (["--resample_ess", "0.5"], "--resample_ess"),
                        (["--resample_ess", "1.0"], "--resample_ess")):
        with pytest.raises(SystemExit) as e:                                 # refused without --resample_draw device
            drv.check_resample_scheme(drv.parse_args(flags))
        assert word in str(e.value) and "--resample_draw device" in str(e.value) and "\n" not in str(e.value)
    with pytest.raises(SystemExit, match="--resample_ess"):
        drv.check_resample_scheme(drv.parse_args(["--resample_draw", "device", "--resample_ess", "1.5"]))
    with pytest.raises(SystemExit, match="--ttc_resample_every"):
        drv.check_resample_scheme(drv.parse_args(["--ttc_resample_every", "0"]))
    ok = ["--resample_draw", "device", "--resample_scheme", "systematic", "--resample_ess", "0.5", "--ttc_resample_every", "2"]
    assert drv.check_resample_scheme(drv.parse_args(ok), "ttc_ddim") is None
    assert drv.check_resample_scheme(drv.parse_args([]), "ddpm") is None
    for keep, word in ((slice(0, 4), "--resample_scheme"), ([0, 1, 4, 5], "--resample_ess"), ([6, 7], "--ttc_resample_every")):
        flags = ok[keep] if isinstance(keep, slice) else [ok[i] for i in keep]
        with pytest.raises(SystemExit) as e:                                 # a sampler whose loop never resamples
            drv.check_resample_scheme(drv.parse_args(flags), "ddim")
        assert word in str(e.value) and "ttc_ddim" in str(e.value) and "ddim)" in str(e.value) and "\n" not in str(e.value)
    with pytest.raises(SystemExit) as e:
        drv.parse_args(["--resample_scheme", "residual"])
    assert e.value.code == 2 and "--resample_scheme" in capsys.readouterr().err


def test_driver_main_refuses_before_touching_the_gpu(monkeypatch):
    import torch
    drv = _driver()

    def no_gpu(*a, **kw):
        raise AssertionError("the check touched the GPU")
    for fn in ("is_available", "set_device", "device_count"):
        monkeypatch.setattr(torch.cuda, fn, no_gpu)
    with pytest.raises(SystemExit, match="--resample_scheme"):
        drv.main(["--resample_scheme", "systematic"])
