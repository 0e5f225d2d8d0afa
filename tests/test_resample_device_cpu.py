"""CPU suite: the device resampling draw -- its two C ABI entry points, the NumPy restatement of the draw rule
(tests/resample_ref.py) as a sampler in its own right, and the driver's --resample_draw option."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import yaml

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_resampling_entry_points():
    from dps_ttc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dpsx.h")).read()
    for name in ("dpsx_resample_draw_seg_f32", "dpsx_resample_seg_f32"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    # d, u, segments, k, inv_scale, ids_out, q_out, stream
    assert _lib.SIGNATURES["dpsx_resample_draw_seg_f32"] == (ctypes.c_int, [p, p, i64, i64, ctypes.c_float, p, p, p])
    # d, u, segments, k, inv_scale, src, dst, d_out, ids_out, q_out, n, chw, stream
    assert _lib.SIGNATURES["dpsx_resample_seg_f32"] == (
        ctypes.c_int, [p, p, i64, i64, ctypes.c_float, p, p, p, p, p, i64, i64, p])
    assert re.search(r"dpsx_resample_seg_f32\([^)]*int64_t \*ids_out, int32_t \*q_out,\s*int64_t n, int64_t chw", hdr)
    assert _lib.ABI_VERSION == 3            # an additive change


SCALE = 100.0                               # ttc_ddim's resample_scale
INV = np.float32(1.0 / SCALE)


def _distances(k, seed):
    return (50.0 + 30.0 * np.random.RandomState(seed).randn(k)).astype(np.float32)


@pytest.mark.parametrize("k", [2, 16, 64, 512, 4096])
def test_restatement_is_a_correct_sampler(k):
    d = _distances(k, 100 + k)
    q = R.weights(d, INV)
    assert q.min() >= 0 and q.max() == R.TWO24 and q[np.argmin(d)] == R.TWO24          # the best particle has weight 1
    total = int(q.sum())
    # the grid ui = j 2^8, j in [0, 2^16): u = j 2^-16, exact in fp32
    j = np.arange(1 << 16)
    u = (j.astype(np.float64) / (1 << 16)).astype(np.float32)
    assert (R.uniform_ints(u) == (j << 8)).all()
    cdf = np.cumsum(q.astype(np.uint64), dtype=np.uint64)
    target = (np.uint64(total) * R.uniform_ints(u)) >> np.uint64(24)
    ids = np.minimum(np.searchsorted(cdf, target, side="right"), k - 1)
    assert ids.min() >= 0 and ids.max() <= k - 1
    assert (np.diff(ids) >= 0).all()                                                   # non-decreasing in u
    # target_j = floor(total j / 2^16), so id i is drawn for the integers j in [cdf_{i-1} 2^16 / total, cdf_i 2^16 / total):
    # an interval of length q_i 2^16 / total holds that many integers give or take one
    counts = np.bincount(ids, minlength=k)
    expect = q.astype(np.float64) * (1 << 16) / total
    assert np.abs(counts - expect).max() <= 1.0
    assert (counts[q == 0] == 0).all()
    # q_i / total against the float64 probabilities p_i = w_i / W, w_i = exp(-(d_i - d_min) / scale), W = sum w >= 1.
    # With q_i = 2^24 w_i + e_i, |e_i| <= e:  |q_i / Q - p_i| = |e_i W - w_i E| / (Q W) with |E| <= K e, Q >= 2^24 (the best
    # particle's weight is exactly 2^24) and w_i <= 1, so the error is at most e (1 + K / W) / 2^24.  Rounding alone is
    # e = 1/2: at most (K + 1) 2^-25.  e also carries, in units of 2^-24 of a weight <= 1: the fp32 exp (NumPy documents at
    # most 4 ulp for its SIMD routines: 4 units), and the fp32 argument x = (d_i - d_min) * fl(1 / scale) -- three roundings,
    # relative 3 * 2^-24, which move w = exp(-x) by w x 3 * 2^-24 <= (1 / e) * 3 units = 1.11 units.  e = 0.5 + 4 + 1.11.
    d64 = d.astype(np.float64)
    w = np.exp(-(d64 - d64.min()) / SCALE)
    p = w / w.sum()
    err = np.abs(q / total - p).max()
    bound = (0.5 + 4.0 + 1.11) * (1.0 + k / w.sum()) / R.TWO24
    print(f"K={k}: max |q/total - p| = {err:.3e} (bound {bound:.3e}, rounding part {(k + 1) * 2.0 ** -25:.3e})")
    assert err <= bound
    # the same distribution as the reference's exp(-d / 100) weights (multinomial normalises)
    p_ref = np.exp(-d64 / SCALE)
    assert np.abs(p_ref / p_ref.sum() - p).max() < 1e-12


def test_restatement_edge_rules():
    u = np.array([0.0, 0.3, 0.6, np.float32(1) - np.float32(2.0 ** -24)], dtype=np.float32)
    # flat: equal distances, K = 1, no finite distance -> identity whatever u holds
    assert R.draw(R.weights([3.0, 3.0, 3.0, 3.0], INV), u).tolist() == [0, 1, 2, 3]
    assert R.draw(R.weights([7.5], INV), u[:1]).tolist() == [0]
    q = R.weights([np.nan, np.inf, -np.inf, np.nan], INV)
    assert q.tolist() == [0, 0, 0, 0] and R.draw(q, u).tolist() == [0, 1, 2, 3]
    # differences below the quantisation step are flat too (the reference's max == min skip on the weights)
    assert R.draw(R.weights([1.0, 1.0 + 1e-6], INV), u[:2]).tolist() == [0, 1]
    # NaN / inf distances have weight 0 and are never drawn
    q = R.weights([5.0, np.nan, 7.0, np.inf], INV)
    assert q[1] == 0 and q[3] == 0 and q[0] == R.TWO24 and 0 < q[2] < R.TWO24
    many = np.linspace(0, 1, 4096, endpoint=False, dtype=np.float32)
    cdf = np.cumsum(q.astype(np.uint64))
    ids = np.searchsorted(cdf, (cdf[-1] * R.uniform_ints(many)) >> np.uint64(24), side="right")
    assert set(ids.tolist()) == {0, 2}
    assert set(R.draw(q, u).tolist()) <= {0, 2}
    # u outside [0, 1) and NaN are clamped, never out of range
    assert R.uniform_ints([np.nan, -1.0, 0.0, 1.0, 2.0, np.inf]).tolist() == [0, 0, 0, R.TWO24 - 1, R.TWO24 - 1, R.TWO24 - 1]
    # ids are global and stay inside their segment
    q2 = np.concatenate([R.weights([5.0, 1.0, 9.0], INV), R.weights([2.0, 2.0, 2.0], INV), R.weights([0.0, 50.0, 900.0], INV)])
    ids = R.draw_segments(q2, np.array([0.9, 0.1, 0.5, 0.9, 0.1, 0.5, 0.9, 0.1, 0.999], dtype=np.float32), 3)
    assert (ids // 3 == np.repeat(np.arange(3), 3)).all() and ids[3:6].tolist() == [3, 4, 5]


# ----------------------------------------------------------------- driver
def _driver():
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    return drv


def test_driver_lets_ttc_ddim_batches_through_with_the_device_draw(monkeypatch):
    import torch
    drv = _driver()

    def no_gpu(*a, **kw):
        raise AssertionError("the check touched the GPU")
    for fn in ("is_available", "set_device", "device_count"):
        monkeypatch.setattr(torch.cuda, fn, no_gpu)
    assert drv.parse_args([]).resample_draw == "multinomial"
    args = drv.parse_args(["--images_per_batch", "2", "--resample_draw", "device"])
    assert drv.check_images_per_batch(args, "ttc_ddim", 1) is None
    with pytest.raises(SystemExit) as e:                          # the default draw keeps the refusal
        drv.check_images_per_batch(drv.parse_args(["--images_per_batch", "2"]), "ttc_ddim", 1)
    assert "ttc_ddim" in str(e.value) and "--resample_draw" in str(e.value) and "\n" not in str(e.value)
    with pytest.raises(SystemExit):                               # several ranks stay out of scope
        drv.check_images_per_batch(args, "ttc_ddim", 2)


def test_driver_rejects_an_unknown_draw(capsys):
    drv = _driver()
    with pytest.raises(SystemExit) as e:
        drv.parse_args(["--resample_draw", "systematic"])
    assert e.value.code == 2 and "--resample_draw" in capsys.readouterr().err


def test_sampler_option_defaults_and_validation():
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    kw = dict(steps=1000, noise_schedule="linear", model_mean_type="epsilon", model_var_type="learned_range",
              dynamic_threshold=False, clip_denoised=True, rescale_timesteps=True, timestep_respacing="20")
    for name in ("ttc_ddim", "search_ddpm"):
        assert create_sampler(sampler=name, **kw).resample_draw == "multinomial"
    with pytest.raises(ValueError, match="resample_draw"):
        create_sampler(sampler="ddpm", **kw)._check_resample_draw("systematic")
