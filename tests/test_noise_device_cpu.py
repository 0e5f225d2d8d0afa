"""CPU suite: the counter-based step noise -- Philox4x32-10 known answers and the counter layout of the NumPy restatement
(tests/noise_ref.py), its moments, the C ABI entry points, the sampler's noise_draw option and the driver flag."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import noise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = ("dpsx_randn_f32", "dpsx_posterior_fwd_rng_f32", "dpsx_step_fwd_rng_f32",
                    "dpsx_search_step_seg_rng_f32", "dpsx_search_step_one_seg_rng_f32")


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("counter, key, expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, expect):
    assert _hex(R.philox4x32_10(counter, key)) == expect


def test_counter_layout():
    """seed -> key, (unit, particle, step, tag) -> counter words 0..3: each input moves exactly its own word"""
    seed = (0x12345678 << 32) | 0x9ABCDEF0
    ctr, key = R.counters(seed, step=7, tag=1, particle=11, units=5)
    assert key == (0x9ABCDEF0, 0x12345678)
    assert ctr[0].tolist() == [0, 1, 2, 3, 4] and ctr[1:] == (11, 7, 1)
    base = R.bits(1, 20, seed, 7, 1, particle_base=11)
    direct = np.stack(R.philox4x32_10((np.arange(5), 11, 7, 1), key), axis=-1).astype(np.uint32).reshape(1, 20)
    assert (base == direct).all()
    for kw in (dict(seed=seed + 1), dict(step=8), dict(tag=0), dict(particle_base=12)):
        args = dict(seed=seed, step=7, tag=1, particle_base=11)
        args.update(kw)
        assert (R.bits(1, 20, **args) != base).any(), kw
    # the unit is the counter's word 0: unit u of a long particle equals unit u of a short one
    assert (R.bits(1, 40, seed, 7, 1, particle_base=11)[:, :20] == base).all()
    # rows of a batch: particle_base + p, or particle_base + p % per_image
    assert R.particle_ids(4, 5).tolist() == [5, 6, 7, 8]
    assert R.particle_ids(4, 5, per_image=2).tolist() == [5, 6, 5, 6]
    four = R.bits(4, 12, 3, 0, particle_base=5, per_image=2)
    assert (four[0] == four[2]).all() and (four[1] == four[3]).all() and (four[0] != four[1]).any()
    assert (R.bits(2, 12, 3, 0, particle_base=6)[0] == four[1]).all()
    # chw % 4 != 0: element e takes word e % 4 of unit e / 4 -- the cut particle is a prefix of the padded one
    assert R.bits(2, 15, 3, 0).shape == (2, 16)
    assert (R.randn(2, 15, 3, 0) == R.randn(2, 16, 3, 0)[:, :15]).all()


def test_moments_of_the_restatement():
    z = R.randn(1, 98304, seed=1234, step=0, tag=0)[0]
    assert np.isfinite(z).all()
    mean, std, share, peak = z.mean(), z.std(), (np.abs(z) < 1).mean(), np.abs(z).max()
    print(f"mean {mean:.4f} std {std:.4f} share(|z| < 1) {share:.4f} max {peak:.2f}")
    assert abs(mean) <= 0.02 and abs(std - 1) <= 0.02 and abs(share - 0.6827) <= 0.01
    assert peak <= 5.77


def test_transform_bounds():
    """u1 in (0, 1], u2 in [0, 1): the extreme words give finite values inside |z| <= sqrt(48 ln 2)"""
    for r in (0, 0xFF, 0x100, 0xFFFFFFFF, 0xFFFFFF00):
        for q in (0, 0xFFFFFFFF, 0x40000000, 0x80000000):
            z = R.normals_from_bits(np.array([[r, q, q, r]], dtype=np.uint32), 4)
            assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(48 * np.log(2.0)) + 1e-12


def test_header_declares_and_lib_binds_the_entry_points():
    from dps_ttc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dpsx.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"typedef struct dpsx_rng \{ uint64_t seed; uint32_t step; uint32_t tag; int64_t particle_base; "
                     r"int64_t per_image; \} dpsx_rng;", hdr)
    assert [f[0] for f in _lib.RngRec._fields_] == ["seed", "step", "tag", "particle_base", "per_image"]
    assert ctypes.sizeof(_lib.RngRec) == 32
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib.SIGNATURES["dpsx_randn_f32"] == (ctypes.c_int, [p, p, i64, i64, ctypes.POINTER(_lib.RngRec), p])
    # dpsx_step_fwd_f32 with the record in the place of the noise pointer
    ref = list(_lib.SIGNATURES["dpsx_step_fwd_f32"][1])
    ref[3] = ctypes.POINTER(_lib.RngRec)
    assert _lib.SIGNATURES["dpsx_step_fwd_rng_f32"] == (ctypes.c_int, ref)
    assert _lib.ABI_VERSION == 3            # an additive change
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_rng_record_validation():
    from dps_ttc_amd import kernels
    r = kernels.Rng((1 << 40) + 5, 3, particle_base=7)
    rec = r.rec()
    assert (rec.seed, rec.step, rec.tag, rec.particle_base, rec.per_image) == ((1 << 40) + 5, 3, 0, 7, 0)
    assert r.offset(4).particle_base == 11 and r.offset(4).step == 3
    multi = kernels.Rng(1, 0, per_image=2, particle_base=7)
    assert multi.offset(4).particle_base == 7                   # whole images: p % per_image is unchanged
    with pytest.raises(ValueError):
        multi.offset(3)
    for bad in (dict(seed=-1), dict(seed=1 << 64), dict(step=1 << 32), dict(tag=-1), dict(particle_base=-1),
                dict(per_image=-2)):
        kw = dict(seed=0, step=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            kernels.Rng(**kw)


def _sampler(name="ddpm"):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing="20")


def test_sampler_option_defaults_and_validation():
    for name in ("ddpm", "ddim", "ttc_ddim", "search_ddpm"):
        s = _sampler(name)
        assert (s.noise_draw, s.noise_seed, s.path_base) == ("torch", 0, 0)
        assert s._step_rng(5, 4) is None
    s = _sampler()
    with pytest.raises(ValueError, match="noise_draw"):
        s._check_noise_draw("philox")
    s.noise_draw = "philox"
    with pytest.raises(ValueError, match="noise_draw"):
        s._step_rng(0, 4)
    s.noise_draw, s.noise_seed, s.path_base = "device", 9, 64
    r = s._step_rng(17, 8)
    assert (r.seed, r.step, r.tag, r.particle_base, r.per_image) == (9, 17, 0, 64, 0)
    assert s._step_rng(17, 8, images=2).per_image == 4


def test_device_draw_conflicts_with_rng_parity():
    s = _sampler()
    s.noise_draw, s.rng_parity = "device", True
    with pytest.raises(ValueError, match="rng_parity"):
        s._step_rng(0, 4)


def test_noise_or_rng_exactly_one():
    from dps_ttc_amd import kernels
    with pytest.raises(ValueError, match="exactly one"):
        kernels._noise_or_rng(None, None)
    with pytest.raises(ValueError, match="exactly one"):
        kernels._noise_or_rng(object(), kernels.Rng(0, 0))


def test_driver_flag(capsys):
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    assert drv.parse_args([]).noise_draw == "torch"
    assert drv.parse_args(["--noise_draw", "device"]).noise_draw == "device"
    with pytest.raises(SystemExit) as e:
        drv.parse_args(["--noise_draw", "philox"])
    assert e.value.code == 2 and "--noise_draw" in capsys.readouterr().err
