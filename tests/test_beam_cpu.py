"""CPU suite: beam search for search_ddpm -- the order's restatement against hand-written cases, the two new entry points
in the header / the exports / the ctypes table, what SearchDDPM and the driver refuse before any launch, and that
beam_width = 1 never reaches the new entry point."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import yaml

import beam_ref
from standin import StandInModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dpsx_topk_seg_f32", "dpsx_search_step_beam_f32")
NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------- the order
def test_order_ties_take_the_lower_index():
    assert beam_ref.topb([3.0, 1.0, 1.0, 2.0, 1.0], 1, 5).tolist() == [1, 2, 4, 3, 0]
    assert beam_ref.topb([7.0] * 6, 2, 2).tolist() == [0, 1, 3, 4]


def test_order_signed_zeros_are_equal():
    assert beam_ref.topb([0.0, -0.0, 0.0, -0.0], 1, 4).tolist() == [0, 1, 2, 3]
    assert beam_ref.topb([1.0, 0.0, -0.0, -1.0], 1, 3).tolist() == [3, 1, 2]


def test_order_nan_first_then_infinities_in_place():
    v = [2.0, NAN, -INF, INF, NAN, -3.0, INF]
    assert beam_ref.topb(v, 1, 7).tolist() == [1, 4, 2, 5, 0, 3, 6]
    assert beam_ref.topb(v, 1, 2).tolist() == [1, 4]
    assert beam_ref.topb([INF, INF, -INF, -INF], 1, 4).tolist() == [2, 3, 0, 1]


def test_order_b1_is_numpys_first_minimum_with_nan_first():
    rng = np.random.RandomState(4)
    for trial in range(40):
        v = rng.randint(-3, 4, size=11).astype(np.float32)       # many ties
        if trial % 3 == 0:
            v[rng.randint(11)] = np.nan
        if trial % 6 == 0:
            v[rng.randint(11)] = np.nan
        # numpy.argmin: the first NaN where there is one, else the first minimum -- torch.argmin's rule
        assert beam_ref.topb(v, 1, 1).tolist() == [int(np.argmin(v))]
    v = rng.randn(3 * 9).astype(np.float32)
    assert beam_ref.topb(v, 3, 1).tolist() == [m * 9 + int(np.argmin(v[m * 9:(m + 1) * 9])) for m in range(3)]


def test_order_b_equal_l_is_a_sorted_permutation_per_segment():
    rng = np.random.RandomState(5)
    v = rng.randn(4 * 13).astype(np.float32)
    ids = beam_ref.topb(v, 4, 13).reshape(4, 13)
    for m in range(4):
        assert sorted(ids[m].tolist()) == list(range(m * 13, (m + 1) * 13))
        assert np.all(np.diff(v[ids[m]]) >= 0)
    with pytest.raises(ValueError):
        beam_ref.topb(v, 4, 14)
    with pytest.raises(ValueError):
        beam_ref.topb(v, 4, 0)
    with pytest.raises(ValueError):
        beam_ref.topb(v, 5, 1)


# ----------------------------------------------------------------- the ABI
def test_header_exports_and_signatures_hold_the_two_entry_points():
    from dps_ttc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dpsx.h")).read()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    # top-k: argmin_seg's arguments plus b; the beam step: the single-state segmented step's plus the second noise
    # source, the state count and the beam width
    assert len(_lib.SIGNATURES["dpsx_topk_seg_f32"][1]) == len(_lib.SIGNATURES["dpsx_argmin_seg_f32"][1]) + 1
    assert len(_lib.SIGNATURES["dpsx_search_step_beam_f32"][1]) == \
        len(_lib.SIGNATURES["dpsx_search_step_one_seg_f32"][1]) + 3
    assert _lib.lib().dpsx_abi_version() == 3


# ----------------------------------------------------------------- SearchDDPM
def _sampler(respacing="4"):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler="search_ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing=respacing)


class _NoLaunch:
    """an operator whose handle must never be asked for: the refusals come before any launch"""
    name = "gaussian_blur"

    def hip_handle(self, *a, **kw):
        raise AssertionError("a handle was requested before the arguments were refused")
    hip_handle_for = hip_handle


def _loop(smp, n, operator, **kw):
    return smp.p_sample_loop(model=StandInModel(), x_start=torch.zeros(n, 3, 8, 8), measurement=torch.zeros(1, 3, 8, 8),
                             measurement_cond_fn=None, record=False, save_root=None, operator=operator, **kw)


def test_beam_width_defaults_to_one():
    from dps_ttc_amd.gaussian_diffusion import SearchDDPM
    assert SearchDDPM.beam_width == 1 and _sampler().beam_width == 1


def test_beam_width_must_divide_the_particles_per_image():
    smp = _sampler()
    smp.beam_width = 4
    with pytest.raises(ValueError, match="beam_width"):
        _loop(smp, 6, _NoLaunch())
    smp.beam_width = 3
    with pytest.raises(ValueError, match="beam_width"):       # 12 particles, 3 images: 4 per image
        smp.p_sample_loop(model=StandInModel(), x_start=torch.zeros(12, 3, 8, 8), measurement=torch.zeros(3, 3, 8, 8),
                          measurement_cond_fn=None, record=False, save_root=None, operator=_NoLaunch(), n_images=3)
    smp.beam_width = 0
    with pytest.raises(ValueError, match="beam_width"):
        _loop(smp, 6, _NoLaunch())


def test_beam_refuses_a_global_select():
    smp = _sampler()
    smp.beam_width = 2
    smp.global_select = lambda *a, **kw: None
    with pytest.raises(NotImplementedError, match="global") as e:
        _loop(smp, 6, _NoLaunch())
    assert "\n" not in str(e.value)


def test_beam_refuses_the_replicated_form():
    smp = _sampler()
    smp.beam_width = 2
    smp.single_state = False
    with pytest.raises(ValueError, match="single_state"):
        _loop(smp, 6, _NoLaunch())


class _FakeHandle:
    """torch stand-ins of the two existing steps (CPU); the beam step is the tripwire"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _pick(sample):
        costs = sample.flatten(1).norm(dim=1)
        best = torch.argmin(costs)
        return costs, best

    def search_step(self, x_t, model_out, noise, y, coefs, replicate=True, segments=None, rng=None):
        self.calls.append("search_step")
        sample = 0.5 * x_t + 0.1 * noise
        costs, best = self._pick(sample)
        return sample[best].repeat(x_t.shape[0], 1, 1, 1), sample, costs, best, costs[best].reshape(1)

    def search_step_one(self, x_one, model_out_one, noise, y, coefs, want_winner=True, segments=None, rng=None, n=None):
        self.calls.append("search_step_one")
        sample = 0.5 * x_one + 0.1 * noise
        costs, best = self._pick(sample)
        return sample[best][None], sample, costs, best, costs[best].reshape(1)

    def search_step_beam(self, *a, **kw):
        self.calls.append("search_step_beam")
        raise AssertionError("the beam step was called")


class _FakeOperator:
    name = "gaussian_blur"

    def __init__(self):
        self.handle = _FakeHandle()

    def hip_handle(self, img):
        return self.handle


def test_beam_width_one_never_reaches_the_new_entry_point(monkeypatch):
    from dps_ttc_amd import _lib, kernels

    def boom(*a, **kw):
        raise AssertionError("beam_width = 1 reached the beam entry point")
    monkeypatch.setattr(kernels, "require_cuda", lambda *a, **kw: None)
    monkeypatch.setattr(kernels.OpHandle, "search_step_beam", boom)
    monkeypatch.setattr(_lib.lib(), "dpsx_search_step_beam_f32", boom)
    smp, op = _sampler(), _FakeOperator()
    monkeypatch.setattr(type(smp), "search_step_beam", boom)
    out = _loop(smp, 6, op)
    assert out.shape == (6, 3, 8, 8)
    assert op.handle.calls == ["search_step"] + ["search_step_one"] * (smp.num_timesteps - 1)


def test_beam_width_above_one_goes_through_the_new_entry_point(monkeypatch):
    from dps_ttc_amd import kernels
    monkeypatch.setattr(kernels, "require_cuda", lambda *a, **kw: None)
    smp, op = _sampler(), _FakeOperator()
    smp.beam_width = 3
    with pytest.raises(AssertionError, match="beam step was called"):
        _loop(smp, 6, op)
    assert op.handle.calls == ["search_step_beam"]


# ----------------------------------------------------------------- the driver
def _driver():
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    return drv


def _argv(tmp_path, sampler, extra=()):
    diff = yaml.load(open(os.path.join(ROOT, "configs", "diffusion_config.yaml")), Loader=yaml.FullLoader)
    diff["sampler"] = sampler
    dpath = tmp_path / "diffusion.yaml"
    yaml.dump(diff, open(dpath, "w"))
    return ["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config", str(dpath),
            "--task_config", os.path.join(ROOT, "configs", "gaussian_deblur_config.yaml"), "--save_dir",
            str(tmp_path / "out"), *extra]


def test_driver_beam_width_defaults_to_one():
    assert _driver().parse_args([]).beam_width == 1


@pytest.mark.parametrize("sampler,extra,env,message", [
    ("search_ddpm", ("--batch_size", "6", "--n_paths", "6", "--beam_width", "4"), {}, "does not divide --batch_size 6"),
    ("search_ddpm", ("--batch_size", "8", "--n_paths", "16", "--beam_width", "2"), {"WORLD_SIZE": "2"}, "WORLD_SIZE"),
    ("search_ddpm", ("--batch_size", "8", "--n_paths", "8", "--beam_width", "0"), {}, "at least 1"),
    ("ddpm", ("--batch_size", "8", "--n_paths", "8", "--beam_width", "2"), {}, "search_ddpm"),
])
def test_driver_rejects_a_bad_beam_width_before_gpu_work(tmp_path, monkeypatch, sampler, extra, env, message):
    drv = _driver()

    def no_gpu(*a, **kw):
        raise AssertionError("the driver touched the GPU before rejecting the arguments")
    for fn in ("is_available", "set_device", "device_count"):
        monkeypatch.setattr(torch.cuda, fn, no_gpu)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(SystemExit) as e:
        drv.main(_argv(tmp_path, sampler, extra))
    msg = str(e.value)
    assert message in msg and "--beam_width" in msg and "\n" not in msg
