"""CPU suite: multi-image batches (M images x K particles per sampler call) -- the C ABI's new entry points, the driver's
batching of --ref_image_idxs and the combinations it rejects before any GPU work."""
import os
import re
import sys

import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dpsx_op_create_mask_n", "dpsx_argmin_seg_f32", "dpsx_search_step_seg_f32",
               "dpsx_search_step_one_seg_f32")


def test_header_declares_and_lib_binds_the_multi_image_entry_points():
    from dps_ttc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dpsx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
    # the segmented search steps take the arguments of the unsegmented ones plus the segment count
    for base in ("dpsx_search_step_f32", "dpsx_search_step_one_f32"):
        seg = base.replace("_f32", "_seg_f32")
        assert len(_lib.SIGNATURES[seg][1]) == len(_lib.SIGNATURES[base][1]) + 1
    assert len(_lib.SIGNATURES["dpsx_op_create_mask_n"][1]) == len(_lib.SIGNATURES["dpsx_op_create_mask"][1]) + 1
    # the measurement rule is "y_n divides n" now, no longer y_n in {1, n}
    assert "{1, n}" not in hdr


def _driver():
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    return drv


def test_image_batches_keep_pick_order_with_a_ragged_tail():
    drv = _driver()
    assert drv.image_batches([4, 0, 7, 2, 9], 2) == [[4, 0], [7, 2], [9]]
    assert drv.image_batches([4, 0, 7], 3) == [[4, 0, 7]]
    assert drv.image_batches([4, 0, 7], 8) == [[4, 0, 7]]
    assert drv.image_batches([4, 0, 7], 1) == [[4], [0], [7]]
    assert drv.parse_args([]).images_per_batch == 1


def _argv(tmp_path, sampler, extra=()):
    diff = yaml.load(open(os.path.join(ROOT, "configs", "diffusion_config.yaml")), Loader=yaml.FullLoader)
    diff["sampler"] = sampler
    dpath = tmp_path / "diffusion.yaml"
    yaml.dump(diff, open(dpath, "w"))
    return ["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config", str(dpath),
            "--task_config", os.path.join(ROOT, "configs", "gaussian_deblur_config.yaml"), "--save_dir",
            str(tmp_path / "out"), "--ref_image_idxs", "0,1,2", "--images_per_batch", "2", *extra]


@pytest.mark.parametrize("sampler,extra,env,message", [
    ("ddpm", (), {"WORLD_SIZE": "2"}, "WORLD_SIZE"),
    ("ttc_ddim", (), {}, "ttc_ddim"),
    ("ddpm", ("--embedder", "standin:toy_embedder"), {}, "--embedder"),
    ("search_ddpm", ("--images_per_batch", "0"), {}, "at least 1"),
])
def test_driver_rejects_unsupported_combinations_before_gpu_work(tmp_path, monkeypatch, sampler, extra, env, message):
    import torch
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
    assert message in msg and "\n" not in msg
