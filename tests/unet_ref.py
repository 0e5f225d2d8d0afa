"""Shared by tests/golden/make_golden.py and tests/test_unet_{cpu,gpu}.py: the denoiser's parity cases.

No checkpoint is available offline, so the product's UNet (dps_ttc_amd/unet.py) is pinned to the reference's
architecture under SHARED SYNTHETIC WEIGHTS: `fill_weights` writes the same seeded numbers into any module that has
the reference's parameter names -- the generator fills the reference's model with it, the tests fill the product's.
The fixture (tests/golden/unet.npz) therefore carries no weights, only results.

To stay a small committed file it carries no inputs either: `inputs(name)` rebuilds x, t, w (and the labels) from
numpy's MT19937 `RandomState`, whose stream is the same on every platform; the fixture stores their CRC-32 so a
drift would be noticed.  Results of 32 x 32 variants are stored whole; larger result tensors are stored at
`SUBSET` seeded positions (`subset_index`), and rel-L2 is taken over those positions.
"""
import os
import zlib

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5            # the suite's gate for outputs and gradients (tests/test_hip_parity.py)
SUBSET = 8192         # stored positions per result tensor larger than a 32 x 32 variant's
WEIGHT_SEED = 2024

_BASE = dict(image_size=32, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="16,8")
_FFHQ_FLAGS = dict(num_head_channels=16, use_scale_shift_norm=True, resblock_updown=True, learn_sigma=True)

VARIANTS = {
    # FFHQ-like flags on a three-level net: attention at 16 x 16 and 8 x 8, head count from the head width
    "A": dict(_BASE, **_FFHQ_FLAGS),
    # every flag off: fixed head count, convolutional Down/Upsample, additive embedding, three output channels
    "B": dict(_BASE, num_heads=2),
    # [q | k | v] attention order, and other head counts on the way up than on the way down
    "C": dict(_BASE, use_new_attention_order=True, num_heads=2, num_heads_upsample=4),
    # class-conditional
    "D": dict(_BASE, class_cond=True, **_FFHQ_FLAGS),
    # the size table (1, 2, 3, 4), two ResBlocks per level, a 96-channel level (three 32-wide heads)
    "E": dict(image_size=64, num_channels=32, num_res_blocks=2, channel_mult="", attention_resolutions="8",
              num_head_channels=32, use_scale_shift_norm=True, resblock_updown=True),
    # A at 64 x 64 with the same down-sampling factors: the denoiser of the conditioning-call and loop tests
    "A64": dict(_BASE, **_FFHQ_FLAGS, image_size=64, attention_resolutions="32,16"),
}
LABELS = {"D": [1, 5]}
CPU_VARIANTS = tuple(VARIANTS)          # FFHQ (below) is GPU only
T = [250.0, 3.0]


def ffhq_config():
    """configs/model_config.yaml as shipped, without the checkpoint path"""
    with open(os.path.join(ROOT, "configs", "model_config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.pop("model_path", None)
    return cfg


def config(name):
    return ffhq_config() if name == "FFHQ" else dict(VARIANTS[name])


def cpu_build():
    """what decides how the CPU libraries round: the torch build, the vector capability it dispatches on, the CPU model"""
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            model = next((line.split(":", 1)[1].strip() for line in f if line.startswith("model name")), "")
    except OSError:
        pass
    return [torch.__version__, torch.backends.cpu.get_cpu_capability(), model]


def crc(a):
    return np.int64(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def fill_weights(model, seed=WEIGHT_SEED):
    """Seeded fill of every entry of `state_dict()`, the zero-initialised modules (proj_out, the last out_layers
    convolution, out.2) included so that they are exercised.  Each tensor depends on its key and shape alone."""
    sd = model.state_dict()
    for key in sorted(sd):
        ref = sd[key]
        z = np.random.RandomState((zlib.crc32(key.encode()) ^ seed) & 0x7fffffff).randn(*ref.shape)
        if ref.dim() >= 2:
            z = z / np.sqrt(np.prod(ref.shape[1:]))           # fan-in
        elif key.endswith(".weight"):
            z = 1.0 + 0.1 * z                                 # norm gains
        else:
            z = 0.1 * z                                       # biases
        sd[key] = torch.from_numpy(z).to(ref.dtype)
    model.load_state_dict(sd)
    return model


def inputs(name, n=None):
    """x [n, 3, S, S], t [n], cotangent w [n, C_out, S, S], labels or None -- numpy, fp32"""
    cfg = config(name)
    s = cfg["image_size"]
    n = n or (1 if name == "FFHQ" else 2)
    rng = np.random.RandomState(zlib.crc32(("in." + name).encode()) & 0x7fffffff)
    x = rng.randn(n, 3, s, s).astype(np.float32)
    w = rng.randn(n, 6 if cfg.get("learn_sigma") else 3, s, s).astype(np.float32)
    t = np.asarray((T * n)[:n], dtype=np.float32)
    labels = np.asarray((LABELS[name] * n)[:n], dtype=np.int64) if name in LABELS else None
    return x, t, w, labels


def stored_whole(name):
    return config(name)["image_size"] <= 32


def subset_index(tag, numel):
    """SUBSET distinct flat positions, the same in the generator and the tests"""
    rng = np.random.RandomState(zlib.crc32(("idx." + tag).encode()) & 0x7fffffff)
    return np.sort(rng.choice(numel, size=min(SUBSET, numel), replace=False))


def pick(tag, a, whole=False):
    """the part of result `a` that the fixture stores under `tag`"""
    a = np.asarray(a)
    return a if whole else a.reshape(-1)[subset_index(tag, a.size)]


def forward_and_vjp(model, x, t, w, labels=None):
    """y = model(x, t) and the VJP of sum(w * y) with respect to x (tensors on the model's device)"""
    x = x.detach().clone().requires_grad_()
    y = model(x, t) if labels is None else model(x, t, y=labels)
    (g,) = torch.autograd.grad((y * w).sum(), x)
    return y.detach(), g.detach()


# ---- the conditioning call with a real denoiser (A64, Gaussian blur 61 / sigma 3, 64 x 64, N = 2, ps scale 0.3)
CALL = dict(variant="A64", hw=64, n=2, scale=0.3, sigma=0.05, ts=(500, 0))
CALL_FIELDS = ("x0_hat", "sample", "ret0", "ret1")


def call_seed(t):
    return 1000 + t


def call_inputs(t):
    """truth [1, 3, hw, hw] in (-1, 1), measurement noise, x_prev [n, 3, hw, hw], and the step noise: the reference's
    p_sample draws it with `randn_like` from torch's global CPU generator, seeded with call_seed(t) just before"""
    hw, n = CALL["hw"], CALL["n"]
    rng = np.random.RandomState(zlib.crc32(b"call") & 0x7fffffff)
    truth = (rng.rand(1, 3, hw, hw) * 2 - 1).astype(np.float32)
    ynoise = rng.randn(1, 3, hw, hw).astype(np.float32)
    rng = np.random.RandomState(zlib.crc32(b"call.t%d" % t) & 0x7fffffff)
    x_prev = rng.randn(n, 3, hw, hw).astype(np.float32)
    noise = torch.randn(n, 3, hw, hw, generator=torch.Generator().manual_seed(call_seed(t))).numpy()
    return truth, ynoise, x_prev, noise
