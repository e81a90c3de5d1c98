"""Stage-by-stage reference of the ray-drop refinement U-Net for tests/test_unet_stages_gpu.py (a plain helper: no fixtures, no GPU).

The oracle is the project's torch module (nvsf/nerf/models/unet.py, pinned to the reference's own module by test_unet_cpu.py) on the CPU,
with forward hooks that capture the 13 tensors nvsf_unet_forward leaves in its workspace (nvsf_unet_layout's rows), the logit and the
probability.  Run in float64 it is the reference; run in float32 it gives, per stage, the error of one plain fp32 evaluation:
`floor_stage` = max |fp32 module - fp64 module|.  Both come from the recipe of tests/golden/unet_params.py at run time; nothing is stored.
"""
import functools
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import unet_params as P  # noqa: E402

# workspace tensor (row order of nvsf_unet_layout) -> the module whose output it is; `att` is the return value of attn.attend
STAGES = ("x0", "x1", "x2", "x3", "x4", "mid", "qkv", "att", "x4a", "u0", "u1", "u2", "u3")
HOOKED = {"x0": "inc", "x1": "down1", "x2": "down2", "x3": "down3", "x4": "down4", "mid": "up4.conv.double_conv.3", "qkv": "attn.proj_qkv",
          "x4a": "attn", "u0": "up1", "u1": "up2", "u2": "up3", "u3": "up4", "logit": "outc"}
OUTPUTS = STAGES + ("logit", "prob")
LOGIT_BAND = (0.02, 0.98)  # the head is compared on logits where the fp64 probability lies strictly inside this band
BAND_MIN_KEPT = 0.4        # ... which has to keep at least this fraction of the pixels

# (H, W): what the shape is the smallest for.  Bottom grid = (H // 16, W // 16), N = its pixels = the attention's keys.
SHAPES = (
    (16, 16),    # 1 x 1, N = 1: minimum size, one-key softmax, Hs = Ws = 1 upsample (sy = sx = 0), every level narrower than a 32-column tile
    (31, 47),    # 1 x 2, N = 2: odd at all four levels of both axes (31 15 7 3 1, 47 23 11 5 2): the zero-padded last row / column at every Up
    (48, 176),   # 3 x 11, N = 33: one full key block + a one-key tail; a second query block with one live lane
    (16, 528),   # 1 x 33, N = 33: the same tail with H4 = 1
    (32, 512),   # 2 x 32, N = 64: two full key blocks, no tail: the running maximum rescaled with no masking
    (2048, 16),  # 128 x 1, N = 128: the 64-channel workgroup form of k_conv in its pool, plain, 1 x 1 and up-cat modes
)
WEIGHT_SEEDS = (0, 1)        # of the stage-by-stage comparison
INPUT_SEED = 0
# The weight draws of the logit comparison.  Which pixels saturate is decided by the weights, not by the input (i.i.d. noise: the kept
# fraction moves by < 0.07 over input seeds 0 .. 7), and draw 0 keeps only 9 % at 48 x 176, 12 % at 32 x 512 and 39 % at 2048 x 16.  Of
# the draws 0 .. 7, 1, 6 and 7 keep >= 40 % at every shape (1: 42 - 67 %, 6: 82 - 94 %); test_unet_cpu.py asserts it for the two used.
LOGIT_WEIGHT_SEEDS = (1, 6)


def run_stages(H, W, weight_seed=0, input_seed=0, dtype=torch.float64):
    """{name: [C, h, w] tensor of `dtype`} for OUTPUTS, of the module with unet_params.load_into(seed=weight_seed) on
    unet_params.unet_input(H, W, input_seed)."""
    from nvsf.nerf.models.unet import UNet
    net = UNet().eval()
    P.load_into(net, weight_seed)
    net = net.to(dtype)
    got = {}
    mods = dict(net.named_modules())
    for name, path in HOOKED.items():
        mods[path].register_forward_hook(lambda m, i, o, name=name: got.__setitem__(name, o.detach()[0].clone()))
    attend = net.attn.attend

    def attend_and_keep(x):
        h = attend(x)
        got["att"] = h.detach()[0].contiguous().clone()  # a permuted view of [H, W, C]: made dense [C, H, W] here
        return h

    net.attn.attend = attend_and_keep
    with torch.no_grad():
        got["prob"] = net(torch.from_numpy(P.unet_input(H, W, input_seed))[None].to(dtype))[0].clone()
    assert set(got) == set(OUTPUTS)
    return got


def logit_of(p):
    """log(p / (1 - p)) in float64 of a probability of any float type."""
    p = p.double()
    return torch.log(p) - torch.log1p(-p)


@functools.lru_cache(maxsize=None)
def reference(H, W, weight_seed=0, input_seed=0):
    """(ref, floor, band): ref = run_stages in float64; floor[name] = max |fp32 module - fp64 module| for OUTPUTS and for "band_logit";
    band = the pixels [1, H, W] with LOGIT_BAND[0] < ref prob < LOGIT_BAND[1].  ref["band_logit"] = logit_of(ref prob): the head's
    quantity is the logit recovered from a probability, so its fp32 evaluation is logit_of(the fp32 module's probability), the rounding
    of that probability to fp32 included, compared inside the band only.  Computed once per case and shared: do not modify."""
    ref, f32 = run_stages(H, W, weight_seed, input_seed, torch.float64), run_stages(H, W, weight_seed, input_seed, torch.float32)
    floor = {name: float((f32[name].double() - ref[name]).abs().max()) for name in OUTPUTS}
    band = (ref["prob"] > LOGIT_BAND[0]) & (ref["prob"] < LOGIT_BAND[1])
    ref["band_logit"] = logit_of(ref["prob"])
    floor["band_logit"] = float((logit_of(f32["prob"]) - ref["band_logit"])[band].abs().max()) if bool(band.any()) else 0.0
    return ref, floor, band
