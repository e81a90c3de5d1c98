"""Timing of the U-Net ray-drop refinement's forward (nvsf/nerf/refine.py, csrc/unet.hip).

    python tools/bench_unet.py [--reps 20] [--out profiles/unet_bench.json]

One 66 x 1030 frame (tests/golden/unet_params.py: the recipe's weights and input).  The HIP forward (probability + gated intensity and
range, 21 launches) against the torch module's evaluation-mode forward on the same device followed by the same gate (PyTorch-ROCm's own
convolutions, TF32 off: fp32 like the kernels).  The two are interleaved rep by rep, so that a busy neighbour hits both; median and
min .. max of --reps runs after warm-up, milliseconds between device events.  `decided`: whether the medians differ by more than the two
spreads combined.  `fraction_of_fp32_matrix_peak`: the network's multiply-adds (counted from the layer shapes, convolutions and the two
attention products) x 2 / median / 157.3 TFLOP/s.  `multiply_adds` lists them per layer, so that a kernel trace's per-launch times
(rocprofv3 --kernel-trace over this tool) turn into per-layer fractions; DESIGN.md section 9g quotes the largest convolution's.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import unet_params as P  # noqa: E402
from nvsf import _hip  # noqa: E402
from nvsf.nerf.refine import RaydropRefiner  # noqa: E402

MATRIX_PEAK = 157.3e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def versus(kernel, yard, reps):
    for _ in range(3):
        kernel(), yard()
    torch.cuda.synchronize()
    tk, ty = [], []
    for _ in range(reps):
        tk.append(event_ms(kernel))
        ty.append(event_ms(yard))
    k, y = stats(tk), stats(ty)
    spreads = (k["max"] - k["min"]) + (y["max"] - y["min"])
    return {"kernel_ms": k, "yardstick_ms": y, "yardstick_over_kernel": y["median"] / k["median"],
            "decided": bool(abs(y["median"] - k["median"]) > spreads)}


def multiply_adds(H, W):
    """Per layer, from the shapes: (name, multiply-adds)."""
    hs, ws = [H], [W]
    for _ in range(4):
        hs.append(hs[-1] // 2)
        ws.append(ws[-1] // 2)
    px = [h * w for h, w in zip(hs, ws)]
    c = [32, 64, 128, 256, 256]
    rows = [("inc", px[0] * 3 * 32)]
    for l in range(1, 5):
        rows += [(f"down{l}.a", px[l] * 9 * c[l - 1] * c[l]), (f"down{l}.b", px[l] * 9 * c[l] * c[l])]
    n = px[4]
    rows += [("attn.qkv", n * 256 * 768), ("attn.qk", 8 * n * n * 32), ("attn.pv", 8 * n * n * 32), ("attn.proj", n * 256 * 256)]
    for i, (cin, cout) in enumerate(((512, 128), (256, 64), (128, 32), (64, 32))):
        rows += [(f"up{i + 1}.a", px[3 - i] * 9 * cin * cin), (f"up{i + 1}.b", px[3 - i] * 9 * cin * cout)]
    rows.append(("outc", px[0] * 32))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    H, W = 66, 1030
    r = RaydropRefiner(dev)
    P.load_into(r.unet)
    r.repack()
    x = torch.from_numpy(P.unet_input(H, W)).to(dev)
    macs = multiply_adds(H, W)
    total = sum(m for _, m in macs)
    res = {"unit": "ms (device events)", "reps": args.reps, "frame": [H, W], "gflop": 2e-9 * total}
    leg = versus(lambda: r(x[0], x[1], x[2], thres=0.5), lambda: r.torch_forward(x[0], x[1], x[2], thres=0.5), args.reps)
    leg["fraction_of_fp32_matrix_peak"] = 2.0 * total / (leg["kernel_ms"]["median"] * 1e-3) / MATRIX_PEAK
    leg["yardstick_fraction_of_fp32_matrix_peak"] = 2.0 * total / (leg["yardstick_ms"]["median"] * 1e-3) / MATRIX_PEAK
    p, want = r(x[0], x[1], x[2]), r.torch_forward(x[0], x[1], x[2])
    leg["max_abs_kernel_minus_torch"] = float((p - want).abs().max())
    res["forward"] = leg
    res["multiply_adds"] = {k: int(v) for k, v in macs}
    res["device"] = torch.cuda.get_device_name(0)
    res["build_digest"] = _hip.build_digest()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
