#!/usr/bin/env python3
"""Generates tests/golden/unet.npz by IMPORTING THE REFERENCE'S nvsf/nerf/models/unet.py (read-only checkout, loaded by path) and
running it on CPU in evaluation mode with the weights of unet_params.py.  Run in the build container only:

    python tests/golden/golden_unet.py

Per shape of unet_params.SHAPES: the input, the fp32 output, `floor` = max |fp32 output - output of the same module in float64|,
and at 34 x 70 the attention block's output.  Only arrays and the digest of the weight bytes are written."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NVSF_REFERENCE", "/root/reference")
sys.path.insert(0, HERE)
import unet_params as P  # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("reference_unet", os.path.join(REF, "nvsf", "nerf", "models", "unet.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(0)
    net = ref.UNet(3, 32, 1).eval()
    digest = P.load_into(net)
    net64 = ref.UNet(3, 32, 1).double().eval()
    net64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in net.state_dict().items()})
    out = {"weights_sha256": np.array(digest)}
    for H, W in P.SHAPES:
        x = torch.from_numpy(P.unet_input(H, W))[None]
        grabbed = {}
        hook = net.attn.register_forward_hook(lambda m, i, o: grabbed.update(attn=o.detach().clone()))
        with torch.no_grad():
            y = net(x)
            y64 = net64(x.double())
        hook.remove()
        floor = float((y.double() - y64).abs().max())
        near = float(((y - 0.5).abs() < 1e-3).float().mean())
        print(f"{H} x {W}: floor {floor:.3e}, above 0.5: {float((y > 0.5).float().mean()):.4f}, min {float(y.min()):.4f}, "
              f"max {float(y.max()):.4f}, within 1e-3 of 0.5: {100 * near:.4f} %")
        assert near <= 1e-3, "too many probabilities sit on the threshold"
        tag = f"{H}x{W}"
        out[f"input_{tag}"] = x[0].numpy()
        out[f"output_{tag}"] = y[0, 0].numpy()
        out[f"floor_{tag}"] = np.array(floor, np.float64)
        if (H, W) == P.SHAPES[0]:
            out[f"attn_{tag}"] = grabbed["attn"][0].numpy()
    path = os.path.join(HERE, "unet.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
