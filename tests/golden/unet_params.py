"""Deterministic U-Net weights and inputs shared by the fixture generator (golden_unet.py) and the tests, so the 6.5 M parameters
are never stored (the job param_init.py does for the fields).  Seeded numpy PCG64, key by key in sorted order:
  convolution weights   N(0, 2 / fan_in)  (He); the final 1 x 1 weight x 4, so the probabilities spread
  convolution biases    N(0, 0.1)
  BatchNorm weight and running variance   U(0.5, 1.5)
  BatchNorm bias and running mean         N(0, 0.1)
"""
import hashlib

import numpy as np

SHAPES = ((34, 70), (66, 1030))  # 34 x 70: the smallest whose chain is odd at two levels of both axes (34 17 8 4 2, 70 35 17 8 4)


def unet_state(shapes, seed=0):
    """shapes: {state-dict key: shape} of UNet(3, 32, 1).  Returns {key: fp32 / int64 array}."""
    rng = np.random.default_rng(7001 + seed)
    out = {}
    for key in sorted(shapes):
        shape = tuple(shapes[key])
        if key.endswith("num_batches_tracked"):
            out[key] = np.zeros(shape, np.int64)
        elif len(shape) == 4:
            w = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
            out[key] = (w * (4.0 if key == "outc.conv.2.weight" else 1.0)).astype(np.float32)
        elif key.endswith("running_var") or (key.endswith("weight") and len(shape) == 1):
            out[key] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        else:  # BatchNorm bias / running mean, convolution bias
            out[key] = (rng.standard_normal(shape) * 0.1).astype(np.float32)
    return out


def state_digest(state):
    h = hashlib.sha256()
    for key in sorted(state):
        h.update(key.encode())
        h.update(np.ascontiguousarray(state[key]).tobytes())
    return h.hexdigest()


def unet_input(H, W, seed=0):
    """[3, H, W] fp32: ray-drop and intensity U(0, 1), range U(0, 0.87) with about 30 % of the pixels 0."""
    rng = np.random.default_rng(7100 + seed)
    x = rng.uniform(0.0, 1.0, (3, H, W))
    x[2] *= 0.87
    x[2][rng.uniform(0.0, 1.0, (H, W)) < 0.3] = 0.0
    return x.astype(np.float32)


def load_into(module, seed=0):
    """Fills a torch module from the recipe (strict); returns the digest of the weight bytes."""
    import torch
    state = unet_state({k: tuple(v.shape) for k, v in module.state_dict().items()}, seed)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return state_digest(state)
