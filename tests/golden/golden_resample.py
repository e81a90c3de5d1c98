"""Fixture generator for the inverse-CDF sampler: runs the reference's own `sample_pdf`
(nvsf/nerf/models/renderer_dynamic.py:8-52, imported from the reference tree with its import-only dependencies stubbed) on the CPU in
fp32 and writes tests/golden/resample.npz:

    python tests/golden/golden_resample.py

Inputs: 64 synthetic LiDAR rays per case.  Per ray `far` is drawn between 0.3 and 1.0 of the LiDAR range, z is the perturbed linspace
of NeRFRenderer.run, sigma is one Gaussian bump (centre anywhere on the ray, width 0.2 to 5 % of its length, peak exp(9 rand)) plus
0.3 rand haze per sample; the first eighth of the rays is empty, the next eighth is scaled by 1e-3.  The weights come from the
reference's compositing expressions (renderer_dynamic.py:181-194) in fp32; bins are the mid points and the pdf weights are
weights[:, 1:-1], as the hierarchical pass forms them.
Cases (nb - 1, U) in {(1, 5), (62, 16), (128, 128), (766, 64)}, each with det = True and det = False.  For det = False the draws are
stored: seed, torch.rand of the same shape, then reseed before the call into the reference.
Stored per case: bins, weights, u, samples (the reference's).  The generator asserts the two conditions of tests/test_resample_cpu.py
(the float64 oracle against these samples) before it writes.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_oracle as RO  # noqa: E402

SCALE = 0.010851959895748291  # nvsf/synthetic.py: the scene scale of the shipped configuration
MIN_NEAR, LIDAR_MAX_DEPTH = 1.0 * SCALE, 80.0 * SCALE

CASES = ((1, 5), (62, 16), (128, 128), (766, 64))
RAYS = 64


def load_reference_sample_pdf():
    class _Any(types.ModuleType):  # an import-only dependency: whatever is asked of it at import time is another stub
        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return _Any(k)

        def __call__(self, *a, **k):
            return self
    stubs = ("trimesh", "nvsf", "nvsf.nerf", "nvsf.nerf.raymarching")
    assert not any(name in sys.modules for name in stubs)
    for name in stubs:
        sys.modules[name] = _Any(name)
    spec = importlib.util.spec_from_file_location("_ref_renderer_dynamic", os.path.join(REF, "nvsf/nerf/models/renderer_dynamic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in stubs:
        del sys.modules[name]
    return mod.sample_pdf


def rays(T, gen):
    """z [RAYS, T] and compositing weights [RAYS, T], fp32 torch."""
    rand = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float32)
    near = torch.full((RAYS, 1), MIN_NEAR)
    far = near + (0.3 + 0.7 * rand(RAYS, 1)) * (LIDAR_MAX_DEPTH - MIN_NEAR)
    sample_dist = (far - near) / T
    z = near + (far - near) * torch.linspace(0.0, 1.0, T).unsqueeze(0)
    z = z + (rand(RAYS, T) - 0.5) * sample_dist
    centre = near + (far - near) * rand(RAYS, 1)
    width = (far - near) * (0.002 + 0.048 * rand(RAYS, 1))
    sigma = torch.exp(9.0 * rand(RAYS, 1)) * torch.exp(-0.5 * ((z - centre) / width) ** 2) + 0.3 * rand(RAYS, T)
    sigma[: RAYS // 8] = 0.0
    sigma[RAYS // 8: RAYS // 4] *= 1e-3
    deltas = torch.cat([z[:, 1:] - z[:, :-1], sample_dist], -1)
    alphas = 1 - torch.exp(-deltas * sigma)
    shifted = torch.cat([torch.ones_like(alphas[:, :1]), 1 - alphas + 1e-15], -1)
    return z, alphas * torch.cumprod(shifted, -1)[:, :-1]


def main():
    sample_pdf = load_reference_sample_pdf()
    out = {"cases": np.array(CASES, np.int32), "torch_version": np.array(torch.__version__)}
    for c, (nw, U) in enumerate(CASES):
        T = nw + 2
        z, weights = rays(T, torch.Generator().manual_seed(100 + c))
        bins = z[:, :-1] + 0.5 * (z[:, 1:] - z[:, :-1])
        w = weights[:, 1:-1].contiguous()
        assert bins.shape == (RAYS, nw + 1) and w.shape == (RAYS, nw)
        for det in (True, False):
            torch.manual_seed(7 + c)
            if det:
                u = torch.linspace(0.0 + 0.5 / U, 1.0 - 0.5 / U, steps=U)
            else:
                u = torch.rand([RAYS, U])
                torch.manual_seed(7 + c)  # the reference draws the same numbers again
            samples = sample_pdf(bins, w, U, det=det)
            assert samples.dtype == torch.float32 and samples.shape == (RAYS, U)
            width = ((bins[:, -1] - bins[:, 0]) / nw).double().numpy()[:, None]
            worst, share = RO.reference_conditions(RO.sample_pdf(bins.numpy(), w.numpy(), u.numpy()), samples.numpy(), width)
            print(f"(nb - 1, U) = ({nw}, {U}) det = {det}: float64 oracle against the reference: largest difference {worst:.3g} bin widths, "
                  f"share beyond 0.01 bin width {share:.3g}")
            assert worst <= 1.0 and share <= 1e-3, "change the inputs, not the cap"
            tag = f"c{c}_{'det' if det else 'rand'}_"
            out[tag + "u"] = u.numpy()
            out[tag + "samples"] = samples.numpy()
        out[f"c{c}_bins"] = bins.numpy()
        out[f"c{c}_weights"] = w.numpy()
    path = os.path.join(HERE, "resample.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
