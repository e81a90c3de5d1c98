"""Timing of the line-of-sight loss (`use_urf_loss`, trainer.py:276-294) and of the distortion loss (`distortion_loss`), alone and inside
the training step.

    python tools/bench_losses.py [--reps 20] [--steps 10] [--label NAME] [--out profiles/urf_loss_bench.json]

Legs, in milliseconds between device events on the current stream, median and min .. max of the repeats after warm-up:
  los_torch        `urf_line_of_sight_loss` on the device, forward + backward to the weights, at 4096 x 768 (the step's own size);
  los_kernel       `UrfLossFn` (nvsf_urf_loss_fwd / _bwd) on the same tensors, interleaved with the torch leg rep by rep so that a busy
                   neighbour hits both; absent on a tree without the kernel.  Per pair this leg pays a Function call, three small
                   allocations and three launches on the host, which is what bounds it;
  los_kernel_queued  the two entries called directly, 20 forward + backward pairs queued between one pair of events, per pair: the
                   kernels' own time.  `bandwidth_gb_s`: the bytes the pair must move -- weights and z_vals once forward, both again
                   plus the gradient backward, 5 x 4 N T bytes, and the N ranges twice -- over the median; `fraction_of_hbm_peak` the
                   same over 8 TB/s;
  step_urf / step  `RenderTrainStep.step` at the config-4 shape (4096 LiDAR + 4096 camera rays x 768 samples) with and without the
                   switch, interleaved.
  dist_torch / dist_kernel / dist_kernel_queued   the same three legs for the distortion loss: `distortion_loss` as torch expressions
                   against `DistortionLossFn` (nvsf_distortion_loss_fwd / _bwd), and the two entries called directly.  Bytes the pair
                   must move: the same 5 x 4 N T, plus the ranges twice, the row totals (16 N) written and read and the per-ray losses.
                   `over_los_pair`: its median over that of `los_kernel_queued` measured in the same run;
  step_dist        the config-4 step with `distortion_loss=True`, interleaved with the two above.
`--label` names the tree that was measured; with --out the result is merged into that file under the label, so that a run on the parent
commit (torch form inside the step) and one on the branch sit side by side.  `decided`: whether two medians differ by more than the two
spreads (max - min) combined.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nvsf import _hip, synthetic as S  # noqa: E402
from nvsf.nerf import losses as L  # noqa: E402
from nvsf.nerf.models.network_static import NeRFNetworkStatic  # noqa: E402
from nvsf.nerf.train_step import RenderTrainStep  # noqa: E402

HBM_PEAK = 8e12
N, T = 4096, 768
QUEUE = 20


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def interleaved(legs, reps, warmup=3):
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(event_ms(fn))
    return {k: stats(v) for k, v in times.items()}


def decided(a, b):
    return bool(abs(a["median"] - b["median"]) > (a["max"] - a["min"]) + (b["max"] - b["min"]))


def los_legs(dev, reps):
    g = torch.Generator().manual_seed(0)
    z = torch.sort(0.02 + 0.96 * torch.rand(N, T, generator=g), dim=1).values.to(dev)
    w = (torch.rand(N, T, generator=g) * 0.01).to(dev).requires_grad_()
    gt = (torch.rand(N, generator=g) * (torch.rand(N, generator=g) > 0.3)).to(dev).view(1, N)
    eps = 0.02

    def run(fn):
        def leg():
            (grad,) = torch.autograd.grad(fn(w, z, gt, eps), w)
            return grad
        return leg
    legs = {"los_torch": run(L.urf_line_of_sight_loss)}
    if hasattr(L, "UrfLossFn"):
        legs["los_kernel"] = run(L.UrfLossFn.apply)
    res = interleaved(legs, reps)
    if "los_kernel" in res:
        # the three launches alone, QUEUE pairs back to back between one pair of events: the autograd leg above is bound by the host's
        # launch rate (a Function call, three small allocations and three launches per pair), this one by the kernels
        wd, state, loss = w.detach(), torch.empty(2, dtype=torch.float64, device=dev), torch.empty((), device=dev)
        ws, grad, one = torch.empty(L.UrfLossFn.WS_BYTES // 8, dtype=torch.float64, device=dev), torch.empty_like(wd), torch.ones((), device=dev)
        hi = float(torch.tensor(eps, dtype=torch.float32))
        head = (_hip.ptr(wd), _hip.ptr(z), _hip.ptr(gt), N, T, hi, eps - hi)

        def queue():
            for _ in range(QUEUE):
                _hip.call("nvsf_urf_loss_fwd", *head, _hip.ptr(ws), L.UrfLossFn.WS_BYTES, _hip.ptr(loss), _hip.ptr(state))
                _hip.call("nvsf_urf_loss_bwd", *head, _hip.ptr(state), _hip.ptr(one), _hip.ptr(grad))
        res["los_kernel_queued"] = {k: v / QUEUE for k, v in interleaved({"q": queue}, reps)["q"].items()}
        moved = 5 * 4 * N * T + 2 * 4 * N
        sec = res["los_kernel_queued"]["median"] * 1e-3
        res["los_kernel_queued"].update(pairs_per_timing=QUEUE, bytes_moved=moved, bandwidth_gb_s=moved / sec / 1e9,
                                        fraction_of_hbm_peak=moved / sec / HBM_PEAK)
        res["torch_over_kernel"] = res["los_torch"]["median"] / res["los_kernel"]["median"]
        res["decided"] = decided(res["los_torch"], res["los_kernel"])
        a, b = legs["los_kernel"]().double(), legs["los_torch"]().double()
        res["kernel_vs_torch_max_abs_grad_diff"] = float((a - b).abs().max())
        res["kernel_minus_torch_loss"] = float(L.UrfLossFn.apply(w, z, gt, eps)) - float(L.urf_line_of_sight_loss(w, z, gt, eps))
    return res


def dist_legs(dev, reps, los_queued):
    g = torch.Generator().manual_seed(1)
    nears = (0.05 + 0.1 * torch.rand(N, generator=g)).to(dev)
    fars = nears + 1.0
    z = (nears.cpu()[:, None] + torch.sort(0.001 + 0.99 * torch.rand(N, T, generator=g), dim=1).values).to(dev)
    w = (torch.rand(N, T, generator=g) / T).to(dev).requires_grad_()
    alpha = 0.01

    def run(fn):
        def leg():
            (grad,) = torch.autograd.grad(fn(w, z, nears, fars, alpha), w)
            return grad
        return leg
    legs = {"dist_torch": run(L.distortion_loss), "dist_kernel": run(L.DistortionLossFn.apply)}
    res = interleaved(legs, reps)
    wd, state, loss, ray = w.detach(), torch.empty(N, 2, dtype=torch.float64, device=dev), torch.empty((), device=dev), torch.empty(N, device=dev)
    ws, grad, one = torch.empty((N + 3) // 4, dtype=torch.float64, device=dev), torch.empty_like(wd), torch.ones((), device=dev)
    head = (_hip.ptr(wd), _hip.ptr(z), _hip.ptr(nears), _hip.ptr(fars), N, T, alpha)

    def queue():
        for _ in range(QUEUE):
            _hip.call("nvsf_distortion_loss_fwd", *head, _hip.ptr(ws), 8 * ws.numel(), _hip.ptr(ray), _hip.ptr(loss), _hip.ptr(state))
            _hip.call("nvsf_distortion_loss_bwd", *head, _hip.ptr(state), _hip.ptr(one), _hip.ptr(grad))
    res["dist_kernel_queued"] = {k: v / QUEUE for k, v in interleaved({"q": queue}, reps)["q"].items()}
    moved = 5 * 4 * N * T + 2 * 2 * 4 * N + 2 * 16 * N + 4 * N
    sec = res["dist_kernel_queued"]["median"] * 1e-3
    res["dist_kernel_queued"].update(pairs_per_timing=QUEUE, bytes_moved=moved, bandwidth_gb_s=moved / sec / 1e9,
                                     fraction_of_hbm_peak=moved / sec / HBM_PEAK)
    if los_queued is not None:
        res["dist_kernel_queued"]["over_los_pair"] = res["dist_kernel_queued"]["median"] / los_queued["median"]
    res["torch_over_kernel"] = res["dist_torch"]["median"] / res["dist_kernel"]["median"]
    res["decided"] = decided(res["dist_torch"], res["dist_kernel"])
    a, b = legs["dist_kernel"]().double(), legs["dist_torch"]().double()
    res["kernel_vs_torch_max_abs_grad_diff"] = float((a - b).abs().max())
    res["kernel_minus_torch_loss"] = float(L.DistortionLossFn.apply(w, z, nears, fars, alpha)) - float(L.distortion_loss(w, z, nears, fars, alpha))
    return res


def step_legs(dev, reps):
    rng = np.random.default_rng(0)
    lo, ld = S.lidar_rays(N, rng)
    co, cd = S.camera_rays(N, rng)
    g = torch.Generator(device="cpu").manual_seed(3)
    batch = {"rays_o_lidar": torch.from_numpy(lo).to(dev)[None], "rays_d_lidar": torch.from_numpy(ld).to(dev)[None],
             "rays_o": torch.from_numpy(co).to(dev)[None], "rays_d": torch.from_numpy(cd).to(dev)[None], "time": torch.tensor([[0.5]], device=dev),
             "gt_depth": torch.rand(1, N, generator=g).to(dev) * 0.5, "gt_raydrop": (torch.rand(1, N, generator=g) > 0.3).float().to(dev),
             "gt_intensity": torch.rand(1, N, generator=g).to(dev), "gt_rgb": torch.rand(1, N, 3, generator=g).to(dev)}
    legs = {}
    for name, urf, dist in (("step_urf", True, False), ("step_dist", False, True), ("step", False, False)):
        torch.manual_seed(0)
        m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH,
                              num_frames=S.NUM_FRAMES).to(dev)
        step = RenderTrainStep(m, num_steps=T, scale=S.SCALE, use_urf_loss=urf, **({"distortion_loss": True} if dist else {}))

        def leg(step=step):
            step.step(batch)
            step.sync()
        legs[name] = leg
    res = interleaved(legs, reps, warmup=2)
    res["urf_costs_ms"] = res["step_urf"]["median"] - res["step"]["median"]
    res["decided"] = decided(res["step_urf"], res["step"])
    res["dist_costs_ms"] = res["step_dist"]["median"] - res["step"]["median"]
    res["dist_decided"] = decided(res["step_dist"], res["step"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"unit": "ms (device events)", "shape": [N, T], "reps": args.reps, "steps": args.steps, "device": torch.cuda.get_device_name(0),
           "build_digest": _hip.build_digest(), "los": los_legs(dev, args.reps)}
    res["dist"] = dist_legs(dev, args.reps, res["los"].get("los_kernel_queued"))
    res["train_step"] = step_legs(dev, args.steps)
    print(json.dumps({args.label: res}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
        merged[args.label] = res
        with open(args.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()
