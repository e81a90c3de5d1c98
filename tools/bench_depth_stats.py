"""Timing of the depth statistics (`ops.ray_depth_stats`, nvsf_ray_depth_stats_fwd / nvsf_ray_depth_quantile_bwd),
alone and inside one whole-frame evaluation render.

    python tools/bench_depth_stats.py [--reps 20] [--frames 5] [--label NAME] [--out profiles/depth_stats_bench.json]

Timing discipline of tools/bench_losses.py: milliseconds between device events on the current stream, median and min .. max of the
repeats after warm-up, the legs of a comparison interleaved rep by rep so that a busy neighbour hits both; `decided`: whether two
medians differ by more than the two spreads (max - min) combined.  Per shape (4096 x 768, the shipped batch, and 4096 x 832, its
hierarchical rows T + U):
  median_torch       the median range as torch expressions on the device: float64 cumsum of the weights, searchsorted of W / 2, gathers of
                     the crossing sample's depth, interval, weight and prefix, the interpolation (no mode, no spread);
  median_kernel      `ops.ray_depth_stats(..., q=(0.5,), want=("quantiles",))`: one launch and one small allocation;
  all_kernel         the same call with four levels, the strongest return and the spread;
  kernel_queued      the forward entry alone, 20 launches queued between one pair of events, per launch: the kernel's own time.
                     `bandwidth_gb_s`: the bytes a call must move -- weights and z_vals once, 2 x 4 N T, the second walk is served by the
                     cache -- over the median; `fraction_of_hbm_peak` the same over 8 TB/s;
  pair_queued        forward with state + backward (nvsf_ray_depth_quantile_bwd), 20 pairs queued, per pair; bytes: the two rows twice and
                     the gradient row once, 5 x 4 N T.
`frame`: the staged LiDAR render of one whole range image (66 x 1030 rays in chunks of 4096, 768 samples; and 768 + 64 resampled) of a
static field with depth_mode "mean", "median" and "mode", interleaved: what the switch costs an evaluation.
`--label` names the tree that was measured; with --out the result is merged into that file under the label.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nvsf import _hip, field_ops as ops, synthetic as S  # noqa: E402
from nvsf.nerf.models.network_static import NeRFNetworkStatic  # noqa: E402

HBM_PEAK = 8e12
SHAPES = ((4096, 768), (4096, 832))
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


def median_torch(w, z, nears, fars):
    """The normalised median of section 9n as torch expressions (cumsum, searchsorted, gather), float64 sums as the kernel's."""
    N, T = w.shape
    C = torch.cumsum(w.double(), dim=1)
    W = C[:, -1:]
    tau = 0.5 * W
    i = torch.searchsorted(C, tau).clamp(max=T - 1)  # the first i with C_i >= tau
    delta = torch.cat([z[:, 1:] - z[:, :-1], ((fars - nears) / T)[:, None]], dim=1).double()
    prev = torch.where(i > 0, C.gather(1, (i - 1).clamp(min=0)), torch.zeros_like(tau))
    wi = w.gather(1, i).double()
    t = z.gather(1, i).double() + delta.gather(1, i) * (tau - prev) / wi.clamp(min=1e-300)
    return torch.where(W > 0, t, torch.zeros_like(t))[:, 0].float()


def rows(N, T, dev):
    """weights of the compositor on a smooth random density with one or two bumps per ray, depths of the uniform sampler"""
    g = torch.Generator().manual_seed(T)
    nears = torch.full((N,), float(S.MIN_NEAR)).to(dev)
    fars = torch.full((N,), float(S.LIDAR_MAX_DEPTH)).to(dev)
    u = (torch.arange(T, dtype=torch.float32)[None, :] + torch.rand(N, T, generator=g)) / T
    z = (float(S.MIN_NEAR) + (float(S.LIDAR_MAX_DEPTH) - float(S.MIN_NEAR)) * u).to(dev)
    centre, second = torch.rand(N, 1, generator=g), torch.rand(N, 1, generator=g)
    sigma = 300.0 * torch.exp(-0.5 * ((u - centre) / 0.01) ** 2) + 200.0 * torch.exp(-0.5 * ((u - second) / 0.02) ** 2) + 0.05
    w = ops.CompositeWeightsFn.apply(sigma.to(dev), z, nears, fars, 1.0)[0]
    return w, z, nears, fars


def shape_legs(N, T, dev, reps):
    w, z, nears, fars = rows(N, T, dev)
    four = (0.05, 0.25, 0.5, 0.95)
    legs = {"median_torch": lambda: median_torch(w, z, nears, fars),
            "median_kernel": lambda: ops.ray_depth_stats(w, z, nears, fars, (0.5,), True, ("quantiles",)),
            "all_kernel": lambda: ops.ray_depth_stats(w, z, nears, fars, four, True)}
    res = interleaved(legs, reps)
    q, mode, std = torch.empty(N, 1, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    state, grad, gq = torch.empty(N, 1, 2, dtype=torch.float64, device=dev), torch.empty_like(w), torch.ones(N, 1, device=dev)
    head = (_hip.ptr(w), _hip.ptr(z), _hip.ptr(nears), _hip.ptr(fars), N, T, _hip.host_f64((0.5,)), 1, 1)

    def queue_fwd():
        for _ in range(QUEUE):
            _hip.call("nvsf_ray_depth_stats_fwd", *head, _hip.ptr(q), _hip.ptr(mode), _hip.ptr(std), None)

    def queue_pair():
        for _ in range(QUEUE):
            _hip.call("nvsf_ray_depth_stats_fwd", *head, _hip.ptr(q), None, None, _hip.ptr(state))
            _hip.call("nvsf_ray_depth_quantile_bwd", *head, _hip.ptr(state), _hip.ptr(gq), _hip.ptr(grad))
    for name, fn, moved in (("kernel_queued", queue_fwd, 2 * 4 * N * T + 5 * 4 * N), ("pair_queued", queue_pair, 5 * 4 * N * T + 4 * 4 * N + 2 * 16 * N)):
        r = {k: v / QUEUE for k, v in interleaved({"q": fn}, reps)["q"].items()}
        sec = r["median"] * 1e-3
        r.update(launches_per_timing=QUEUE, bytes_moved=moved, bandwidth_gb_s=moved / sec / 1e9, fraction_of_hbm_peak=moved / sec / HBM_PEAK)
        res[name] = r
    res["torch_over_kernel"] = res["median_torch"]["median"] / res["median_kernel"]["median"]
    res["decided"] = decided(res["median_torch"], res["median_kernel"])
    res["kernel_vs_torch_max_abs_diff"] = float((legs["median_kernel"]()["quantiles"][:, 0].double() - legs["median_torch"]().double()).abs().max())
    return res


def frame_legs(dev, reps):
    H, W = S.LIDAR_HW
    o, d = S.lidar_rays(H * W, np.random.default_rng(0))
    o, d, t = torch.from_numpy(o).to(dev)[None], torch.from_numpy(d).to(dev)[None], torch.tensor([[0.5]], device=dev)
    torch.manual_seed(0)
    m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH, num_frames=S.NUM_FRAMES).to(dev).eval()
    out = {"rays": H * W, "max_ray_batch": 4096}
    for name, kw in (("T768", dict(num_steps=768)), ("T768+U64", dict(num_steps=768, upsample_steps=64, hierarchical=True))):
        def leg(mode, kw=kw):
            def run():
                with torch.no_grad():
                    m.render(o, d, t, cal_lidar_color=True, staged=True, max_ray_batch=4096, depth_mode=mode, **kw)
            return run
        res = interleaved({mode: leg(mode) for mode in ("mean", "median", "mode")}, reps, warmup=2)
        res["median_costs_ms"] = res["median"]["median"] - res["mean"]["median"]
        res["median_decided"] = decided(res["median"], res["mean"])
        res["mode_costs_ms"] = res["mode"]["median"] - res["mean"]["median"]
        res["launches_added"] = -(-H * W // 4096)
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"unit": "ms (device events)", "reps": args.reps, "frames": args.frames, "device": torch.cuda.get_device_name(0),
           "build_digest": _hip.build_digest()}
    for N, T in SHAPES:
        res[f"{N}x{T}"] = shape_legs(N, T, dev, args.reps)
    res["frame"] = frame_legs(dev, args.frames)
    print(json.dumps({args.label: res}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
        merged[args.label] = res
        with open(args.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()
