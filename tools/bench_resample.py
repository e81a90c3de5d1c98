"""Timing record of the hierarchical importance resampling (csrc/resample.hip, NeRFRenderer.run(hierarchical=True)); no bar.

    python tools/bench_resample.py [--reps 20] [--rays 4096] [--out profiles/resample_bench.json]

4096 LiDAR rays on the config-2 static field (bench.py's model; the hash tables drawn from N(0, 0.5) as __graft_entry__.smoke() does,
so that the density has structure to resample), under no_grad.  Every figure is the median and min .. max of --reps runs after three
warm-up runs, in milliseconds between device events on the current stream (tools/bench_depth_image.py: event_ms, stats); the legs of
one group are interleaved rep by rep.  Legs:
  resample_merge   nvsf_resample_merge alone (steps 2-4: bins, cdf, draws, sort, merge, positions), per (T, U), shared u and per-ray u;
  merge_rows       the row merges of one hierarchical render: sigma (4 B rows), geo_feat (fp32 x 15, 60 B rows), positions (12 B rows);
  run_hier         the whole run(hierarchical=True) at (T, U) = (768, 128), (192, 64), (96, 32);
  run_chain_768    the operator-chain run at 768 even samples (the fused renders switched off for the call);
  run_fused_768    the fused one-launch render at 768 even samples (what run does by default under no_grad).
For each render setting `range_mae` is the mean absolute range difference against a 4096-sample even render of the same field through
the operator chain, in scene units and in metres.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_depth_image import event_ms, stats  # noqa: E402
from nvsf import _hip, field_ops as ops, synthetic as S  # noqa: E402
from nvsf.nerf.models.network_static import NeRFNetworkStatic  # noqa: E402

SETTINGS = ((768, 128), (192, 64), (96, 32))


def interleaved(legs, reps, warm=3):
    """{name: fn} -> {name: stats}, the legs run one after the other inside every rep."""
    for _ in range(warm):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(event_ms(fn))
    return {k: stats(v) for k, v in times.items()}


class _ChainOnly:
    """Switches the fused renders of a model off for the calls inside: run then takes the operator chain."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.model.fused_uniform_render, self.model.fused_train_forward = None, False

    def __exit__(self, *exc):
        del self.model.fused_uniform_render, self.model.fused_train_forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH,
                          num_frames=S.NUM_FRAMES)
    with torch.no_grad():
        m.hash_encoder_lidar.params.normal_(0.0, 0.5)
    m = m.to(dev).eval()
    N = args.rays
    o, d = S.lidar_rays(N, np.random.default_rng(1000))
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    t = torch.tensor([[0.5]], device=dev)
    res = {"unit": "ms (device events)", "rays": N, "reps": args.reps, "device": torch.cuda.get_device_name(0), "build_digest": _hip.build_digest()}

    def run(**kw):
        return m.run(o[None], d[None], t, cal_lidar_color=True, perturb=False, **kw)

    with torch.no_grad():
        # the kernels alone, on the coarse pass of each setting
        nears, fars = m._near_far(o, d, True, m.aabb_infer)
        res["resample_merge"], res["merge_rows"] = {}, {}
        for T, U in SETTINGS:
            z, xyz = ops.uniform_samples(o, d, nears, fars, T, m.aabb_infer, None)
            dens = m.density(xyz.view(-1, 3), t, True)
            w = ops.CompositeWeightsFn.apply(dens["sigma"].view(N, T), z, nears, fars, m._k_scale())[0]
            u_shared, u_rays = ops.stratified_u(U, dev), torch.rand(N, U, device=dev)
            res["resample_merge"][f"T{T}_U{U}"] = interleaved({
                "shared_u": lambda: ops.resample_merge(o, d, m.aabb_infer, z, w, u_shared),
                "per_ray_u": lambda: ops.resample_merge(o, d, m.aabb_infer, z, w, u_rays)}, args.reps)
            _, xyz_new, _, src = ops.resample_merge(o, d, m.aabb_infer, z, w, u_shared)
            fine = m.density(xyz_new.view(-1, 3), t, True)
            rows = {"sigma_4B": (dens["sigma"].reshape(N, T, 1).contiguous(), fine["sigma"].reshape(N, U, 1).contiguous()),
                    "geo_feat_60B": (dens["geo_feat"].reshape(N, T, -1).float().contiguous(), fine["geo_feat"].reshape(N, U, -1).float().contiguous()),
                    "positions_12B": (xyz, xyz_new)}
            legs = {k: (lambda a=a, b=b: ops.MergeRowsFn.apply(a, b, src)) for k, (a, b) in rows.items()}
            legs["all_three"] = lambda: [ops.MergeRowsFn.apply(a, b, src) for a, b in rows.values()]
            res["merge_rows"][f"T{T}_U{U}"] = interleaved(legs, args.reps)
            res["merge_rows"][f"T{T}_U{U}"]["bytes_moved_all_three"] = 2 * N * (T + U) * (4 + 60 + 12) + 3 * N * (T + U) * 4
        # whole renders
        legs = {f"run_hier_T{T}_U{U}": (lambda T=T, U=U: run(num_steps=T, upsample_steps=U, hierarchical=True)) for T, U in SETTINGS}
        legs["run_fused_768"] = lambda: run(num_steps=768)

        def chain_768():
            with _ChainOnly(m):
                return run(num_steps=768)
        legs["run_chain_768"] = chain_768
        res["run"] = interleaved(legs, args.reps)
        # range against a 4096-sample even render
        with _ChainOnly(m):
            truth = run(num_steps=4096)["depth_lidar"].view(-1).double()
        res["range_mae"] = {}
        for name, fn in legs.items():
            mae = float((fn()["depth_lidar"].view(-1).double() - truth).abs().mean())
            res["range_mae"][name] = {"scene_units": mae, "metres": mae / S.SCALE}
        for T in (96 + 32, 192 + 64):
            with _ChainOnly(m):
                mae = float((run(num_steps=T)["depth_lidar"].view(-1).double() - truth).abs().mean())
            res["range_mae"][f"run_chain_{T}_even"] = {"scene_units": mae, "metres": mae / S.SCALE}
    torch.cuda.synchronize()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
