"""Timing of the hash grid's coordinate gradient and of the four-launch density gradient, and -- with --dynamic --
of the space-time model's (section 9m).

    python tools/bench_normals.py [--reps 20] [--label NAME] [--out profiles/normals_bench.json]
    python tools/bench_normals.py --dynamic [--reps 20] [--label NAME] [--out profiles/normals_dynamic_bench.json]

Legs, in milliseconds between device events on the current stream, median and min .. max of the repeats after warm-up, at 4096 x 768
ray-ordered samples (LiDAR rays of the synthetic scene, the config-2 batch), interleaved rep by rep so that a busy neighbour hits all:
  fwd / grad_x          `hashgrid_forward` next to `hashgrid_grad_x` (fp32 gradient rows) on the config-2 grid (L16 F2, T = 2^19, 16 ->
                        2048) and on the L8 F4 grid (T = 2^19, 512 -> 32768; its forward is the one-level-per-XCD kernel): the two do
                        the same gathers;
  grad_x_level_major    the same gradient read level by level ([L, M, F], what the density MLP's backward writes);
  density / density_gradient   NeRFNetworkStatic.density under no_grad (three launches) next to density_gradient (four launches plus
                        the one-hot fill and the normalisation in torch).
Per leg `bytes_per_sample` is what the launch must move if every table read hits a cache (positions, gradient or feature rows, result)
and `fraction_of_hbm_peak` that figure over the median at 8 TB/s: the gathers themselves are cache traffic, so the share says how far
from a streaming kernel the leg is, not how well it uses HBM.  `--label` names the tree; with --out the result is merged into that file.
--dynamic: the config-5 space-time model (bench.py's dynamic leg: time_resolution 8, 93.6 M parameters; random hash tables, the flow field
as initialised) at the same samples, frame time 0.5, the flow MLP in the fp16 regime:
  hash4d_fwd / hash4d_grad_x    nvsf_hashgrid4d_dynamic_fwd (mode 0) next to nvsf_hashgrid4d_dynamic_grad_x on the same inputs, the gradient
                        read in place as columns 96..119 of a 120-column matrix (what density_gradient passes): the two make
                        the same gathers;
  density / density_gradient / density_gradient_no_flow_jacobian    NeRFNetwork.density under no_grad next to density_gradient with and
                        without the J_f^T term;
  lagrange_expansion / flow_grid_jtp    the [M, 2 L] -> [M, 8 L] expansion of the flow grid's gradient alone and the whole product
                        (expansion + hashgrid_grad_x at D = 3, F = 8); `expansion_share_of_density_gradient` is the first over
                        density_gradient's median.
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
from nvsf.nerf import normals  # noqa: E402
from nvsf.nerf.models.network_static import NeRFNetworkStatic  # noqa: E402

HBM_PEAK = 8e12
N, T = 4096, 768


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


def with_bytes(res, per_sample, M):
    for k, b in per_sample.items():
        sec = res[k]["median"] * 1e-3
        res[k].update(bytes_per_sample=b, bandwidth_gb_s=b * M / sec / 1e9, fraction_of_hbm_peak=b * M / sec / HBM_PEAK)
    return res


def sample_positions(model, dev):
    """x01 [N T, 3] of 4096 LiDAR rays x 768 uniform samples, ray by ray, and the world-space points."""
    o, d = S.lidar_rays(N, np.random.default_rng(0))
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    nears, fars = model._near_far(o, d, True, model.aabb_infer)
    _, xyzs = ops.uniform_samples(o, d, nears, fars, T, model.aabb_infer, None)
    xyz = xyzs.view(-1, 3)
    return ((xyz + model.bound) / (2 * model.bound)).contiguous(), xyz


def grid_legs(spec, x01, dev, reps):
    g = torch.Generator().manual_seed(0)
    M = x01.shape[0]
    table = (torch.randn(spec.n_params, generator=g) * 0.1).half().to(dev)
    rows = torch.randn(M, spec.n_output_dims, device=dev)
    level_major = rows.view(M, spec.L, spec.F).permute(1, 0, 2).contiguous()
    feat = torch.empty(M, spec.n_output_dims, dtype=torch.float16, device=dev)
    gx = torch.empty(M, 3, device=dev)
    cols = (0, 1, 2)
    legs = {"fwd": lambda: ops.hashgrid_forward(x01, cols, table, spec, out=feat),
            "grad_x": lambda: ops.hashgrid_grad_x(x01, cols, table, spec, rows, out=gx),
            "grad_x_level_major": lambda: ops.hashgrid_grad_x(x01, cols, table, spec, level_major, out=gx)}
    res = interleaved(legs, reps)
    lf = spec.n_output_dims
    res = with_bytes(res, {"fwd": 12 + 2 * lf, "grad_x": 12 + 4 * lf + 12, "grad_x_level_major": 12 + 4 * lf + 12}, M)
    res["gather_bytes_per_sample"] = 8 * spec.L * spec.F * 2  # eight corners per level, F halves each: through the caches
    res["grad_x_over_fwd"] = res["grad_x"]["median"] / res["fwd"]["median"]
    res["levels"], res["features"], res["table_bytes"] = spec.L, spec.F, 2 * spec.n_params
    return res


def density_legs(model, xyz, reps):
    legs = {"density": lambda: model.density(xyz, cal_lidar_color=True), "density_gradient": lambda: normals.density_gradient(model, xyz, True)}
    with torch.no_grad():
        res = interleaved(legs, reps)
    res["gradient_over_density"] = res["density_gradient"]["median"] / res["density"]["median"]
    return res


def dynamic_result(dev, reps):
    from nvsf.nerf.models.hash_field import lagrange_weights_host, time_slot
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    model = NeRFNetwork(time_resolution=8, num_frames=S.NUM_FRAMES, bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR,
                        lidar_max_depth=S.LIDAR_MAX_DEPTH)
    with torch.no_grad():
        for p in model.hash_encoder_lidar.parameters():
            p.normal_(0.0, 0.1)
    model = model.to(dev).eval()
    x01, xyz = sample_positions(model, dev)
    M = x01.shape[0]
    t_host = 0.5
    t = torch.tensor([[t_host]], dtype=torch.float32, device=dev)
    enc = model.hash_encoder_lidar
    slot = time_slot(t, t_host, enc.hash_dynamic[0].time_resolution)
    g24 = torch.randn(M, 120, device=dev)[:, 96:120]  # as the chain hands it over: columns of the density MLP's input gradient, rows 480 B apart
    gx = torch.empty(M, 3, device=dev)
    flow_net = model.flow_net
    L = flow_net.grid_enc.spec.L
    g_red = torch.randn(M, 2 * L, device=dev)
    w4 = lagrange_weights_host(t_host, 4, True)
    xt = torch.cat([x01, t.expand(M, 1)], -1).contiguous()
    with torch.no_grad():
        kernel = interleaved({"hash4d_fwd": lambda: enc._forward_dynamic_fused(x01, t, slot, None, 0),
                              "hash4d_grad_x": lambda: enc.dynamic_grad_x(x01, t, t_host, g24, out=gx)}, reps)
        # forward: 12 position + 96 features; grad_x: 12 + 96 gradient (of rows of 480: every line of them is touched) + 12; the gathers (2 slices x 4 corners x 8 bytes per item) are cache traffic
        kernel = with_bytes(kernel, {"hash4d_fwd": 12 + 96, "hash4d_grad_x": 12 + 96 + 12}, M)
        kernel["gather_bytes_per_sample"] = 24 * (1 if slot.same else 2) * 4 * 8
        kernel["same_slice"] = bool(slot.same)
        kernel["grad_x_over_fwd"] = kernel["hash4d_grad_x"]["median"] / kernel["hash4d_fwd"]["median"]
        chain = interleaved({"density": lambda: model.density(xyz, t, True, fp16=True),
                             "density_gradient": lambda: normals.density_gradient(model, xyz, True, time=t, fp16=True),
                             "density_gradient_no_flow_jacobian": lambda: normals.density_gradient(model, xyz, True, time=t, fp16=True, flow_jacobian=False),
                             "lagrange_expansion": lambda: normals.expand_lagrange_gradient(g_red, w4),
                             "flow_grid_jtp": lambda: normals.flow_grid_jtp(flow_net, xt, t_host, g_red)}, reps)
    chain["gradient_over_density"] = chain["density_gradient"]["median"] / chain["density"]["median"]
    chain["expansion_share_of_density_gradient"] = chain["lagrange_expansion"]["median"] / chain["density_gradient"]["median"]
    return {"unit": "ms (device events)", "shape": [N, T], "reps": reps, "device": torch.cuda.get_device_name(0), "build_digest": _hip.build_digest(),
            "frame_time": t_host, "parameters_M": sum(p.numel() for p in model.parameters()) / 1e6, "hash4d": kernel, "chain": chain}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dynamic", action="store_true", help="the space-time model's legs (DESIGN.md 9m) instead of the static field's")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.dynamic:
        return emit(args, dynamic_result(dev, args.reps))
    model = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH)
    with torch.no_grad():
        model.hash_encoder_lidar.params.normal_(0.0, 0.1)
    model = model.to(dev).eval()
    x01, xyz = sample_positions(model, dev)
    l8f4 = ops.GridSpec(3, 8, 4, 19, 512, float(np.exp2(np.log2(32768 / 512) / 7)))
    res = {"unit": "ms (device events)", "shape": [N, T], "reps": args.reps, "device": torch.cuda.get_device_name(0), "build_digest": _hip.build_digest(),
           "config2_L16_F2": grid_legs(model.hash_encoder_lidar.spec, x01, dev, args.reps), "L8_F4": grid_legs(l8f4, x01, dev, args.reps),
           "density": density_legs(model, xyz, args.reps)}
    emit(args, res)


def emit(args, res):
    print(json.dumps({args.label: res}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
        merged[args.label] = res
        with open(args.out, "w") as f:
            f.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()
