"""Timing of the mesh export (nvsf/nerf/mesh.py, csrc/marching_cubes.hip).

    python tools/bench_mesh.py [--reps 20] [--out profiles/mesh_bench.json]

Legs (milliseconds, median over --reps after warm-up, events on the current stream):
  mc_512        marching cubes alone on a 512^3 analytic grid (a sphere plus ripples, ~1.5 % of the cubes cut):
                count pass (k_mc_count + k_mc_scan), host read of the totals, emit pass (k_mc_emit), and the three together;
  export_c2     export_mesh_density at the reference's main settings (main_nvsf.py:297-300: 500 x 500 x 50 over
                [-0.5, -0.5, 0.06] .. [0.5, 0.5, 0.09]) on the static config-2 network, split into field query and the rest;
  export_c5     the same on the config-5 space-time network (time 0.5).
Bytes per grid point of the two passes (compulsory DRAM traffic, neighbours re-read from cache are not counted): count reads u (4)
and writes the packed point word (4); emit reads u (4) and the point word (4) and writes the vertices (12 per vertex) and triangles (12
per triangle).  The fraction of 8 TB/s those bytes reach is printed beside each pass.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nvsf import _hip, synthetic as S  # noqa: E402
from nvsf.nerf import mesh  # noqa: E402

PEAK = 8.0e12  # bytes / s


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def mc_leg(dev, reps):
    n = 512
    ax = torch.arange(n, device=dev, dtype=torch.float32)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c = (n - 1) / 2 + 0.37
    r = torch.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    u = (0.35 * n - r + 3.0 * torch.sin(x * 0.05) * torch.cos(y * 0.07)).contiguous()
    del x, y, z, r
    tables = mesh._tables_on(dev)
    ws_bytes = mesh.workspace_bytes(u.shape)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    args = [_hip.ptr(u), n, n, n, 0.0, _hip.ptr(tables), _hip.ptr(ws)]
    count = lambda: _hip.call("nvsf_marching_cubes_count", *args, ws_bytes, _hip.ptr(totals))
    count()
    nv, nt = (int(v) for v in totals.cpu())
    V = torch.empty(nv, 3, device=dev)
    T = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    emit = lambda: _hip.call("nvsf_marching_cubes_emit", *args, ws_bytes, nv, nt, _hip.ptr(V), nv, _hip.ptr(T), nt)
    t_count = timed(count, reps)
    t_emit = timed(emit, reps)
    t_all = timed(lambda: mesh.marching_cubes(u, 0.0), reps)
    pts = n ** 3
    b_count = 8 * pts
    b_emit = 8 * pts + 12 * nv + 12 * nt
    return {"grid": [n, n, n], "vertices": nv, "triangles": nt, "count_ms": t_count, "emit_ms": t_emit, "marching_cubes_ms": t_all,
            "count_bytes_per_point": 8, "emit_bytes_per_point": b_emit / pts,
            "count_frac_of_8TBs": b_count / (t_count * 1e-3) / PEAK, "emit_frac_of_8TBs": b_emit / (t_emit * 1e-3) / PEAK,
            "host_read_and_alloc_ms": max(0.0, t_all - t_count - t_emit)}


def export_leg(model, dev, reps, time_value=None):
    b_min, b_max, res = [-0.5, -0.5, 0.06], [0.5, 0.5, 0.09], [500, 500, 50]
    t = None if time_value is None else torch.tensor([[time_value]], dtype=torch.float32, device=dev)
    query = lambda p: model.density(p, t)["sigma"].float()
    with torch.no_grad():
        t_query = timed(lambda: mesh.extract_fields(b_min, b_max, res, query, device=dev), max(3, reps // 4))
        u, _ = mesh.extract_fields(b_min, b_max, res, query, device=dev)
        thr = float(u.median())
        t_mc = timed(lambda: mesh.marching_cubes(u, thr), reps)
        v, tri = mesh.marching_cubes(u, thr)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "bench_mesh.ply")
    t0 = time.perf_counter()
    mesh.export_mesh_density(model, path, b_min, b_max, res, thr, time=time_value)
    torch.cuda.synchronize()
    t_export = (time.perf_counter() - t0) * 1e3
    return {"grid": res, "threshold_median": thr, "vertices": int(v.shape[0]), "triangles": int(tri.shape[0]), "field_query_ms": t_query,
            "marching_cubes_ms": t_mc, "export_total_wall_ms": t_export}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"unit": "ms (median, device events); export_total_wall_ms: host wall clock of one export_mesh_density call incl. PLY write",
           "peak_bytes_per_s": PEAK}
    res["mc_512"] = mc_leg(dev, args.reps)
    torch.cuda.empty_cache()
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    torch.manual_seed(0)
    m = NeRFNetworkStatic(bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR, lidar_max_depth=S.LIDAR_MAX_DEPTH)
    with torch.no_grad():
        for enc in (m.hash_encoder_lidar, m.hash_encoder_camera):
            enc.params.normal_(0.0, 0.5)
    res["export_c2"] = export_leg(m.to(dev).eval(), dev, args.reps)
    del m
    torch.cuda.empty_cache()
    from nvsf.nerf.models.network_dynamic import NeRFNetwork
    torch.manual_seed(0)
    m = NeRFNetwork(time_resolution=8, num_frames=64, bound=S.BOUND, min_near=S.MIN_NEAR, min_near_lidar=S.MIN_NEAR,
                    lidar_max_depth=S.LIDAR_MAX_DEPTH).to(dev).eval()
    res["export_c5"] = export_leg(m, dev, args.reps, time_value=0.5)
    res["device"] = torch.cuda.get_device_name(0)
    res["build_digest"] = _hip.build_digest()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
