"""Timing of the per-frame prediction export (csrc/export.hip, nvsf/nerf/export.py) at the range-image size of the recording.

    python tools/bench_export.py [--reps 20] [--out profiles/export_bench.json]

Method as tools/bench_depth_image.py (whose helpers are used): every leg is the median and min .. max of --reps runs after warm-up, in
milliseconds between device events on the current stream; the entry and its yardstick are interleaved rep by rep; `decided`: whether
the medians differ by more than the two spreads combined.  A frame is 68 k pixels (0.27 MB): every form is launch-bound and no bandwidth
figure is derived.  Both sides include their one device -> host read of the point count.
Legs, on one 66 x 1030 street range image with rendered-looking ray-drop and intensity planes:
  frame_export   what export_frames does per frame after test_step: the ray-drop gate on intensity and range (torch), the three uint8
                 planes (nvsf_quantize_u8) and the two clouds with the quantised intensity as payload (nvsf_pano_to_cloud), against
                   torch   today's torch form: the same gate, `(x * 255).to(uint8)` for the planes (inputs inside [0, 1]),
                           evaluate.pano_to_lidar's boolean-mask compaction with the payload gathered by the same mask, a true
                           division by the scale and a float64 matmul for the world frame;
  clouds_only    nvsf_pano_to_cloud alone against the torch cloud alone.
The torch form and the entry are compared on the way: counts, payload column and the largest coordinate difference are in the result.
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

from bench_depth_image import versus  # noqa: E402
from nvsf import _hip, synthetic as S  # noqa: E402
from nvsf.nerf import export as X  # noqa: E402
from nvsf.nerf.evaluate import pano_to_lidar  # noqa: E402

FOV, FOV_HOZ, SCALE, OFFSET, THRES = (2.0, 26.9), (180.0, 360.0), 0.01, (1.5, -2.0, 0.25), 0.5


def torch_clouds(depth, payload, T64, scale32):
    """pano_to_lidar with a payload column, the rescale and the world frame as utils.get_pcd_bound_to_world orders them."""
    pts = pano_to_lidar(depth, FOV, FOV_HOZ) / scale32
    lidar = torch.cat([pts, payload[depth != 0.0][:, None]], 1)
    world = torch.cat([pts.double() @ T64[:3, :3].T + T64[:3, 3], lidar[:, 3:].double()], 1)
    return lidar, world


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    depth = torch.from_numpy((S.street_range_image(rng)[0] * SCALE).astype(np.float32)).to(dev)
    depth[depth == 0] = 0.3  # the render has a range everywhere; the gate below drops about a third
    raydrop = torch.from_numpy(rng.random(tuple(depth.shape)).astype(np.float32)).to(dev) * 0.75 + 0.2
    intensity = torch.from_numpy(rng.random(tuple(depth.shape)).astype(np.float32)).to(dev)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = [[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]
    pose[:3, 3] = [0.4, -0.2, 0.01]
    pose_t = torch.from_numpy(pose)
    T64 = torch.from_numpy(X.world_matrix(pose, SCALE, OFFSET).astype(np.float64)).to(dev)
    scale32 = torch.full((), SCALE, dtype=torch.float32, device=dev)

    def gate():
        m = (raydrop > THRES).to(torch.float32)
        return m, intensity * m, depth * m

    def entry():
        m, i, d = gate()
        planes = (X.quantize_u8(m), X.quantize_u8(i), X.quantize_u8(d))
        return planes, X.pano_to_cloud(d, planes[1].to(torch.float32), pose_t, SCALE, OFFSET, FOV, FOV_HOZ)

    def by_torch():
        m, i, d = gate()
        planes = tuple((p * 255.0).to(torch.uint8) for p in (m, i, d))
        return planes, torch_clouds(d, planes[1].to(torch.float32), T64, scale32)
    res = {"unit": "ms (device events)", "reps": args.reps, "range_image": list(depth.shape)}
    leg = versus(entry, {"torch": by_torch}, args.reps)
    (pk, (lk, wk)), (pt, (lt, wt)) = entry(), by_torch()
    leg.update(points=int(lk.shape[0]), points_torch=int(lt.shape[0]), planes_equal=bool(all(torch.equal(a, b) for a, b in zip(pk, pt))),
               payload_equal=bool(torch.equal(lk[:, 3], lt[:, 3])), lidar_max_abs_diff_m=float((lk[:, :3] - lt[:, :3]).abs().max()),
               world_max_abs_diff_m=float((wk[:, :3] - wt[:, :3]).abs().max()))
    res["frame_export"] = leg
    _, _, d = gate()
    pay = intensity.contiguous()
    res["clouds_only"] = versus(lambda: X.pano_to_cloud(d, pay, pose_t, SCALE, OFFSET, FOV, FOV_HOZ), {"torch": lambda: torch_clouds(d, pay, T64, scale32)},
                                args.reps)
    res["device"] = torch.cuda.get_device_name(0)
    res["build_digest"] = _hip.build_digest()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
