"""Timing of the LiDAR cloud cleaning (nvsf/nerf/pointcloud.py, csrc/pointcloud.hip).

    python tools/bench_pointcloud.py [--reps 20] [--out profiles/pointcloud_bench.json]

The cloud: one 66 x 1030 frame of nvsf.synthetic.street_range_image (seed 0) after the range filter, N ~ 55 k, k = 64.
Legs (milliseconds, median and min .. max over --reps after warm-up, device events on the current stream):
  knn_kernel        nvsf_knn_mean_distance, one call;
  knn_torch         the same statistic from torch.cdist + topk in query chunks on the same device: the yardstick the kernel exists to
                    beat (the two are interleaved rep by rep; their largest difference is reported);
  plane_count       nvsf_plane_inlier_count for K = 64 hypotheses; plane_mask for 6 planes;
  process_frame     process_pointcloud per frame over three frames (host wall clock around a synchronise, setup code included).
Distance evaluations: N^2 per call, 8 fp32 operations each (3 subtractions, 3 multiplications, 2 additions; no contraction); the
fraction of the 157.3 TFLOP/s fp32 vector peak they reach is a kernel figure (kernel time from events, launch included).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nvsf import _hip, synthetic as S  # noqa: E402
from nvsf.nerf import pointcloud as P  # noqa: E402
from nvsf.nerf.dataset import formats as F  # noqa: E402
from nvsf.nerf.evaluate import pano_to_lidar  # noqa: E402

PEAK_FP32 = 157.3e12
FLOP_PER_EVAL = 8


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def knn_torch(points, k=64, chunk=4096):
    out = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
    kk = min(k, points.shape[0])
    for s in range(0, points.shape[0], chunk):
        d = torch.cdist(points[s:s + chunk], points)
        out[s:s + chunk] = torch.topk(d, kk, dim=1, largest=False).values.mean(dim=1)
    return out


def frame_set(dev, root, n_frames=3):
    rng = np.random.default_rng(1)
    _, boxes, _ = S.street_range_image(rng)
    panos, frames = [], []
    for i in range(n_frames):
        moved = boxes.copy()
        moved[0, [0, 3]] += 1.5 * i
        panos.append(S.street_range_image(rng, boxes=moved)[0])
        pose = np.eye(4)
        pose[:3, 3] = [0.02 * i, 0, 0]
        frames.append({"frame_id": i, "file_path": f"train/0/img_{i:04d}.npy", "transform_matrix": pose,
                       "lidar_file_path": f"train/0/pano_{i:04d}.npy", "lidar2world": pose})
    os.makedirs(os.path.join(root, "train", "0"), exist_ok=True)
    F.write_transforms(F.transforms_path(root, "0", "train"), w=6, h=4, w_lidar=S.LIDAR_HW[1], h_lidar=S.LIDAR_HW[0],
                       K=np.array([[5.0, 0, 3], [0, 5.0, 2], [0, 0, 1]]), frame_start=0, frame_end=n_frames - 1, num_frames=n_frames,
                       frames=frames)
    return F.FrameSet(root, "0", "train", S.SCALE, device=dev, training=False, images=[np.zeros((4, 6, 3), np.uint8)] * n_frames,
                      range_images=[np.stack([np.zeros_like(p), np.zeros_like(p), p], -1) for p in panos])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pano, _, _ = S.street_range_image(np.random.default_rng(0))
    pts = pano_to_lidar(torch.from_numpy(pano).to(dev), S.LIDAR_FOV[:2], (180.0, S.LIDAR_FOV[2]))
    pts = pts[P.range_filter(pts, 1, 60)].contiguous()
    n = pts.shape[0]
    res = {"unit": "ms (device events; process_frame: host wall clock)", "points": n, "k": 64, "reps": args.reps}
    kernel = lambda: P.knn_mean_distance(pts, 64)
    yard = lambda: knn_torch(pts, 64)
    for _ in range(3):
        a, b = kernel(), yard()
    torch.cuda.synchronize()
    res["knn_kernel_vs_torch_max_abs_diff_m"] = float((a - b).abs().max())
    tk, ty = [], []
    for _ in range(args.reps):  # alternating, so that a busy neighbour hits both
        tk.append(event_ms(kernel))
        ty.append(event_ms(yard))
    res["knn_kernel_ms"], res["knn_torch_ms"] = stats(tk), stats(ty)
    res["knn_torch_over_kernel"] = res["knn_torch_ms"]["median"] / res["knn_kernel_ms"]["median"]
    evals = float(n) * n
    res["distance_evals_per_s"] = evals / (res["knn_kernel_ms"]["median"] * 1e-3)
    res["fraction_of_fp32_vector_peak"] = res["distance_evals_per_s"] * FLOP_PER_EVAL / PEAK_FP32
    triples = torch.randint(0, n, (64, 3), generator=torch.Generator().manual_seed(0)).to(dev)
    planes, _ = P.plane_from_triples(pts, triples)
    counts = torch.zeros(64, dtype=torch.int32, device=dev)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    count = lambda: _hip.call("nvsf_plane_inlier_count", _hip.ptr(pts), n, _hip.ptr(planes), 64, 0.15, _hip.ptr(counts))
    six = planes[:6].contiguous()
    mask_fn = lambda: _hip.call("nvsf_plane_inlier_mask", _hip.ptr(pts), n, _hip.ptr(six), 6, 0.15, -1.0, _hip.ptr(mask))
    for fn in (count, mask_fn, lambda: P.fit_ground(pts)):
        for _ in range(3):
            fn()
    res["plane_count_k64_ms"] = stats([event_ms(count) for _ in range(args.reps)])
    res["plane_mask_r6_ms"] = stats([event_ms(mask_fn) for _ in range(args.reps)])
    res["fit_ground_ms"] = stats([event_ms(lambda: P.fit_ground(pts)) for _ in range(args.reps)])
    with tempfile.TemporaryDirectory() as root:
        fs = frame_set(dev, root)
        P.process_pointcloud(fs, S.LIDAR_MAX_DEPTH)  # warm-up
        torch.cuda.synchronize()
        wall = []
        for _ in range(max(3, args.reps // 4)):
            t0 = time.perf_counter()
            pcs, grounds = P.process_pointcloud(fs, S.LIDAR_MAX_DEPTH)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3 / len(fs))
        res["process_frame_ms"] = stats(wall)
        res["process_frame_points"] = [int(p.shape[0]) for p in pcs.values()]
        res["process_frame_ground"] = [int(g.shape[0]) for g in grounds.values()]
    res["device"] = torch.cuda.get_device_name(0)
    res["build_digest"] = _hip.build_digest()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
