"""Timing of the object masks and of the range-image z-buffer (csrc/object_masks.hip).

    python tools/bench_object_masks.py [--reps 20] [--out profiles/object_masks_bench.json]

Method as tools/bench_depth_image.py (whose helpers are used): every leg is the median and min .. max of --reps runs after warm-up, in
milliseconds between device events on the current stream; an entry and its yardsticks are interleaved rep by rep; `decided`: whether the
medians differ by more than the two spreads combined.  A frame is 0.27 MB: the kernels are expected to be launch-bound, and no bandwidth
figure is derived.
Legs:
  fused_mask_10 / _64   nvsf_range_image_object_mask on one 66 x 1030 street range image with 10 and with 64 yawed boxes (planes already on
                        the device), against
                          torch   a torch-on-device restatement: cloud, half-space tests as one [P, B K] product in fp64, projection,
                                  scatter_reduce(amin) over 64-bit keys, a gather of the membership;
                          numpy   the host path restated: vectorised cloud and membership, then the reference's per-point Python loop
                                  (lib/convert.py:143-176) -- it takes about a second, so it joins the first 3 reps only;
  zbuffer_47k / _120k   nvsf_lidar_to_pano on random clouds with payloads into 66 x 1030, against the same two yardsticks without the
                        membership;
  image_mask            nvsf_box_mask_image, 10 boxes into 376 x 1408, against a torch broadcast compare and the reference's double
                        Python loop over the boxes' pixels (utils.py:857-868).
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
from nvsf.nerf import object_masks as OM  # noqa: E402

HL, WL = 66, 1030
FOV, FOV_HOZ, MAX_DEPTH = (2.0, 26.9), (180.0, 360.0), 80.0


def constants(H, W):
    return (np.float32(FOV_HOZ[0] * np.pi / 180), np.float32((FOV_HOZ[1] * np.pi / 180) / W), np.float32((FOV[1] - FOV[0]) / 180 * np.pi),
            np.float32(FOV[1] / 180 * np.pi / H))


def boxes_lidar(n, rng):
    """n yawed car-sized boxes standing on the street around the sensor -> list of [6, 4] half-spaces in the LiDAR frame."""
    hulls = []
    for _ in range(n):
        yaw, r, az = rng.uniform(-3, 3), rng.uniform(4, 40), rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * [2.2, 0.9, 0.8]
        hulls.append(OM.hull_planes(corners @ R.T + [r * np.cos(az), r * np.sin(az), -0.95]))
    return hulls


def torch_cloud(r):
    H, W = r.shape
    i = torch.arange(W, dtype=torch.float32, device=r.device)[None, :]
    j = torch.arange(H, dtype=torch.float32, device=r.device)[:, None]
    beta = -(i - W / 2) / W * FOV_HOZ[1] / 180 * np.pi
    alpha = (FOV[0] - j / H * FOV[1]) / 180 * np.pi
    dirs = torch.stack([torch.cos(alpha) * torch.cos(beta), torch.cos(alpha) * torch.sin(beta), torch.sin(alpha).expand(H, W)], -1)
    return (dirs * r[..., None])[r != 0.0]


def torch_member(pc, planes, counts):
    B, K, _ = planes.shape
    s = pc.double() @ planes[..., :3].reshape(B * K, 3).T + planes[..., 3].reshape(B * K)
    live = (torch.arange(K, device=pc.device)[None, :] < counts[:, None]).reshape(B * K)
    return ((s <= 0) | ~live).view(-1, B, K).all(-1).any(-1)


def torch_zbuffer(pc, payload, H, W):
    az0, step_h, el0, step_v = (float(v) for v in constants(H, W))
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    dist = torch.sqrt(x * x + y * y + z * z)
    c = torch.round((az0 - torch.atan2(y, x)) / step_h)
    r = torch.round(H - (torch.atan2(z, torch.sqrt(x * x + y * y)) + el0) / step_v)
    ok = (dist < MAX_DEPTH) & (dist != 0) & (r >= 0) & (r < H) & (c >= 0) & (c < W)
    idx = torch.nonzero(ok)[:, 0]
    key = (dist[idx].view(torch.int32).long() << 32) | idx
    ws = torch.full((H * W,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=pc.device)
    ws.scatter_reduce_(0, r[idx].long() * W + c[idx].long(), key, "amin")
    hit = ws != torch.iinfo(torch.int64).max
    win = (ws & 0xFFFFFFFF).clamp(max=pc.shape[0] - 1)
    pano = torch.where(hit, (ws >> 32).int().view(torch.float32), torch.zeros((), device=pc.device))
    return pano.view(H, W), torch.where(hit, payload[win], torch.zeros((), device=pc.device)).view(H, W)


def numpy_cloud(r):
    H, W = r.shape
    az = -(np.arange(W, dtype=np.float32) - W / 2) / W * FOV_HOZ[1] / 180 * np.pi
    el = (FOV[0] - np.arange(H, dtype=np.float32) / H * FOV[1]) / 180 * np.pi
    dirs = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (H, W))], -1)
    return (dirs * r[..., None])[r != 0.0]


def numpy_member(pc, hulls):
    p = pc.astype(np.float64)
    out = np.zeros(p.shape[0], bool)
    for h in hulls:
        out |= (p @ h[:, :3].T + h[:, 3] <= 0).all(1)
    return out


def numpy_zbuffer(pc, payload, H, W):
    """The per-point loop of lib/convert.py:143-176 on numpy scalars, as the reference runs it."""
    az0, step_h, el0, step_v = constants(H, W)
    pano, img = np.zeros((H, W)), np.zeros((H, W))
    for (x, y, z), dist, v in zip(pc, np.linalg.norm(pc, axis=1), payload):
        if dist >= MAX_DEPTH:
            continue
        c = int(round((az0 - np.arctan2(y, x)) / step_h))
        r = int(round(H - (np.arctan2(z, np.sqrt(x ** 2 + y ** 2)) + el0) / step_v))
        if r >= H or r < 0 or c >= W or c < 0:
            continue
        if pano[r, c] == 0.0 or pano[r, c] > dist:
            pano[r, c], img[r, c] = dist, v
    return pano, img


def fused_legs(dev, reps):
    res = {}
    r_host = S.street_range_image(np.random.default_rng(0))[0].astype(np.float32)
    r = torch.from_numpy(r_host).to(dev)
    geom = _hip.host_f64([FOV[0], FOV[1], FOV_HOZ[0], FOV_HOZ[1], MAX_DEPTH])
    ws, dyn = torch.empty(HL * WL, dtype=torch.int64, device=dev), torch.empty(HL, WL, device=dev)
    for n in (10, 64):
        hulls = boxes_lidar(n, np.random.default_rng(n))
        planes, counts = OM.pack_planes(hulls)
        dp, dc = torch.from_numpy(planes).to(dev), torch.from_numpy(counts.view(np.int32)).to(dev)
        entry = lambda: _hip.call("nvsf_range_image_object_mask", _hip.ptr(r), HL, WL, geom, _hip.ptr(dp), _hip.ptr(dc), n, planes.shape[1],
                                  _hip.ptr(ws), ws.numel() * 8, _hip.ptr(dyn))

        def by_torch():
            pc = torch_cloud(r)
            return torch_zbuffer(pc, torch_member(pc, dp, dc.long()).float(), HL, WL)[1]

        def by_numpy():
            pc = numpy_cloud(r_host)
            return numpy_zbuffer(pc, numpy_member(pc, hulls).astype(np.float32), HL, WL)[1]
        leg = versus(entry, {"torch": by_torch, "numpy": by_numpy}, reps, fewer={"numpy": 3})
        entry()
        got = dyn.clone()
        leg.update(boxes=n, points=int((r != 0).sum()), dynamic_pixels=int(got.sum()),
                   pixels_not_equal_to_torch=int((got != by_torch()).sum()), pixels_not_equal_to_numpy=int((got.cpu().numpy() != by_numpy()).sum()))
        res[f"fused_mask_{n}"] = leg
    return res


def zbuffer_legs(dev, reps):
    res = {}
    geom = _hip.host_f64([FOV[0], FOV[1], FOV_HOZ[0], FOV_HOZ[1], MAX_DEPTH])
    ws, pano, img = torch.empty(HL * WL, dtype=torch.int64, device=dev), torch.empty(HL, WL, device=dev), torch.empty(HL, WL, device=dev)
    for name, P in (("zbuffer_47k", 47000), ("zbuffer_120k", 120000)):
        rng = np.random.default_rng(P)
        az, el, rad = rng.uniform(-np.pi, np.pi, P), np.deg2rad(rng.uniform(-26.0, 3.0, P)), rng.uniform(1.0, 90.0, P)
        host = np.stack([rad * np.cos(el) * np.cos(az), rad * np.cos(el) * np.sin(az), rad * np.sin(el)], -1).astype(np.float32)
        pay_host = rng.random(P).astype(np.float32)
        pts, pay = torch.from_numpy(host).to(dev), torch.from_numpy(pay_host).to(dev)
        entry = lambda: _hip.call("nvsf_lidar_to_pano", _hip.ptr(pts), _hip.ptr(pay), P, HL, WL, geom, _hip.ptr(ws), ws.numel() * 8, _hip.ptr(pano),
                                  _hip.ptr(img))
        leg = versus(entry, {"torch": lambda: torch_zbuffer(pts, pay, HL, WL), "numpy": lambda: numpy_zbuffer(host, pay_host, HL, WL)}, reps,
                     fewer={"numpy": 3})
        entry()
        leg.update(points=P, non_empty_pixels=int((pano != 0).sum()),
                   pixels_not_bit_equal_to_torch=int((pano.view(torch.int32) != torch_zbuffer(pts, pay, HL, WL)[0].view(torch.int32)).sum()))
        res[name] = leg
    return res


def image_mask_leg(dev, reps, H=376, W=1408, n=10):
    rng = np.random.default_rng(1)
    x0, y0 = rng.integers(0, W - 200, n), rng.integers(0, H - 120, n)
    boxes = np.stack([x0, y0, x0 + rng.integers(40, 200, n), y0 + rng.integers(30, 120, n)], 1).astype(np.int32)
    db, out = torch.from_numpy(boxes).to(dev), torch.empty(H, W, dtype=torch.uint8, device=dev)
    xs, ys = torch.arange(W, device=dev)[None, None, :], torch.arange(H, device=dev)[None, :, None]
    entry = lambda: _hip.call("nvsf_box_mask_image", _hip.ptr(db), n, H, W, _hip.ptr(out))

    def by_torch():
        b = db[:, :, None, None]
        return ((xs >= b[:, 0]) & (xs <= b[:, 2]) & (ys >= b[:, 1]) & (ys <= b[:, 3])).any(0)

    def by_numpy():
        pixels = []
        for bx0, by0, bx1, by1 in boxes.tolist():
            for y in range(by0, by1 + 1):
                for x in range(bx0, bx1 + 1):
                    pixels.append((y, x))
        pixels = np.vstack(pixels)
        static = np.ones([H, W], dtype=bool)
        static[pixels[:, 0], pixels[:, 1]] = False
        return ~static
    leg = versus(entry, {"torch": by_torch, "numpy": by_numpy}, reps, fewer={"numpy": 5})
    entry()
    leg.update(boxes=n, dynamic_pixels=int(out.sum()), pixels_not_equal_to_torch=int((out.bool() != by_torch()).sum()),
               pixels_not_equal_to_numpy=int((out.bool().cpu().numpy() != by_numpy()).sum()))
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"unit": "ms (device events)", "reps": args.reps}
    res.update(fused_legs(dev, args.reps))
    res.update(zbuffer_legs(dev, args.reps))
    res["image_mask"] = image_mask_leg(dev, args.reps)
    res["device"] = torch.cuda.get_device_name(0)
    res["build_digest"] = _hip.build_digest()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
