"""CPU side of the depth-map tests: the fixture of tests/golden/golden_depth_image.py, a vectorised numpy restatement of the
reference's projection and z-buffer (dataset_utils.py:17-32, 69-96), the bookkeeping of points that sit on a pixel boundary, and
restatements of the camera depth term (trainer.py:506-518, criteria of main_nvsf.py:205-212) and of the camera depth RMSE
(error_matrices.py:90-100)."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CRITERIA = ("l1", "mse", "smoothl1", "huber", "bce")


def fixture():
    return dict(np.load(os.path.join(HERE, "golden", "depth_image.npz")))


def fixture_cloud(fx, f):
    """The reference's cloud of frame f, rebuilt from the stored factors (the generator asserted that this is bit-equal)."""
    r = fx["range_m"][f]
    dirs = np.stack([fx["ca"][:, None] * fx["cb"][None, :], fx["ca"][:, None] * fx["sb"][None, :], np.broadcast_to(fx["sa"][:, None], r.shape)], -1)
    pc = (dirs * r[..., None])[r != 0.0]
    assert pc.dtype == np.float32 and pc.shape[0] == int(fx[f"f{f}_n_points"])
    return pc


def range_cloud(range_m, fov, fov_hoz):
    """Step 1 in numpy (convert.py:241-266), factored: fp32 cos / sin of the H elevations and the W azimuths, their products times the
    range, zero-range pixels left out, row-major.  fov = (fov_up, fov), fov_hoz = (fov_hoz_up, fov_hoz), degrees."""
    r = np.asarray(range_m, np.float32)
    Hl, Wl = r.shape
    col, row = np.arange(Wl, dtype=np.float32), np.arange(Hl, dtype=np.float32)
    (fov_up, fov_v), fov_h = (float(v) for v in fov), float(fov_hoz[1])  # Python floats: the arrays stay fp32
    az = -(col - Wl / 2) / Wl * fov_h / 180 * np.pi
    el = (fov_up - row / Hl * fov_v) / 180 * np.pi
    assert az.dtype == np.float32 and el.dtype == np.float32
    dirs = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], r.shape)], -1)
    return (dirs * r[..., None])[r != 0.0]


def fixture_image(fx, key):
    img = np.zeros(int(fx["H"]) * int(fx["W"]), np.float32)
    img[fx[f"{key}_img_idx"]] = fx[f"{key}_img_val"]
    return img.reshape(int(fx["H"]), int(fx["W"]))


def project(points, lidar2cam, K):
    """Step 2: fp32 points, fp32 lidar2cam, fp64 K -> fp64 [P, 3] = (u, v, z), z clipped, (u, v) divided.  Sums written out left to
    right (what the kernel does) instead of a BLAS call, so that every machine rounds alike."""
    p = np.asarray(points, np.float32).astype(np.float64)
    m = np.asarray(lidar2cam, np.float32).astype(np.float64)
    k = np.asarray(K, np.float64)[:3, :3]
    c = [((p[:, 0] * m[r, 0] + p[:, 1] * m[r, 1]) + p[:, 2] * m[r, 2]) + m[r, 3] for r in range(3)]
    q = [(c[0] * k[r, 0] + c[1] * k[r, 1]) + c[2] * k[r, 2] for r in range(3)]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z = np.clip(q[2], 1e-5, 99999)
        return np.stack([q[0] / z, q[1] / z, z], -1)


def zbuffer(uvz, H, W):
    """Step 3: the smallest z per pixel, rounded to fp32, 0 where empty.  (Rounding is monotonic: min then round = round then min.)"""
    u, v, z = uvz[:, 0], uvz[:, 1], uvz[:, 2]
    with np.errstate(invalid="ignore"):
        inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    pix = v[inside].astype(np.int64) * W + u[inside].astype(np.int64)
    img = np.full(H * W, np.inf, np.float32)
    np.minimum.at(img, pix, z[inside].astype(np.float32))
    img[np.isinf(img)] = 0.0
    return img.reshape(H, W)


def borderline_pixels(uvz, eps, H, W):
    """bool [H, W]: the pixels that hold, or could receive, a point whose u or v lies within eps of a pixel boundary -- every pixel such a
    point reaches when it moves by up to eps in u and in v.  -> (mask, number of such points)."""
    u, v = uvz[:, 0], uvz[:, 1]
    with np.errstate(invalid="ignore"):
        close = (np.abs(u - np.round(u)) < eps) | (np.abs(v - np.round(v)) < eps)
        close &= (u > -eps) & (u < W + eps) & (v > -eps) & (v < H + eps)
    mask = np.zeros((H, W), bool)
    for du in (-eps, 0.0, eps):
        for dv in (-eps, 0.0, eps):
            x, y = np.floor(u[close] + du).astype(np.int64), np.floor(v[close] + dv).astype(np.int64)
            ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            mask[y[ok], x[ok]] = True
    return mask, int(close.sum())


def _criterion(x, y, criterion, scale):
    """The per-element criteria of main_nvsf.py:205-212 written out: x prediction (logit under bce), y target."""
    e = x - y
    a = e.abs()
    if criterion == "l1":
        return a
    if criterion == "mse":
        return e * e
    if criterion == "smoothl1":  # beta 0.1
        return torch.where(a < 0.1, 0.5 * e * e / 0.1, a - 0.05)
    if criterion == "huber":     # delta 0.2 scale
        delta = 0.2 * scale
        return torch.where(a <= delta, 0.5 * e * e, delta * (a - 0.5 * delta))
    if criterion == "bce":       # BCE-with-logits: -y log s(x) - (1 - y) log(1 - s(x)) in its overflow-free form
        return x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    raise ValueError(criterion)


def reference_depth_terms(pred_depth, image_depths, scale, criterion, alpha_rd):
    """The camera depth term as trainer.py:506-518 defines it, restated: pred_depth [B, N] in scene units (may require grad),
    image_depths [B, N, 1] in metres.  Target = map times scale, target and prediction both capped at 80 scale -- the cap REPLACES the
    prediction, so a capped ray has no gradient --, rays whose target is 0 are masked on both sides, and every ray, masked or not,
    contributes criterion(masked prediction, masked target) times alpha_rd.  Returns the [B, N] terms; the trainer sums them
    (trainer.py:545-547)."""
    cap = 80 * scale
    target = (image_depths[..., 0] * scale).clamp(max=cap)
    over = pred_depth > cap
    pred = pred_depth.masked_fill(over, cap)
    seen = (target > 0).to(pred.dtype)
    return alpha_rd * _criterion(pred * seen, target * seen, criterion, scale)


def camera_depth_rmse(pred_m, truth_m):
    """RMSEMeter(rgb_metric=True) of one frame as error_matrices.py:90-100 defines it, restated in float64: the prediction counts only
    where the map holds a depth, both are capped at 80 m, root of the mean squared difference over ALL pixels."""
    p, t = np.asarray(pred_m, np.float32).astype(np.float64), np.asarray(truth_m, np.float32).astype(np.float64)
    p = np.minimum(np.where(t == 0, 0.0, p), 80.0)
    t = np.minimum(t, 80.0)
    return float(np.sqrt(np.mean((t - p) ** 2)))


def loss_rays(n, scale, seed, dtype=torch.float32):
    """A ray batch for the camera terms: ~85 % empty map pixels, some map depths and some rendered depths over the 80 m cap.
    -> image [1, n, 3], gt_rgb [1, n, 3], depth [1, n] (scene units), gt_m [1, n] (metres)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    gt_m = rnd(1, n) * 95.0 + 0.5                       # up to 95.5 m: ~16 % of the hits beyond the cap
    gt_m[rnd(1, n) < 0.85] = 0.0
    depth = (gt_m + (rnd(1, n) - 0.5) * 4.0).clamp(min=0.05) * scale
    empty = gt_m == 0
    depth[empty] = (rnd(1, n)[empty] * 100.0 + 0.05) * scale   # rendered depth where the map is empty, some over the cap too
    return rnd(1, n, 3).to(dtype), rnd(1, n, 3).to(dtype), depth.to(dtype), gt_m.to(dtype)
