"""CPU side of the device meters (nvsf/nerf/meters.py, csrc/metrics.hip): the float64 oracles the GPU tests compare the kernels with,
checked against literal loops; the price of evaluating SSIM and the error sums in fp64 where the libraries the reference calls work
in fp32; report formats; refusal of CPU tensors; the evaluate_frames signature.

The oracles restate the PUBLISHED definitions of skimage.metrics.structural_similarity (uniform 7 x 7 window, sample covariance,
crop by (size - 1) / 2) and of torchmetrics' structural_similarity_index_measure (Gaussian 11 x 11, sigma 1.5, population covariance,
same crop).  Neither library is installed where these tests run, so -- like the Open3D filter of DESIGN.md 9c -- the two forms are
not pinned against the compiled libraries themselves."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))

UNIFORM, GAUSSIAN = 0, 1


# ---- oracles (float64) -----------------------------------------------------------------------------------------------------------
def gaussian_weights(size, sigma):
    d = np.arange(size, dtype=np.float64) - (size - 1) / 2
    w = np.exp(-0.5 * (d / sigma) ** 2)
    return w / w.sum()


def _window_mean(x, window, size, sigma):
    """Windowed mean of a [H, W] float64 image at the positions whose window lies inside it: [H - size + 1, W - size + 1]."""
    from scipy import ndimage
    pad = (size - 1) // 2
    if window == UNIFORM:
        f = ndimage.uniform_filter(x, size=size)
    else:
        w = gaussian_weights(size, sigma)
        f = ndimage.correlate1d(ndimage.correlate1d(x, w, axis=0), w, axis=1)
    return f[pad:x.shape[0] - pad, pad:x.shape[1] - pad]


def ssim_map_oracle(p, t, data_range, window, size, sigma=1.5, sample_cov=False):
    """S per window position and channel, [H - size + 1, W - size + 1, C] float64, from fp32 images [H, W] or [H, W, C]."""
    p, t = (np.asarray(a, dtype=np.float64).reshape(a.shape[0], a.shape[1], -1) for a in (p, t))
    R = np.float64(data_range)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    k = size * size / (size * size - 1.0) if sample_cov else 1.0
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(p.shape[2]):
            a, b = p[..., c], t[..., c]
            ma, mb = (_window_mean(v, window, size, sigma) for v in (a, b))
            maa, mbb, mab = (_window_mean(v, window, size, sigma) for v in (a * a, b * b, a * b))
            va, vb, vab = k * (maa - ma * ma), k * (mbb - mb * mb), k * (mab - ma * mb)
            out.append(((2 * ma * mb + c1) * (2 * vab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2)))
    return np.stack(out, axis=-1)


def ssim_oracle(p, t, data_range, window, size, sigma=1.5, sample_cov=False):
    return float(ssim_map_oracle(p, t, data_range, window, size, sigma, sample_cov).mean())


def ssim_literal(p, t, data_range, window, size, sigma=1.5, sample_cov=False):
    """The definition written out: one double loop over window positions, the 2-D window as an explicit weight matrix."""
    p, t = (np.asarray(a, dtype=np.float64).reshape(a.shape[0], a.shape[1], -1) for a in (p, t))
    w1 = gaussian_weights(size, sigma) if window == GAUSSIAN else np.full(size, 1.0 / size)
    w2 = np.outer(w1, w1)
    R = float(data_range)
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    k = size * size / (size * size - 1.0) if sample_cov else 1.0
    H, W, C = p.shape
    total, count = 0.0, 0
    for c in range(C):
        for y in range(H - size + 1):
            for x in range(W - size + 1):
                a, b = p[y:y + size, x:x + size, c], t[y:y + size, x:x + size, c]
                ma, mb = (w2 * a).sum(), (w2 * b).sum()
                va, vb, vab = k * ((w2 * a * a).sum() - ma * ma), k * ((w2 * b * b).sum() - mb * mb), k * ((w2 * a * b).sum() - ma * mb)
                total += ((2 * ma * mb + c1) * (2 * vab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
                count += 1
    return total / count


def clamp_ref(x, lo, hi):
    """The reference's `x[x < lo] = lo; x[x > hi] = hi` on a float32 copy (NaN passes through)."""
    x = np.array(x, dtype=np.float32)
    x[x < np.float32(lo)] = np.float32(lo)
    x[x > np.float32(hi)] = np.float32(hi)
    return x


def stats_oracle(p, t, lo=-np.inf, hi=np.inf):
    """float64 [6]: sum d^2, sum |d|, min t, max t, min p, max p with d = t - p formed in float32 after the clamp."""
    p, t = clamp_ref(p, lo, hi).reshape(-1), clamp_ref(t, lo, hi).reshape(-1)
    d = (t - p).astype(np.float64)
    return np.array([(d * d).sum(), np.abs(d).sum(), t.min(), t.max(), p.min(), p.max()], dtype=np.float64)


def median_oracle(p, t, lo=-np.inf, hi=np.inf):
    """np.median of the float32 abs-error array: what error_matrices.py:204, 274 evaluate."""
    return np.median(np.abs(clamp_ref(t, lo, hi) - clamp_ref(p, lo, hi)))


def confusion_oracle(p, t, ratio):
    """(int counts TP, FP, TN, FN, equal; float64 sum d^2), error_matrices.py:384-395."""
    p, t = np.asarray(p, np.float32).reshape(-1), np.asarray(t, np.float32).reshape(-1)
    m = np.where(p > np.float32(ratio), 1, 0)
    counts = [int(np.sum((t == 1) & (m == 1))), int(np.sum((t == 0) & (m == 1))), int(np.sum((t == 0) & (m == 0))),
              int(np.sum((t == 1) & (m == 0))), int(np.sum(m == t))]
    d = (t - p).astype(np.float64)
    return counts, float((d * d).sum())


# ---- seeded inputs shared with tests/test_meters_gpu.py --------------------------------------------------------------------------
def lidar_pair(seed=0, drop=0.1):
    """(pred, truth) range images [66, 1030] float32 in metres: a street scene and a prediction of it -- noise on the returns, and its
    own 10 % of dropped rays.  Where neither has a return the error is exactly 0: ties for the select (18 % of the frame at the
    generator's default drop rate, 36 % at drop = 0.3, about the share of a measured KITTI-360 frame)."""
    from nvsf import synthetic as S
    rng = np.random.default_rng(seed)
    truth = S.street_range_image(rng, drop=drop)[0]
    pred = np.where(truth > 0, truth + rng.normal(0.0, 0.15, truth.shape), 0.0).astype(np.float32)
    pred[rng.random(truth.shape) < 0.1] = 0.0
    return pred, truth


def camera_pair(seed=0, H=376, W=1408):
    """(pred, truth) smooth images [H, W, 3] float32 in [0, 1]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    truth = np.zeros((H, W, 3))
    for c in range(3):
        for _ in range(6):
            fy, fx, ph = rng.uniform(0.002, 0.05), rng.uniform(0.002, 0.05), rng.uniform(0, 2 * np.pi)
            truth[..., c] += rng.uniform(0.05, 0.2) * np.sin(fy * y + fx * x + ph)
    truth = np.clip(0.5 + truth, 0.0, 1.0)
    pred = np.clip(truth + 0.05 * np.sin(0.03 * x + 0.02 * y)[..., None] + rng.normal(0.0, 0.02, truth.shape), 0.0, 1.0)
    return pred.astype(np.float32), truth.astype(np.float32)


# ---- tests -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,size,sample_cov", [(UNIFORM, 7, True), (GAUSSIAN, 11, False), (UNIFORM, 3, False), (GAUSSIAN, 5, True)])
def test_oracle_equals_literal_window_loop(window, size, sample_cov):
    rng = np.random.default_rng(3)
    for shape in ((size, size), (size + 4, size + 9), (15, 17, 3)):
        t = rng.random(shape).astype(np.float32)
        p = np.clip(t + rng.normal(0, 0.1, shape), 0, 1).astype(np.float32)
        R = float(t.max() - t.min())
        got, want = ssim_oracle(p, t, R, window, size, 1.5, sample_cov), ssim_literal(p, t, R, window, size, 1.5, sample_cov)
        assert got == pytest.approx(want, rel=1e-12), (shape, got, want)


def test_identical_images_give_exactly_one():
    rng = np.random.default_rng(4)
    t = rng.random((20, 31, 3)).astype(np.float32)
    assert ssim_oracle(t, t, 1.0, UNIFORM, 7, sample_cov=True) == 1.0
    assert ssim_oracle(t, t, 1.0, GAUSSIAN, 11, 1.5) == 1.0


def test_gaussian_weights_are_the_published_ones():
    w = gaussian_weights(11, 1.5)
    assert w.sum() == pytest.approx(1.0, abs=1e-15) and np.array_equal(w, w[::-1])
    assert w[5] / w[4] == pytest.approx(np.exp(0.5 / 1.5 ** 2), rel=1e-14)


def test_price_of_the_fp64_deviation(capsys):
    """What evaluating in fp64 changes against the libraries' fp32 arithmetic (DESIGN.md 9d records the printed figures).
    torchmetrics filters in the input's fp32: E[pp] - E[p]^2 then carries an absolute error of a few fp32 ulps of E[pp] <= 1, about
    2e-7, against a denominator of at least C2 = 9e-4 -- per pixel at most a few 1e-4, so 1e-3 bounds the mean.  numpy's fp32 pairwise
    mean of 1.6 M squares is good to a few ulps: 1e-5 relative bounds RMSE and PSNR's argument."""
    import torch.nn.functional as F
    p, t = camera_pair(0)
    R = max(float(p.max() - p.min()), float(t.max() - t.min()))
    want = ssim_oracle(p, t, R, GAUSSIAN, 11, 1.5)
    g = torch.from_numpy(gaussian_weights(11, 1.5)).float()
    kernel = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    a, b = (torch.from_numpy(v).permute(2, 0, 1)[None] for v in (p, t))
    mom = F.conv2d(torch.cat([a, b, a * a, b * b, a * b]), kernel, groups=3)  # fp32, valid positions only
    ma, mb, maa, mbb, mab = mom
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    s32 = ((2 * ma * mb + c1) * (2 * (mab - ma * mb) + c2)) / ((ma * ma + mb * mb + c1) * ((maa - ma * ma) + (mbb - mb * mb) + c2))
    d_ssim = abs(float(s32.mean()) - want)
    rmse32 = float(np.sqrt(((t - p) ** 2).mean()))                       # the reference: fp32 throughout
    s = stats_oracle(p, t)
    rmse64 = float(np.sqrt(s[0] / p.size))
    psnr32, psnr64 = float(-10 * np.log10(np.mean((p - t) ** 2) + 1e-8)), float(-10 * np.log10(s[0] / p.size + 1e-8))
    with capsys.disabled():
        print(f"\nfp64 deviation on 376 x 1408 x 3: SSIM fp64 {want:.12f}, |fp32 torch - fp64| = {d_ssim:.3e}; "
              f"RMSE fp64 {rmse64:.10f}, rel |fp32 numpy - fp64| = {abs(rmse32 - rmse64) / rmse64:.3e}; "
              f"PSNR |fp32 - fp64| = {abs(psnr32 - psnr64):.3e} dB")
    assert d_ssim <= 1e-3
    assert abs(rmse32 - rmse64) <= 1e-5 * rmse64 and abs(psnr32 - psnr64) <= 1e-4


def _with_rows(meter, rows, counts):
    """A meter whose device rows are replaced by host arrays: report formats need no device."""
    meter.N = len(rows)
    meter.rows = lambda: (np.asarray(rows, dtype=np.float64), np.asarray(counts, dtype=np.float64))
    return meter


def test_report_strings_match_the_reference_formats():
    from nvsf.nerf import meters as M
    n = 100.0
    stats = [[4.0, 10.0, 0.0, 1.0, 0.0, 1.0], [1.0, 5.0, 0.0, 1.0, 0.0, 1.0]]
    assert re.fullmatch(r"PSNR = -?\d+\.\d{3}", _with_rows(M.PSNRMeter(), stats, [n, n]).report())
    assert _with_rows(M.PSNRMeter(), stats, [n, n]).measure() == pytest.approx(np.mean([-10 * np.log10(0.04 + 1e-8), -10 * np.log10(0.01 + 1e-8)]))
    assert _with_rows(M.RMSEMeter(rgb_metric=True), stats, [n, n]).report() == "RMSE = 0.150"
    assert _with_rows(M.RMSEMeter(), stats, [n, n]).report() == "RMSE_intensity = 0.150"
    assert _with_rows(M.MAEMeter(), stats, [n, n]).report() == "MAE_intensity = 0.075"
    row = stats[0] + [1.0, 0.125, 0.75, float("nan")]
    depth = _with_rows(M.DepthMeter_L4D(scale=0.01), [row], [n])
    want = np.array([0.2, 0.125, np.nan, 0.75, 10 * np.log10(6400 / 0.04)])
    assert np.allclose(depth.measure(), want, equal_nan=True)
    assert depth.report() == f"Depth_error (RMSE, MedAE, LPIPS, SSIM, PNSR) = {depth.measure()}" and "nan" in depth.report()
    inten = _with_rows(M.IntensityMeter_L4D(scale=1), [row], [n])
    assert inten.report().startswith("Intensity_error (RMSE, MedAE, LPIPS, SSIM, PNSR) = [")
    assert inten.measure()[4] == pytest.approx(10 * np.log10(1 / 0.04))
    counts = np.array([[30, 10, 50, 10, 80]], dtype=np.int64).view(np.float64)
    drop = _with_rows(M.RaydropMeter(0.5), np.concatenate([counts, [[9.0]]], axis=1), [n])
    assert np.allclose(drop.measure(), [0.3, 0.8, 0.75])  # precision = recall = 0.75
    assert drop.report() == f"Rdrop_error (RMSE, Accuracy, F_score) = {drop.measure()}"
    ssim = _with_rows(M.SSIMMeter(), [stats[0] + [1.0, 0.5], stats[0] + [1.0, float("nan")]], [n, n])
    assert ssim.report() == "SSIM = 0.250"  # a NaN frame counts as 0 (error_matrices.py:459)
    res = {"chamfer_distance": 0.12345, "f_score": 0.9, "depth": list(want), "intensity": list(want), "raydrop": [0.3, 0.8, 0.75],
           "rgb_rmse": 0.15, "psnr": 20.0, "rgb_ssim": 0.25}
    lines = M.table_report(res)
    assert lines[0] == "Points_error(CD, F-score) = [0.123, 0.9]" and lines[-1] == "SSIM = 0.250" and lines[-2] == "PSNR = 20.000"

    class Writer:
        def __init__(self):
            self.tags = []

        def add_scalar(self, tag, value, step):
            self.tags.append(tag)
    w = Writer()
    depth.write(w, 3, prefix="LiDAR", suffix="_x")
    inten.write(w, 3, prefix="LiDAR")
    drop.write(w, 3, prefix="LiDAR")
    ssim.write(w, 3, prefix="RGB")
    assert w.tags == ["LiDAR/depth error_x", "LiDAR/intensity error", "LiDAR/raydrop error", "RGB/SSIM"]


def test_meters_refuse_cpu_tensors_loudly():
    from nvsf import _hip
    from nvsf.nerf import meters as M
    p, t = torch.rand(1, 16, 24), torch.rand(1, 16, 24)
    for meter in (M.PSNRMeter(), M.RMSEMeter(True), M.MAEMeter(), M.DepthMeter_L4D(0.01), M.IntensityMeter_L4D(1), M.RaydropMeter(0.5)):
        with pytest.raises(_hip.NvsfHipError, match="no CPU fallback"):
            meter.update(p, t)
        assert meter.N == 0
    with pytest.raises(_hip.NvsfHipError, match="no CPU fallback"):
        M.SSIMMeter().update(torch.rand(1, 16, 24, 3), torch.rand(1, 16, 24, 3))
    with pytest.raises(TypeError):
        M.PSNRMeter().update(p.numpy(), t.numpy())
    for fn in (M.image_error_stats, M.median_abs_error, M.raydrop_confusion):
        with pytest.raises(_hip.NvsfHipError):
            fn(p, t)
    with pytest.raises(_hip.NvsfHipError):
        M.ssim_mean(p[0], t[0], torch.ones(1, dtype=torch.float64))


def test_evaluate_frames_signature_defaults():
    from nvsf.nerf.evaluate import evaluate_frames
    params = inspect.signature(evaluate_frames).parameters
    assert params["meters"].default is None and params["intensity_inv_scale"].default == 1
    assert "outside this package's scope" not in evaluate_frames.__doc__


def test_workspace_sizes_follow_the_header():
    from nvsf.nerf import meters as M
    assert M.stats_ws_bytes(1) == 64 and M.stats_ws_bytes(1025) == 128 and M.stats_ws_bytes(1 << 30) == 64 * 2048
    assert M.confusion_ws_bytes(67980) == 48 * 67 and M.MEDIAN_WS_BYTES == 16448
    assert M.ssim_ws_bytes(7, 7, 7) == 8 and M.ssim_ws_bytes(376, 1408, 11) == 8 * 44 * 23
