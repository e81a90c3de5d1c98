"""CPU side of whole-frame evaluation (nvsf/nerf/evaluate.py): the layout of evaluate_frames' statistics vector packed by two
"ranks", added and unpacked against means taken directly from the per-frame values; eval_step / test_step over a stub model and a stub
refiner (what reaches the renders, the gate, the masks, the loss formula); the one table feeder of nvsf/nerf/meters.py on stub meters."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))

BASE = {"loss", "psnr", "depth_rmse_m", "chamfer_distance", "f_score", "frames"}
TABLE = {"depth", "intensity", "raydrop", "rgb_ssim", "rgb_rmse"}
SPLIT = {"depth", "intensity", "raydrop", "chamfer_distance", "f_score", "rgb_psnr", "rgb_ssim"}
WIDTHS = {"depth": 5, "intensity": 5, "raydrop": 3}


def _expected_keys(table, rgb_depth, splits):
    keys = set(BASE)
    if table:
        keys |= TABLE | ({"rgb_depth_rmse"} if rgb_depth else set())
        if splits:
            keys |= {f"{k}_{s}" for s in ("static", "dynamic") for k in SPLIT | ({"rgb_depth_rmse"} if rgb_depth else set())}
    return keys


def _frame_values(layout, n_frames):
    """Per-frame values in which every column of every frame is a distinct small integer; "frames" counts one per frame."""
    vals, c = {}, 1
    for key, w, _ in layout:
        if key == "frames":
            vals[key] = np.ones(n_frames)
            continue
        vals[key] = np.arange(c, c + n_frames * w, dtype=np.float64).reshape(n_frames, w)
        c += n_frames * w
    return vals


CONFIGS = [(False, False, False), (True, False, False), (True, True, False), (True, True, True), (True, False, True)]


@pytest.mark.parametrize("table,rgb_depth,splits", CONFIGS)
def test_layout_round_trip_over_two_ranks(table, rgb_depth, splits):
    from nvsf.nerf.evaluate import pack_sums, stats_layout, unpack_means
    layout = stats_layout(table, rgb_depth, splits)
    stem = lambda key: key.replace("_static", "").replace("_dynamic", "")
    assert all((kind == "list") == (stem(k) in WIDTHS) and w == WIDTHS.get(stem(k), 1) for k, w, kind in layout if k != "frames")
    vals = _frame_values(layout, 3)
    assert len({float(x) for k, v in vals.items() if k != "frames" for x in v.ravel()}) == sum(3 * w for k, w, _ in layout if k != "frames")
    # the host metrics arrive as lists of Python floats, everything else as arrays
    rank = lambda rows: {k: [float(v[r, 0]) for r in rows] if k in ("loss", "psnr", "depth_rmse_m") else v[rows] for k, v in vals.items()}
    a, b = pack_sums(layout, rank([0, 2])), pack_sums(layout, rank([1]))
    assert len(a) == len(b) == sum(w for _, w, _ in layout) and all(type(x) is float for x in a + b)
    res = unpack_means(layout, [x + y for x, y in zip(a, b)])
    assert set(res) == _expected_keys(table, rgb_depth, splits)
    assert res["frames"] == 3 and type(res["frames"]) is int
    for key, v in res.items():
        if key == "frames":
            continue
        want = vals[key].sum(0) / 3
        if stem(key) in WIDTHS:
            assert type(v) is list and len(v) == WIDTHS[stem(key)] and all(type(x) is float for x in v)
            assert v == [float(x) for x in want], key
        else:
            assert type(v) is float and v == float(want[0]), key


@pytest.mark.parametrize("table,rgb_depth,splits", CONFIGS)
def test_layout_zero_frames(table, rgb_depth, splits):
    from nvsf.nerf.evaluate import pack_sums, stats_layout, unpack_means
    layout = stats_layout(table, rgb_depth, splits)
    vals = {k: [] if k in ("loss", "psnr", "depth_rmse_m") else v[:0] for k, v in _frame_values(layout, 1).items()}
    res = unpack_means(layout, pack_sums(layout, vals))
    assert set(res) == _expected_keys(table, rgb_depth, splits)
    assert res["frames"] == 0 and type(res["frames"]) is int
    assert res["loss"] == 0.0 and (not table or res["depth"] == [0.0] * 5)


def test_pack_sums_keeps_the_two_summation_orders():
    """Over many frames np.sum of a list (pairwise) and the sum of a matrix over its first axis (frame after frame) round differently;
    the host metrics have always had the first, every other column the second."""
    from nvsf.nerf.evaluate import pack_sums, stats_layout, unpack_means
    F = 300
    rng = np.random.default_rng(0)
    layout = stats_layout(True, False, False)
    vals = {k: rng.standard_normal((F, w)) * 1e3 for k, w, _ in layout}
    vals["frames"] = np.ones(F)
    for k in ("loss", "psnr", "depth_rmse_m"):
        vals[k] = [float(x) for x in vals[k][:, 0]]
    res = unpack_means(layout, pack_sums(layout, vals))
    for k in ("loss", "psnr", "depth_rmse_m"):
        assert res[k] == float(np.sum(vals[k])) / F
    cdf = np.concatenate([vals["chamfer_distance"], vals["f_score"]], axis=1).sum(0)
    assert (res["chamfer_distance"], res["f_score"]) == (float(cdf[0]) / F, float(cdf[1]) / F)
    t = np.concatenate([vals[k] for k in ("depth", "intensity", "raydrop", "rgb_ssim", "rgb_rmse")], axis=1).sum(0)
    assert res["depth"] == [float(x) / F for x in t[0:5]] and res["raydrop"] == [float(x) / F for x in t[10:13]]
    assert res["rgb_ssim"] == float(t[13]) / F and res["rgb_rmse"] == float(t[14]) / F
    seq = 0.0
    for x in vals["loss"]:
        seq += x
    assert float(np.sum(vals["loss"])) != seq  # the two orders do differ on these values


# ---- frame prediction on a stub ---------------------------------------------------------------------------------------------------
B, HL, WL, H, W = 2, 3, 5, 4, 6


class StubModel:
    """render() returns fixed planes and records its keyword arguments."""

    def __init__(self):
        g = torch.Generator().manual_seed(0)
        r = lambda *s: torch.rand(*s, generator=g)
        self.planes = {"image_lidar": r(B, HL * WL, 2), "depth_lidar": r(B, HL * WL) * 10, "image": r(B, H * W, 3), "depth": r(B, H * W) * 10}
        self.calls = []

    def render(self, o, d, t, staged=False, **k):
        assert staged
        self.calls.append(k)
        return dict(self.planes)


def stub_refiner(raydrop, intensity, depth, thres=0.5):
    """Three planes when `thres` is given, the probability alone when it is None."""
    p = 1.0 - raydrop * 0.9
    if thres is None:
        return p
    m = (p > thres).float()
    return p, intensity * m, depth * m


def _data(with_masks=False):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g)
    d = {"rays_o_lidar": r(B, HL * WL, 3), "rays_d_lidar": r(B, HL * WL, 3), "rays_o": r(B, H * W, 3), "rays_d": r(B, H * W, 3),
         "time": r(B, 1), "images_lidar": r(B, HL, WL, 3), "images": r(B, H, W, 3), "H_lidar": HL, "W_lidar": WL, "H": H, "W": W}
    d["images_lidar"][..., 0] = (d["images_lidar"][..., 0] > 0.3).float()
    if with_masks:
        d["masks_lidar"] = (r(B, HL, WL) > 0.5).float()
        d["masks"] = (r(B, H, W, 1) > 0.5).float()
    return d


NAMES = ("pred_rgb", "pred_rgb_depth", "pred_raydrop", "pred_intensity", "pred_depth")


@pytest.mark.parametrize("refiner", [None, stub_refiner])
def test_test_step_equals_eval_step_on_a_stub(refiner):
    from nvsf.nerf.evaluate import eval_step, test_step
    m, data = StubModel(), _data()
    e = eval_step(m, data, 8, raydrop_thres=0.45, split_rays=False, refiner=refiner)
    t = test_step(m, data, 8, raydrop_thres=0.45, split_rays=False, refiner=refiner)
    for name, got in zip(NAMES, t):
        assert got.shape == e[name].shape and torch.equal(got, e[name]), name
    assert t[2].shape == (B, HL, WL) and t[0].shape == (B, H, W, 3) and t[1].shape == (B, H, W)
    gated = (t[3] == 0) & (t[4] == 0)
    assert 0 < int(gated.sum()) < gated.numel()  # the gate is on, and it matters
    assert [("cal_lidar_color" in k, k.get("bg_color")) for k in m.calls] == [(True, None), (False, 1)] * 2  # LiDAR first, then camera
    assert all(k["perturb"] is False and k["num_steps"] == 8 and k["max_ray_batch"] == 4096 for k in m.calls)


@pytest.mark.parametrize("refiner", [None, stub_refiner])
def test_alpha_r_zero_leaves_the_planes_ungated(refiner):
    from nvsf.nerf.evaluate import test_step
    m, data = StubModel(), _data()
    _, _, rd, it, dp = test_step(m, data, 8, alpha_r=0, raydrop_thres=0.45, split_rays=False, refiner=refiner)
    img = m.planes["image_lidar"].reshape(B, HL, WL, 2)
    assert torch.equal(it, img[..., 1]) and torch.equal(dp, m.planes["depth_lidar"].reshape(B, HL, WL))
    assert torch.equal(rd, img[..., 0] if refiner is None else torch.stack([stub_refiner(img[b, ..., 0], None, None, thres=None) for b in range(B)]))


def test_masks_multiply_the_predictions():
    from nvsf.nerf.evaluate import test_step
    m, plain, masked = StubModel(), _data(), _data(with_masks=True)
    p = test_step(m, plain, 8, raydrop_thres=0.45, split_rays=False)
    q = test_step(m, masked, 8, raydrop_thres=0.45, split_rays=False)
    assert torch.equal(q[0], p[0] * masked["masks"]) and torch.equal(q[1], p[1])  # the image, not its depth
    for i in (2, 3, 4):
        assert torch.equal(q[i], p[i] * masked["masks_lidar"])
    assert not torch.equal(q[0], p[0]) and not torch.equal(q[4], p[4])


def test_bg_color_perturb_and_render_kwargs_reach_the_renders():
    from nvsf.nerf.evaluate import eval_step, test_step
    m, data = StubModel(), _data()
    test_step(m, data, 8, split_rays=False)
    test_step(m, data, 8, split_rays=False, bg_color=0, perturb=True, max_ray_batch=512, upsample_steps=7)
    lidar0, cam0, lidar1, cam1 = m.calls
    assert "bg_color" not in lidar0 and "bg_color" not in lidar1 and cam0["bg_color"] == 1 and cam1["bg_color"] == 0
    assert lidar0["perturb"] is False and cam0["perturb"] is False and lidar1["perturb"] is True and cam1["perturb"] is True
    assert all(k["max_ray_batch"] == 512 and k["upsample_steps"] == 7 for k in (lidar1, cam1)) and "upsample_steps" not in cam0
    m.calls.clear()
    eval_step(m, data, 8, split_rays=False, upsample_steps=7)
    assert all(k["upsample_steps"] == 7 and k["perturb"] is False for k in m.calls) and m.calls[1]["bg_color"] == 1


@pytest.mark.parametrize("refiner", [None, stub_refiner])
def test_eval_step_loss_is_the_documented_formula(refiner):
    """loss = mean-reduced L1 range + MSE ray-drop + MSE intensity + MSE RGB, predictions gated by the predicted mask, the ground truth
    by its own.  Against float64: each fp32 term is a pairwise mean of at most 72 values (log2 72 < 7 roundings) of an expression of at
    most 3 operations, scaled and added to the others (4 more), all terms positive: under 16 unit roundoffs of 2^-24 in all."""
    from nvsf.nerf.evaluate import eval_step
    m, data = StubModel(), _data()
    a_d, a_r, a_i, a_rgb, thres = 0.7, 0.03, 0.2, 1.3, 0.45
    e = eval_step(m, data, 8, alpha_d=a_d, alpha_r=a_r, alpha_i=a_i, alpha_rgb=a_rgb, raydrop_thres=thres, split_rays=False, refiner=refiner)
    img = m.planes["image_lidar"].reshape(B, HL, WL, 2).double()
    rd, it, dp = img[..., 0], img[..., 1], m.planes["depth_lidar"].reshape(B, HL, WL).double()
    if refiner is not None:
        rd = 1.0 - rd * 0.9
    mask = (rd.float() > thres).double()
    gl = data["images_lidar"].double()
    g_rd, g_it, g_dp = gl[..., 0], gl[..., 1] * gl[..., 0], gl[..., 2] * gl[..., 0]
    want = a_d * (dp * mask - g_dp).abs().mean() + a_r * ((rd - g_rd) ** 2).mean() + a_i * ((it * mask - g_it) ** 2).mean() \
        + a_rgb * ((m.planes["image"].reshape(B, H, W, 3).double() - data["images"].double()) ** 2).mean()
    assert e["loss"].dtype == torch.float32 and abs(float(e["loss"]) - float(want)) <= 16 * 2.0 ** -24 * float(want)
    assert torch.equal(e["gt_depth"], data["images_lidar"][..., 2] * data["images_lidar"][..., 0]) and torch.equal(e["gt_rgb"], data["images"])


# ---- the table feeder --------------------------------------------------------------------------------------------------------------
class StubMeter:
    def __init__(self):
        self.fed = []

    def update(self, p, t):
        self.fed.append((p, t))


def test_update_table_feeds_plain_and_masked():
    from nvsf.nerf import meters as M
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.rand(*s, generator=g)
    e = {f"{side}_{k}": r(1, HL, WL) for side in ("pred", "gt") for k in ("depth", "intensity", "raydrop")}
    e.update(pred_rgb=r(1, H, W, 3), gt_rgb=r(1, H, W, 3), pred_rgb_depth=r(1, H, W), gt_rgb_depth=r(1, H, W))
    plain = {k: StubMeter() for k in ("depth", "intensity", "raydrop", "psnr", "rmse", "ssim")}
    M.update_table(plain, e, 2.0)
    for k in ("depth", "intensity", "raydrop"):  # masks=None multiplies nothing: the very tensors of the dictionary
        assert plain[k].fed[0][0] is e["pred_" + k] and plain[k].fed[0][1] is e["gt_" + k]
    assert all(plain[k].fed[0][0] is e["pred_rgb"] and plain[k].fed[0][1] is e["gt_rgb"] and len(plain[k].fed) == 1 for k in ("psnr", "rmse", "ssim"))
    mp, mg, mi = ((r(1, *s) > 0.5).float() for s in ((HL, WL), (HL, WL), (H, W)))
    split = {k: StubMeter() for k in ("depth", "intensity", "raydrop", "psnr", "ssim", "rgb_depth")}
    M.update_table(split, e, 2.0, masks=(mp, mg, mi))
    for k in ("depth", "intensity", "raydrop"):
        assert torch.equal(split[k].fed[0][0], e["pred_" + k] * mp) and torch.equal(split[k].fed[0][1], e["gt_" + k] * mg)
    for k in ("psnr", "ssim"):
        assert torch.equal(split[k].fed[0][0], e["pred_rgb"] * mi[..., None]) and torch.equal(split[k].fed[0][1], e["gt_rgb"] * mi[..., None])
    assert torch.equal(split["rgb_depth"].fed[0][0], e["pred_rgb_depth"] / 2.0 * mi) and torch.equal(split["rgb_depth"].fed[0][1], e["gt_rgb_depth"] * mi)
    assert not hasattr(M, "update_split_table")
