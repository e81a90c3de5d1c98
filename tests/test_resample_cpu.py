"""CPU: the float64 restatement of the hierarchical resampling pass (tests/resample_oracle.py) against the reference's own fp32
`sample_pdf` (tests/golden/resample.npz, written by tests/golden/golden_resample.py), and the host side of the feature: the
ValueError paths, the loud failure on CPU tensors, and the default `hierarchical=False` that ignores `upsample_steps` as before."""
import os

import numpy as np
import pytest
import torch

import resample_oracle as RO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample.npz")
CASES = ((1, 5), (62, 16), (128, 128), (766, 64))


def fixture_case(g, c, det):
    """(bins, weights, u, the reference's samples, bin width [B, 1]) of one case of the fixture."""
    tag = f"c{c}_{'det' if det else 'rand'}_"
    bins, w = g[f"c{c}_bins"], g[f"c{c}_weights"]
    width = ((bins[:, -1].astype(np.float64) - bins[:, 0]) / w.shape[1])[:, None]  # span / (nb - 1)
    return bins, w, g[tag + "u"], g[tag + "samples"], width


@pytest.mark.parametrize("det", [True, False], ids=["det", "rand"])
@pytest.mark.parametrize("c", range(len(CASES)), ids=[f"nw{a}_U{b}" for a, b in CASES])
def test_oracle_against_the_reference_fixture(c, det):
    """Every sample within one bin width of the reference's; at most 0.1 % of a case beyond 0.01 bin width (the reference runs in fp32:
    its cdf carries ~1e-7 per entry, which moves a sample by up to a bin where the pdf is ~1e-5 / sum; measured when the fixture was
    written: at most 0.85 bin widths and a share of 7.4e-4, both in the (766, 64) random case)."""
    g = np.load(GOLD)
    assert tuple(map(tuple, g["cases"])) == CASES
    bins, w, u, ref, width = fixture_case(g, c, det)
    nw, U = CASES[c]
    assert bins.shape == (64, nw + 1) and w.shape == (64, nw) and ref.shape == (64, U) and u.shape == ((U,) if det else (64, U))
    assert not w[:8].any() and w[8:].any()  # the empty eighth
    got = RO.sample_pdf(bins, w, u)
    worst, share = RO.reference_conditions(got, ref, width)
    print(f"(nb - 1, U) = {CASES[c]} det = {det}: largest difference {worst:.3g} bin widths, share beyond 0.01 bin width {share:.3g}")
    assert worst <= 1.0
    assert share <= 1e-3


def test_oracle_merge_is_stable_and_a_permutation():
    rng = np.random.default_rng(0)
    N, T, U = 7, 9, 6
    z = np.sort(rng.random((N, T)).astype(np.float32), -1)
    z[0, 3] = z[0, 4] = z[0, 5]  # a plateau: the bins around it coincide, the one-hot weight below puts every draw on it
    w = rng.random((N, T)).astype(np.float32)
    w[0] = 0
    w[0, 4] = 1e6
    o, d = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    r = RO.resample_merge(o, d, np.array([-1, -1, -1, 1, 1, 1], np.float32), z, w, np.linspace(0.1, 0.9, U, dtype=np.float32), bound=1.0)
    assert (np.sort(r["src"], -1) == np.arange(T + U)).all()
    assert (np.diff(r["z_merged"], axis=-1) >= 0).all() and (np.diff(r["z_new"], axis=-1) >= 0).all()
    assert (r["z_new"][0] == z[0, 4]).all()
    assert list(r["src"][0, 3:6]) == [3, 4, 5] and list(r["src"][0, 6:6 + U]) == list(range(T, T + U))  # coarse first on equal values
    assert r["x01"].min() >= 0 and r["x01"].max() <= 1


def _Recorder():
    """A field on NeRFRenderer that records what the renderer asks of it: the fused no-grad render (so that `run` needs no device)."""
    from nvsf.nerf.models.renderer_dynamic import NeRFRenderer

    class Recorder(NeRFRenderer):
        def __init__(self):
            super().__init__(bound=2, min_near_lidar=0.01, lidar_max_depth=0.8)
            self.out_color_dim, self.out_lidar_color_dim = 3, 2
            self.calls = []

        def fused_uniform_render(self, rays_o, rays_d, nears, fars, T, aabb, noise, cal_lidar_color, bg_host, **kwargs):
            self.calls.append((T, None if noise is None else noise.clone(), sorted(k for k in kwargs if k != "time")))
            N = rays_o.shape[0]
            z = nears[:, None] + (fars - nears)[:, None] * torch.linspace(0, 1, T)[None]
            return z, torch.zeros(N, T), torch.zeros(N), torch.zeros(N), torch.zeros(N, self.out_lidar_color_dim)
    return Recorder()


def _rays(N=4):
    g = torch.Generator().manual_seed(0)
    d = torch.randn(1, N, 3, generator=g)
    return torch.zeros(1, N, 3), d / d.norm(dim=-1, keepdim=True), torch.tensor([[0.5]])


def test_default_ignores_upsample_steps():
    """hierarchical=False (the default): `upsample_steps` changes nothing -- same calls into the field, same random draws, same result."""
    m = _Recorder().eval()
    o, d, t = _rays()
    outs = []
    with torch.no_grad():
        for kw in ({}, {"upsample_steps": 0}, {"upsample_steps": 128}, {"upsample_steps": 7, "hierarchical": False}):
            torch.manual_seed(3)
            outs.append(m.run(o, d, t, cal_lidar_color=True, num_steps=16, perturb=True, **kw))
            after = torch.rand(1)
            if len(outs) > 1:
                assert torch.equal(after, after0)  # no further draw was made
            after0 = after
    assert len(m.calls) == 4
    for T, noise, kwargs in m.calls:
        assert T == 16 and torch.equal(noise, m.calls[0][1]) and kwargs == []  # neither keyword leaks into the field's kwargs
    for out in outs:
        assert tuple(out["z_vals"].shape) == (4, 16) and torch.equal(out["z_vals"], outs[0]["z_vals"])
    # staged render passes the keyword through as well
    with torch.no_grad():
        m.render(o, d, t, cal_lidar_color=True, staged=True, num_steps=16, upsample_steps=5, hierarchical=False)
    assert m.calls[-1][0] == 16 and m.calls[-1][2] == ["rays_in_image_order"]


def test_hierarchical_bypasses_the_fused_render_and_fails_without_a_device():
    from nvsf import _hip
    m = _Recorder().eval()
    o, d, t = _rays()
    for staged in (False, True):
        with torch.no_grad(), pytest.raises(_hip.NvsfHipError):  # the operator chain's first kernel is handed a CPU tensor
            m.render(o, d, t, cal_lidar_color=True, staged=staged, num_steps=16, upsample_steps=4, hierarchical=True)
    assert m.calls == []


def test_value_errors():
    from nvsf import field_ops as ops
    m = _Recorder().eval()
    o, d, t = _rays()
    run = lambda **kw: m.run(o, d, t, cal_lidar_color=True, **kw)
    with pytest.raises(ValueError, match="num_steps >= 3"):
        run(num_steps=2, upsample_steps=4, hierarchical=True)
    for U in (0, -1):
        with pytest.raises(ValueError, match="upsample_steps >= 1"):
            run(num_steps=16, upsample_steps=U, hierarchical=True)
    with pytest.raises(ValueError, match=f"num_steps <= {ops.RESAMPLE_MAX_COARSE}"):
        run(num_steps=ops.RESAMPLE_MAX_COARSE + 1, upsample_steps=4, hierarchical=True)
    with pytest.raises(ValueError, match=f"upsample_steps <= {ops.RESAMPLE_MAX_FINE}"):
        run(num_steps=16, upsample_steps=ops.RESAMPLE_MAX_FINE + 1, hierarchical=True)
    ops.check_resample_sizes(ops.RESAMPLE_MAX_COARSE, ops.RESAMPLE_MAX_FINE)
    ops.check_resample_sizes(768, 128)  # the defaults of run's signature
    assert m.calls == []
    with pytest.raises(ValueError, match="occupancy-grid"):
        m.run_cuda(o, d, t, cal_lidar_color=True, hierarchical=True)
    m.cuda_ray = True
    with pytest.raises(ValueError, match="occupancy-grid"):
        m.render(o, d, t, cal_lidar_color=True, hierarchical=True, upsample_steps=4)
    # the thin calls check their sizes before any pointer is taken
    with pytest.raises(ValueError, match="at most"):
        ops.sample_pdf(torch.zeros(2, ops.RESAMPLE_MAX_BINS + 1), torch.zeros(2, ops.RESAMPLE_MAX_BINS), torch.zeros(4))
    with pytest.raises(ValueError, match="num_steps >= 3"):
        ops.resample_merge(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(6), torch.zeros(2, 2), torch.zeros(2, 2), torch.zeros(4))
    with pytest.raises(ValueError, match=r"\[U\]"):
        ops.resample_merge(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(6), torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(3, 4))
    from nvsf.nerf.models.renderer_dynamic import sample_pdf
    with pytest.raises(ValueError, match="n_samples"):
        sample_pdf(torch.zeros(2, 5), torch.zeros(2, 4), 8, u=torch.zeros(4))


def test_train_step_checks_upsample_steps():
    from nvsf.nerf.models.network_static import NeRFNetworkStatic
    from nvsf.nerf.train_step import RenderTrainStep
    m = NeRFNetworkStatic(bound=2, log2_hashmap_size=8)
    assert RenderTrainStep(m, ema_decay=None)._resample_kw == {}
    assert RenderTrainStep(m, ema_decay=None, num_steps=32, upsample_steps=16)._resample_kw == {"hierarchical": True, "upsample_steps": 16}
    with pytest.raises(ValueError):
        RenderTrainStep(m, ema_decay=None, num_steps=32, upsample_steps=-1)
    with pytest.raises(ValueError, match="upsample_steps <= 256"):
        RenderTrainStep(m, ema_decay=None, num_steps=32, upsample_steps=257)
    with pytest.raises(ValueError, match="num_steps >= 3"):
        RenderTrainStep(m, ema_decay=None, num_steps=2, upsample_steps=4)
    m.cuda_ray = True  # what enable_occupancy_grid() sets: render() would go to run_cuda, which has no hierarchical pass
    with pytest.raises(ValueError, match="occupancy-grid"):
        RenderTrainStep(m, ema_decay=None, num_steps=32, upsample_steps=16)
    assert RenderTrainStep(m, ema_decay=None, num_steps=32)._resample_kw == {}


def test_cpu_tensors_fail_loudly():
    """No CPU fallback: the new ops raise on a CPU tensor, as every other op does, before anything is computed."""
    from nvsf import _hip
    from nvsf import field_ops as ops
    from nvsf.nerf.models.renderer_dynamic import sample_pdf
    with pytest.raises(_hip.NvsfHipError):
        ops.sample_pdf(torch.rand(2, 5), torch.rand(2, 4), torch.rand(8))
    with pytest.raises(_hip.NvsfHipError):
        sample_pdf(torch.rand(2, 5), torch.rand(2, 4), 8, det=True)
    with pytest.raises(_hip.NvsfHipError):
        ops.resample_merge(torch.zeros(2, 3), torch.ones(2, 3), torch.tensor([-1., -1, -1, 1, 1, 1]), torch.rand(2, 8).sort(-1)[0],
                           torch.rand(2, 8), torch.rand(4))
    with pytest.raises(_hip.NvsfHipError):
        ops.MergeRowsFn.apply(torch.rand(2, 8, 3), torch.rand(2, 4, 3), torch.arange(12, dtype=torch.int32).repeat(2, 1))
    with pytest.raises(ValueError):
        ops.MergeRowsFn.apply(torch.rand(2, 8, 3), torch.rand(2, 4, 3), torch.arange(12).repeat(2, 1))  # int64 index
    with pytest.raises(ValueError):
        ops.MergeRowsFn.apply(torch.rand(8), torch.rand(4), torch.arange(12, dtype=torch.int32).repeat(2, 1))  # rows without a ray axis
