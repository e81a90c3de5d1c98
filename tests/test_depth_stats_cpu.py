"""CPU: the float64 restatement of the depth statistics (tests/depth_stats_oracle.py) against independent
forms -- the inversion of the piecewise-linear CDF with np.interp, central differences, direct numpy -- on the cases the GPU tests
share, the two-surface ray the statistics exist for, the edge rows, and the refusals of the Python surface that need no device."""
import numpy as np
import pytest
import torch

import depth_stats_oracle as O


def _f64(c):
    return tuple(c[k].double() for k in ("w", "z", "nears", "fars"))


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "absolute"])
@pytest.mark.parametrize("shape", [(5, 3), (5, 64), (67, 65), (5, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantile_inverts_the_piecewise_linear_cdf(shape, normalize):
    """Rows without zero weights: the CDF through (z_i, C_{i-1}) and (z_{T-1} + delta_{T-1}, W) is strictly increasing, and np.interp
    of tau on it is t_q.  Bar: 1e-12, the interpolation's own fp64 operations on depths below 2, plus what the last bit of the cumsum
    does to (tau - C_{i-1}) / w_i where w_i is tiny: the oracle's scan_error delta_i / w_i."""
    N, T = shape
    w, z, nears, fars = _f64(O.case(N, T, "random"))
    assert bool((w > 0).all())
    levels = (0.05, 0.25, 0.5, 0.95, 1.0) if normalize else (0.05, 0.15, 0.5)
    s = O.stats(w, z, nears, fars, levels, normalize)
    delta = O.intervals(z, nears, fars)
    seen = 0
    for n in range(N):
        xs = np.concatenate([z[n].numpy(), [float(z[n, -1] + delta[n, -1])]])
        cdf = np.concatenate([[0.0], np.cumsum(w[n].numpy())])
        for l, q in enumerate(levels):
            tau = q * cdf[-1] if normalize else q
            got = float(s["quantiles"][n, l])
            if tau > cdf[-1]:
                assert got == 0.0
                continue
            seen += 1
            p = s["parts"][l]
            tol = 1e-12 + float(O.scan_error(T, p["W"][n]) * p["delta"][n] / p["wi"][n])
            assert abs(got - float(np.interp(tau, cdf, xs))) <= tol, (n, q)
    assert seen >= N


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "absolute"])
def test_gradient_agrees_with_central_differences(normalize):
    """t_q is linear-fractional in w inside a crossing sample: with h = 1e-7 the central difference is off by O(h^2 t''') + rounding /
    h, about 1e-8 relative to the largest entry of a row (r = delta / w up to ~1e3 here)."""
    N, T = 5, 16
    w, z, nears, fars = _f64(O.case(N, T, "random"))
    levels = (0.25, 0.5, 0.95) if normalize else (0.05, 0.15, 0.5)
    gq = O.grad_seed(N, len(levels)).double()
    ref = O.quantile_grad(w, z, nears, fars, levels, normalize, gq)
    base = O.stats(w, z, nears, fars, levels, normalize)
    assert all(float(p["margin"].min()) > 1e-5 for p in base["parts"])  # h moves no crossing
    h = 1e-7
    num = torch.zeros_like(ref)
    for j in range(T):
        e = torch.zeros(T, dtype=torch.float64)
        e[j] = h
        up = O.stats(w + e, z, nears, fars, levels, normalize)["quantiles"]
        dn = O.stats(w - e, z, nears, fars, levels, normalize)["quantiles"]
        num[:, j] = ((up - dn) * gq).sum(dim=1) / (2 * h)
    scale = ref.abs().max(dim=1, keepdim=True).values
    assert float(((num - ref).abs() / scale).max()) <= 1e-6
    assert float(ref.abs().max()) > 0
    if not normalize:  # a ray whose total stays below the level returned 0 and gets a zero row
        dead = ~base["parts"][2]["ok"]
        assert bool(dead.any()) and bool((base["quantiles"][dead, 2] == 0).all())
        only = O.quantile_grad(w, z, nears, fars, levels[2:], normalize, gq[:, 2:])
        assert bool((only[dead] == 0).all()) and bool((only[~dead] != 0).any())


def test_gradient_formula_of_the_design_section():
    """The closed form of section 9n against autograd, one level: r (q - [j < i]) off the crossing sample, r q - delta a / w^2 on it."""
    N, T = 5, 63
    w, z, nears, fars = _f64(O.case(N, T, "random"))
    for normalize in (True, False):
        q = 0.5 if normalize else 0.1
        p = O.quantile_parts(w, z, nears, fars, q, normalize)
        r = p["delta"] / p["wi"]
        j = torch.arange(T)[None, :]
        form = r[:, None] * ((q if normalize else 0.0) - (j < p["idx"][:, None]).double())
        form = form - (j == p["idx"][:, None]) * (p["delta"] * p["a"] / p["wi"] ** 2)[:, None]
        form = form * p["ok"][:, None]
        ref = O.quantile_grad(w, z, nears, fars, (q,), normalize, torch.ones(N, 1))
        assert float((form - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("kind", O.KINDS)
def test_mode_and_std_against_direct_numpy(kind):
    N, T = 67, 65
    w, z, nears, fars = _f64(O.case(N, T, kind))
    s = O.stats(w, z, nears, fars)
    for n in range(N):
        wn, zn = w[n].numpy(), z[n].numpy()
        if wn.sum() == 0:
            assert float(s["mode"][n]) == 0.0 and float(s["std"][n]) == 0.0
            continue
        assert float(s["mode"][n]) == zn[int(np.argmax(wn))]  # np.argmax: the first maximum
        std = np.sqrt(np.average((zn - np.average(zn, weights=wn)) ** 2, weights=wn))
        assert abs(float(s["std"][n]) - std) <= 1e-13
    if kind == "plateaus":
        assert bool(((w == w.max(dim=1, keepdim=True).values).sum(dim=1) > 1).any())  # ties are there


def test_two_surface_ray():
    """0.45 of the weight on each of two surfaces: the mean lies between them, on neither; the quartile ranges lie within one interval
    of a surface each, and the strongest return is the first surface."""
    w, z, nears, fars = O.two_surface_ray()
    T = w.shape[1]
    s = O.stats(w, z, nears, fars, (0.25, 0.5, 0.75))
    mean = float((w.double() * z.double()).sum())
    step = 1.0 / T
    assert abs(mean - 0.4) < 0.02 and 0.2 + step < mean < 0.6 - step
    t25, t50, t75 = (float(v) for v in s["quantiles"][0])
    assert 0.2 <= t25 <= 0.2 + step and 0.6 <= t75 <= 0.6 + step
    assert 0.2 + step <= t50 <= 0.6  # the median of a tie between two surfaces falls in the dust between: a quartile is the robust pick
    assert float(s["mode"][0]) == float(z[0, 10]) and abs(float(s["mode"][0]) - 0.2) < 1e-7
    assert float(s["std"][0]) > 0.15  # and the spread says that the ray saw two things


def test_edge_rows():
    T = 8
    z = (torch.arange(T, dtype=torch.float64) / 16)[None].float()
    nears, fars = torch.zeros(1), torch.full((1,), 0.5)  # delta = 1 / 16 everywhere, the last interval included
    row = lambda *v: torch.tensor([list(v) + [0.0] * (T - len(v))])
    s = O.stats(row(), z, nears, fars, (0.5, 1.0))
    assert bool((s["quantiles"] == 0).all()) and float(s["mode"]) == 0 and float(s["std"]) == 0              # all-zero weights
    s = O.stats(row(0.5, 0.25), z, nears, fars, (0.25, 1.0))
    assert float(s["quantiles"][0, 0]) == 0.0 + (1 / 16) * 0.1875 / 0.5                                      # crossing in the first sample
    assert float(s["quantiles"][0, 1]) == 1 / 16 + 1 / 16                                                    # q = 1: the end of the last positive sample
    w_last = torch.zeros(1, T)
    w_last[0, -1] = 0.5
    s = O.stats(w_last, z, nears, fars, (0.5, 1.0))
    assert float(s["quantiles"][0, 0]) == 7 / 16 + 1 / 32 and float(s["quantiles"][0, 1]) == 0.5              # crossing in the last sample
    s = O.stats(torch.tensor([[0.25]]), torch.tensor([[0.125]]), nears, fars, (0.5, 1.0))                     # T = 1: delta = far - near
    assert float(s["quantiles"][0, 0]) == 0.125 + 0.5 * 0.5 and float(s["quantiles"][0, 1]) == 0.625
    assert float(s["mode"]) == 0.125 and float(s["std"]) == 0
    s = O.stats(row(0.25, 0.125), z, nears, fars, (0.25, 0.5), normalize=False)                              # absolute: W = 0.375 < 0.5
    assert float(s["quantiles"][0, 0]) == 1 / 16 and float(s["quantiles"][0, 1]) == 0.0
    g = O.quantile_grad(row(0.25, 0.125), z, nears, fars, (0.5,), False, torch.ones(1, 1))
    assert bool((g == 0).all())                                                                               # "no return" has no gradient


def test_dyadic_case_is_exact_in_fp64():
    """What the GPU test's bit-exact case rests on: with these inputs the cumsum in any order is exact (integers / 1024 below 2^53)."""
    w, z, nears, fars, levels = O.dyadic_case()
    wd = w.double()
    assert bool(((wd * 1024) == (wd * 1024).round()).all()) and bool(((z.double() * 256) == (z.double() * 256).round()).all())
    a = torch.cumsum(wd, dim=1)
    b = torch.flip(torch.cumsum(torch.flip(wd, [1]), dim=1), [1])
    assert bool((a[:, -1] == b[:, 0]).all())
    s = O.stats(w, z, nears, fars, levels)
    assert bool((s["quantiles"][0] == 0).all()) and float(s["quantiles"][1, 3]) == float(z[1, -1]) + 1 / 256
    assert float(s["quantiles"][3, 3]) <= float(z[3, w.shape[1] // 2])  # q = 1 ends at the last positive sample, not at the row's end


@pytest.mark.parametrize("kind", O.KINDS)
def test_shared_cases_have_no_unsettled_ray(kind):
    """The GPU test may leave out a ray whose crossing the scan order can move (margin below the scan error).  The seeds are chosen so
    that the oracle finds none, in any shared case, at either set of levels, in either form."""
    for N, T in O.SHAPES + [O.BIG]:
        for Q in (1, 4):
            for normalize in (True, False):
                if (N, T) == O.BIG and (kind != "random" or not normalize):
                    continue
                s = O.reference(N, T, kind, Q, normalize)
                for p in s["parts"]:
                    assert bool(O.settled(p, T).all()), (N, T, kind, Q, normalize)
                    live = p["ok"]
                    assert bool((p["wi"][live] > 0).all()) and bool((p["a"][live] > 0).all()) and bool((p["a"][live] <= p["wi"][live]).all())


def test_python_surface_refuses_bad_levels_and_modes():
    from nvsf import field_ops as ops
    for bad in (0.0, -0.5, 1.5, float("nan"), (), (0.1, 0.2, 0.3, 0.4, 0.5), (0.5, 0.0)):
        with pytest.raises(ValueError):
            ops.depth_levels(bad)
    assert ops.depth_levels(1) == (1.0,) and ops.depth_levels([0.25, 0.5]) == (0.25, 0.5)
    assert ops.parse_depth_mode("mean") == ("mean", None, True) and ops.parse_depth_mode("mode") == ("mode", None, True)
    assert ops.parse_depth_mode("median") == ("quantile", 0.5, True) and ops.parse_depth_mode(0.9) == ("quantile", 0.9, True)
    assert ops.parse_depth_mode(("absolute", 0.5)) == ("quantile", 0.5, False)
    for bad in ("max", None, 0.0, 2, ("absolute",), ("relative", 0.5), ("absolute", float("nan")), True):
        with pytest.raises(ValueError):
            ops.parse_depth_mode(bad)
    w = torch.rand(3, 4)
    with pytest.raises(ValueError):
        ops.ray_depth_stats(w, w, torch.zeros(3), torch.ones(3), q=2.0)
    with pytest.raises(ValueError):
        ops.ray_depth_stats(w, w, torch.zeros(3), torch.ones(3), want=("mean",))
    with pytest.raises(ValueError):
        ops.ray_depth_stats(w, w[:, :3], torch.zeros(3), torch.ones(3))
    with pytest.raises(ValueError):
        ops.DepthQuantileFn.apply(w, w, torch.zeros(2), torch.ones(3), (0.5,), True)


def test_run_cuda_refuses_depth_modes_without_a_device():
    """The occupancy march has no [N, T] rows: any statistic but the mean is refused before anything touches a device."""
    from nvsf.nerf.models.renderer_dynamic import NeRFRenderer
    r = NeRFRenderer(bound=1)
    rays = torch.zeros(1, 4, 3)
    for kw in (dict(depth_mode="median"), dict(depth_mode="mode"), dict(depth_mode=0.9), dict(depth_stats=True)):
        with pytest.raises(ValueError, match="occupancy-grid march"):
            r.run_cuda(rays, rays, None, **kw)
    with pytest.raises(ValueError, match="depth_mode"):
        r.run_cuda(rays, rays, None, depth_mode="max")
