"""The one-launch gathering render (k_render_uniform<*, false>) serves a coarse level group of a 16-sample tile from ONE gather per lane
when the whole wave sits in the cells of its rows' first and last samples (density_encode, SHARE form: corner c & 7 of cell A / B per
lane, exchanged through a per-wave LDS scratch), and falls back to the per-lane form -- eight gathers per lane -- on any other tile.
Both forms fetch the same table entries, so every output must be bit-identical between

    corner_share = "never"   the per-lane form on every tile,
    corner_share = "gated"   production: a level group tries the shared form on the rays whose step is short enough (lambda below),
    corner_share = "always"  both coarse groups try on every ray, so that the fallback runs where production would not look.

The kernel has no counters: that the ray sets below reach the shared form, the two-cell case and the fallback is shown on the CPU by a
numpy restatement of the cell computation (`floor(scale * x01 + 0.5)` of the clamped sample positions), on the rays of the (64, 128)
batch, with the witness samples at least 1e-3 cell away from every cell face."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_render_static_gpu import _model, _t
from test_density_sliced_gpu import OVERSHOOT_T, _overshoot_batch

SHAPES = [(5, 7, False), (1, 16, False), (9, 48, False), (37, 100, True), (64, 128, False)]
SET_ORDER = "dbcaef"  # ray i of a batch comes from set SET_ORDER[i % 6]
BENCH_T = 768         # the sets keep the step of a T = 768 render, whatever T a case uses


def _consts():
    from nvsf import synthetic as S
    return float(S.BOUND), float(S.MIN_NEAR), float(S.LIDAR_MAX_DEPTH)


def _grid_scales(spec):
    return np.asarray(spec.scales, np.float64)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _x01(o, d, near, far, T, bound):
    """Unit-cube sample positions [n, T, 3] (fused_field.hip sample_z / sample_x01, without jitter) in fp64 from the fp32 inputs."""
    lin = torch.linspace(0.0, 1.0, T).numpy().astype(np.float64)
    o, d, near, far = (np.asarray(a, np.float32).astype(np.float64) for a in (o, d, near, far))
    z = near[:, None] + (far - near)[:, None] * lin[None]
    p = np.clip(o[:, None, :] + d[:, None, :] * z[..., None], -bound, bound)
    return (p + bound) / (2.0 * bound)


def _cells(x01, scale):
    """Cell [.., 3] of every position on a level and its distance (in cells) to the nearest cell face."""
    pos = scale * x01 + 0.5
    c = np.floor(pos)
    fr = pos - c
    return c.astype(np.int64), np.minimum(fr, 1.0 - fr).min(-1)


def _tiles(a, T):
    assert T % 16 == 0
    return a.reshape(a.shape[0], T // 16, 16, *a.shape[2:])


def _slot_eligible(x01, scales, q, T):
    """[n, tiles]: every sample of the tile lies in the cell of the tile's first or last sample on each of the levels 4q .. 4q + 3 (the
    wave-wide condition of the shared form), and the smallest face distance of the tile's samples over those levels."""
    ok, margin = None, None
    for l in range(4 * q, 4 * q + 4):
        c, m = _cells(x01, scales[l])
        c, m = _tiles(c, T), _tiles(m, T)
        in_ab = ((c == c[:, :, :1]).all(-1) | (c == c[:, :, -1:]).all(-1)).all(-1)
        ok = in_ab if ok is None else ok & in_ab
        margin = m.min(-1) if margin is None else np.minimum(margin, m.min(-1))
    return ok, margin


def _distinct(x01, scale, T):
    """[n, tiles] number of distinct cells of a tile on a level, and the tile's smallest face distance."""
    c, m = _cells(x01, scale)
    c, m = _tiles(c, T), _tiles(m, T).min(-1)
    key = (c[..., 0] << 42) + (c[..., 1] << 21) + c[..., 2]
    cnt = np.array([[len(np.unique(t)) for t in ray] for ray in key])
    return cnt, m


def _lidar_step():
    bound, near, far = _consts()
    return (far - near) / BENCH_T


def _ray_set(name, n, T, scales):
    """n rays of a set as fp32 (o, d, near, far); the step along the ray is that of a T = 768 render of the set's kind."""
    bound, min_near, lidar_far = _consts()
    from nvsf import synthetic as S
    rng = np.random.default_rng({"a": 101, "b": 102, "c": 103, "d": 104, "e": 105, "f": 106}[name])
    step = _lidar_step()
    if name == "a":  # the whole ray inside one cell of every level 0 .. 7, far from its faces: a range of 4e-3 level-7 cells
        out = []
        while len(out) < n:
            x0 = rng.uniform(0.1, 0.9, 3)
            if min(_cells(x0[None], scales[l])[1][0] for l in range(8)) >= 0.05:
                out.append(x0)
        x0 = np.array(out)
        d = _unit(rng.standard_normal((n, 3)))
        near = np.full(n, 0.1)
        o = (x0 * 2.0 * bound - bound) - d * near[:, None]
        far = near + 1e-4
    elif name == "b":
        o, d = S.lidar_rays(n, rng)
        near = np.full(n, min_near)
        far = near + step * T
    elif name == "c":
        o, d = S.camera_rays(n, rng)
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        with np.errstate(divide="ignore"):
            t0, t1 = (-bound - o64) / d64, (bound - o64) / d64
        near = np.maximum(np.minimum(t0, t1).max(1), min_near)
        far = near + (np.maximum(t0, t1).min(1) - near) * T / BENCH_T
    elif name == "d":  # along a cube diagonal, 0.02 cell beside a vertex of the level-3 lattice: three faces crossed within six samples
        sign = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float64)[np.arange(n) % 8]
        d = sign / np.sqrt(3.0)
        k = rng.integers(10, 32, (n, 3)).astype(np.float64)
        vertex = (k - 0.5) / scales[3]  # faces of level 3: scale * x + 0.5 integer
        aim = vertex + np.array([0.02, 0.0, -0.02]) / scales[3]
        near = np.full(n, 0.1)
        far = near + step * T
        at = (min(40, T // 2) + 0.37 + np.arange(n) % 16) / max(T - 1, 1)  # sample index (a fraction of it) at which the ray passes `aim`
        o = (aim * 2.0 * bound - bound) - d * (near + (far - near) * at)[:, None]
    elif name == "e":  # leaves the box through the +x face half way: clamped, repeated positions behind it
        d = _unit(np.stack([np.ones(n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)], -1))
        near = np.full(n, 0.1)
        far = near + step * T
        o = np.stack([bound - d[:, 0] * (near + far) / 2.0, rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)], -1)
    elif name == "f":
        d = np.tile(np.array([[-1.0, 0.0, 0.0]]), (n, 1))
        o = rng.uniform(-1.0, 1.0, (n, 3))
        near = np.full(n, 0.1)
        far = near + step * T
    else:
        raise KeyError(name)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return f32(o), f32(d), f32(near), f32(far)


def _batch(N, T, scales):
    per = -(-N // len(SET_ORDER))
    sets = {s: _ray_set(s, per, T, scales) for s in SET_ORDER}
    pick = [(SET_ORDER[i % 6], i // 6) for i in range(N)]
    return tuple(np.stack([sets[s][k][j] for s, j in pick]) for k in range(4))


def _lambda(d, near, far, T, bound, scales):
    """The per-ray figure of the kernel's prologue in fp32, same order of operations: expected cell-face crossings of a 16-sample tile
    at the finest level of group q, 16 * scale(4 q + 3) * (|dx| + |dy| + |dz|) of the step in the unit cube."""
    f = np.float32
    d, near, far = np.asarray(d, f), np.asarray(near, f), np.asarray(far, f)
    sample_dist = (far - near) / f(T)
    inv_extent = f(1.0) / (f(2.0) * f(bound))
    step1 = (sample_dist * inv_extent) * ((np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2]))
    return [(f(16.0) * f(scales[4 * q + 3])) * step1 for q in (0, 1)]


def _lambda_max():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "selfsupervised-nvsf_amd", "csrc", "fused_field.hip")
    m = re.search(r"constexpr float kShareLambdaMax = ([0-9.]+)f;", open(src).read())
    assert m, "kShareLambdaMax not found in fused_field.hip"
    return float(m.group(1))


@pytest.fixture(scope="module")
def field(dev):
    """The config-2 model (L16 F2 T2^19, random fp16 tables) and an L16 F2 grid with a 2^14 table: levels 0-1 dense, 2-15 hashed, so that
    level group 0 mixes both index forms in the general instance."""
    from nvsf import field_ops as ops
    m = _model(dev, 0.1)
    spec = m.hash_encoder_lidar.spec
    assert spec.L == 16 and spec.F == 2 and spec.log2_hashmap_size == 19
    small = ops.GridSpec(3, 16, 2, 14, spec.base_resolution, spec.per_level_scale)
    first_hashed = next(l for l in range(16) if small.res[l] ** 3 > small.offsets[l + 1] - small.offsets[l])
    assert 0 < first_hashed < 4
    g = torch.Generator().manual_seed(7)
    small_table = (torch.randn(small.n_params, generator=g) * 0.1).to(torch.float16).to(dev)
    return m, small, small_table


def _coverage_sets():
    from nvsf import field_ops as ops
    spec = ops.GridSpec(3, 16, 2, 19, 16, float(np.exp(np.log(2048 / 16) / 15)))
    return spec


def test_ray_sets_reach_every_path_of_the_shared_form():
    """Coverage, on the CPU, of the (64, 128) batch's sets (11 rays each; a face distance of 1e-3 cell wherever a claim depends on
    the side a sample is on)."""
    from nvsf import field_ops as ops
    bound = _consts()[0]
    spec = _coverage_sets()
    scales = _grid_scales(spec)
    T, n = 128, 11
    x = {s: _x01(*_ray_set(s, n, T, scales), T, bound) for s in "abcd"}
    for q in (0, 1):  # (a): the shared form on every tile of both groups
        ok, margin = _slot_eligible(x["a"], scales, q, T)
        print(f"set a, group {q}: eligible {ok.mean():.3f}, min face distance {margin.min():.4f}")
        assert ok.all() and margin.min() >= 1e-3
    two = three = 0
    for l in range(4):  # (d): two-cell tiles (cell B in use) and tiles of three or more cells (the fallback inside group 0)
        cnt, margin = _distinct(x["d"], scales[l], T)
        two += int(((cnt == 2) & (margin >= 1e-3)).sum())
        three += int(((cnt >= 3) & (margin >= 1e-3)).sum())
    print(f"set d, levels 0-3: {two} tiles of exactly two cells, {three} tiles of three or more")
    assert two >= 1 and three >= 1
    ok_c, _ = _slot_eligible(x["c"], scales, 1, T)  # (c): group 1 falls back almost everywhere when it is made to try
    print(f"set c, group 1: eligible {ok_c.mean():.4f}")
    assert ok_c.mean() < 0.05
    ok_b0, _ = _slot_eligible(x["b"], scales, 0, T)
    ok_b1, _ = _slot_eligible(x["b"], scales, 1, T)
    print(f"set b: group 0 eligible {ok_b0.mean():.3f}, group 1 {ok_b1.mean():.3f}")
    assert ok_b0.mean() > 0.5 and 0.0 < ok_b1.mean() < 1.0  # LiDAR steps: both forms of group 1 inside one batch


def test_lambda_gate_keeps_lidar_groups_and_drops_the_camera_group_1():
    """Production gate (corner_share = 0): group q tries the shared form iff lambda_q <= kShareLambdaMax.  LiDAR-length steps keep both
    groups, camera-length steps keep group 0 and drop group 1 -- at every T of the cases below, the sets keep their step."""
    bound = _consts()[0]
    scales = _grid_scales(_coverage_sets())
    thr = _lambda_max()
    for T in (7, 16, 48, 100, 128, 768):
        _, d, near, far = _ray_set("b", 16, T, scales)
        lam = _lambda(d, near, far, T, bound, scales)
        assert (lam[0] <= thr).all() and (lam[1] <= thr).all(), (T, lam)
        _, d, near, far = _ray_set("c", 16, T, scales)
        lam = _lambda(d, near, far, T, bound, scales)
        assert (lam[0] <= thr).all() and (lam[1] > thr).all(), (T, lam)


@pytest.mark.parametrize("level_kinds", ["compiled", "runtime"])
@pytest.mark.parametrize("grid", ["config2", "small_hash"])
@pytest.mark.parametrize("lidar", [True, False])
@pytest.mark.parametrize("N,T,noise", SHAPES)
def test_shared_corner_gathers_are_bit_identical_to_the_per_lane_form(dev, field, variants, N, T, noise, lidar, grid, level_kinds):
    from nvsf import field_ops as ops
    m, small, small_table = field
    enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
    spec, table = (enc.spec, enc.table_f16()) if grid == "config2" else (small, small_table)
    o, d, near, far = (_t(a, dev) for a in _batch(N, T, _grid_scales(spec)))
    nz = torch.rand(N, T, generator=torch.Generator().manual_seed(N * T)).to(dev) if noise else None
    heads = (m.raydrop_net.weights_f16(), m.intensity_net.weights_f16()) if lidar else (m.color_net.weights_f16(), None)
    bg = None if lidar else [1.0, 0.5, 0.25]
    args = (o, d, near, far, T, m._aabb_host, float(m.bound), table, spec, m.sigma_net.weights_f16(), lidar, heads[0], heads[1], m._k_scale(), bg, nz)
    targs = (o, d, near, far, T, m._aabb_host, float(m.bound), nz, table, spec, m.sigma_net.weights_f16(), lidar, heads[0], heads[1], m._k_scale(), bg,
             ops.W_THRESH, False)
    variants.set(level_kinds=level_kinds)
    res = {}
    for form in ("never", "gated", "always"):
        variants.set(corner_share=form)
        res[form] = tuple(ops.render_uniform(*args, sliced=False)) + tuple(ops.render_uniform_train_forward(*targs))
    variants.clear("corner_share")
    variants.clear("level_kinds")
    assert len(res["never"]) == 15
    for form in ("gated", "always"):
        for k, (a, b) in enumerate(zip(res[form], res["never"])):
            assert torch.equal(a, b), (form, k)
    assert float(res["never"][1].abs().max()) > 0.0  # the render is not empty


@pytest.mark.parametrize("grid", ["config2", "small_hash"])
@pytest.mark.parametrize("lidar", [True, False])
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("T", OVERSHOOT_T)
def test_shared_corner_gathers_on_the_faces_of_the_box(dev, field, variants, T, noise, lidar, grid):
    """Rays that overshoot the box (test_density_sliced_gpu._overshoot_rays): the clamped tail of a ray is whole tiles in ONE cell on a
    face, an edge or a corner of the box, where the dense levels' index wraps and the shared form gathers one corner per lane.  The three
    forms agree bit for bit; config2 runs the instance with the level kinds compiled in, small_hash the run-time one with a mixed group."""
    from nvsf import field_ops as ops
    m, small, small_table = field
    enc = m.hash_encoder_lidar if lidar else m.hash_encoder_camera
    spec, table = (enc.spec, enc.table_f16()) if grid == "config2" else (small, small_table)
    (o, d, near, far), nz, _ = _overshoot_batch(float(m.bound), dev, T, noise)
    heads = (m.raydrop_net.weights_f16(), m.intensity_net.weights_f16()) if lidar else (m.color_net.weights_f16(), None)
    bg = None if lidar else [1.0, 0.5, 0.25]
    args = (o, d, near, far, T, m._aabb_host, float(m.bound), table, spec, m.sigma_net.weights_f16(), lidar, heads[0], heads[1], m._k_scale(), bg, nz)
    res = {}
    for form in ("never", "gated", "always"):
        variants.set(corner_share=form)
        res[form] = tuple(ops.render_uniform(*args, sliced=False))
    variants.clear("corner_share")
    assert len(res["never"]) == 5
    for form in ("gated", "always"):
        for k, (a, b) in enumerate(zip(res[form], res["never"])):
            assert torch.equal(a, b), (form, k)
    assert float(res["never"][1].abs().max()) > 0.0  # the render is not empty
