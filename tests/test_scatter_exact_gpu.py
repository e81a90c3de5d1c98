"""The table / texel scatters on inputs whose sums do not depend on the order of the additions.

fp32 atomics arrive in another order every run, so the other tests compare two formulations of a scatter with a tolerance and cannot
show that a scatter is UNCHANGED.  Here every addend is a non-negative multiple of 2^-u and every per-entry sum stays below 2^(24-u):
any order of fp32 additions, the fp64 LDS images and the 2^(33-e) fixed-point image of the binned scatter are then all exact, and every
formulation of an operator must be `torch.equal` to every other and to an fp64 sum formed on the CPU.  The CPU side asserts both
properties of the inputs (ExactSum) before anything is compared, so a wrong choice of inputs fails there and not as noise on the GPU.
These tests pin the ADDITION; the addends -- bilinear and corner weights, blend factors, Lagrange weights, the product rule -- are pinned
against float64 restatements on generic inputs in tests/test_dynamic_f64_gpu.py (space-time encoders) and tests/test_static_grad_f64_gpu.py.

  grids   per_level_scale = 2 and an integer base resolution: every scale_l is an integer; positions are multiples of 1/8 in [0, 1] and
          gradients integers 0..3, so the weights are multiples of 2^-9 (3-D) / 2^-6 (2-D);
  planes  resolutions 2^a + 1, positions on a 1/16 lattice, texels in {0, 1}, gradients 0 or 1.  The coarsest scale (res 3) gives
          eighths per axis: interpolated values in units of 2^-6, addends g (v v) w in units of 2^-18 (2^-20 behind the blend's 1/4),
          which leaves room for few addends per texel: ~100 rows carry a gradient, in bursts of 3-5 consecutive rows inside one
          texel quad of the coarse scales, some of them across rows 32 k, 128 k (staging round, item) and a slice of the time kernel.
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from planes_calls import multi_bwd_call

pytestmark = pytest.mark.gpu

M_SMALL = 1003
M_LARGE = (1 << 16) + 77  # the production forms (LDS images) start at 2^16 rows
_M32 = np.uint64(0xFFFFFFFF)


class ExactSum:
    """fp64 scatter-add on the CPU that checks what makes the GPU sums order-independent: every addend a non-negative multiple of
    2^-u, every per-entry sum below 2^(24-u)."""

    def __init__(self, n, u):
        self.sum, self.u = np.zeros(n, np.float64), u

    def add(self, idx, val):
        idx, val = np.broadcast_arrays(np.asarray(idx, np.int64), np.asarray(val, np.float64))
        scaled = val * 2.0 ** self.u
        assert (val >= 0).all() and np.array_equal(scaled, np.round(scaled)), f"an addend is no non-negative multiple of 2^-{self.u}"
        np.add.at(self.sum, idx.ravel(), val.ravel())

    def result(self):
        assert self.sum.max() > 0 and self.sum.max() < 2.0 ** (24 - self.u), f"a per-entry sum reaches 2^{24 - self.u}: {self.sum.max()}"
        return torch.from_numpy(self.sum.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# hash grids
# ---------------------------------------------------------------------------------------------------------------------------------
def _grid_rows(cc, res, hsize):
    """grid_row<D> of csrc/hashgrid_device.h on uint32 cell coordinates [N, D]."""
    D = cc.shape[1]
    stride, dense = 1, True
    index = np.zeros(len(cc), np.uint64)
    for d in range(D):
        if stride <= hsize:
            index = (index + cc[:, d].astype(np.uint64) * np.uint64(stride)) & _M32
            stride *= res
        else:
            dense = False
    if not dense or hsize < stride:
        index = np.zeros(len(cc), np.uint64)
        for d, prime in zip(range(D), (1, 2654435761, 805459861)):
            index ^= (cc[:, d].astype(np.uint64) * np.uint64(prime)) & _M32
    return (index & np.uint64(hsize - 1) if hsize & (hsize - 1) == 0 else index % np.uint64(hsize)).astype(np.int64)


def _level_corners(x, spec, l):
    """[(rows, weights)] of the 2^D corners of level l for positions x (fp64 [N, D])."""
    scale = float(spec.scales[l])
    assert scale == round(scale), "per_level_scale = 2 and an integer base resolution make every scale an integer"
    row0, hsize = int(spec.offsets[l]), int(spec.offsets[l + 1] - spec.offsets[l])
    pos = scale * x + 0.5
    fl = np.floor(pos)
    frac, cell = pos - fl, fl.astype(np.int64)
    out = []
    for c in range(1 << spec.D):
        bits = np.array([(c >> d) & 1 for d in range(spec.D)])
        w = np.prod(np.where(bits == 1, frac, 1.0 - frac), axis=1)
        out.append((row0 + _grid_rows(cell + bits, int(spec.res[l]), hsize), w))
    return out


def _lattice8(rng, M, D=3):
    """Positions k / 8 in [0, 1], both ends included."""
    x = rng.integers(0, 9, size=(M, D)).astype(np.float64) / 8.0
    x[0], x[1] = 0.0, 1.0
    return x


@functools.lru_cache(maxsize=None)
def _grid3d_case(F):
    """D = 3, L = 4: levels 0, 1 dense (4^3, 8^3 cells), levels 2, 3 hashed into 2^11 rows; M = 1003 rows, every one with a gradient."""
    from nvsf import field_ops as ops
    spec = ops.GridSpec(3, 4, F, 11, 4, 2.0)
    rows = [int(b - a) for a, b in zip(spec.offsets[:-1], spec.offsets[1:])]
    assert [int(r) ** 3 > n for r, n in zip(spec.res, rows)] == [False, False, True, True]
    rng = np.random.default_rng(100 + F)
    x = _lattice8(rng, M_SMALL)
    g = rng.integers(0, 4, size=(M_SMALL, spec.L * F)).astype(np.float64)
    ref = ExactSum(spec.n_rows * F, 9)
    for l in range(spec.L):
        for rows_c, w in _level_corners(x, spec, l):
            ref.add(rows_c[:, None] * F + np.arange(F), w[:, None] * g[:, l * F:(l + 1) * F])
    return spec, x.astype(np.float32), g.astype(np.float32), ref.result()


@pytest.mark.parametrize("f16", [False, True], ids=["g32", "g16"])
@pytest.mark.parametrize("F", [2, 4])
def test_hashgrid_backward_every_form_is_the_exact_sum(dev, variants, F, f16):
    """hashgrid_backward: one thread per (row, level), corner-parallel run merging, and the binned entry with the run-sum / per-row
    split at (2, 4) and (2, 3), from rows and from the level-major gradient: all the fp64 sum."""
    from nvsf import _hip, field_ops as ops
    spec, x_np, g_np, ref = _grid3d_case(F)
    x = torch.from_numpy(x_np).to(dev)
    g = torch.from_numpy(g_np).to(dev)
    g = g.half() if f16 else g
    g_lm = g.view(M_SMALL, spec.L, F).permute(1, 0, 2).contiguous()
    got = {"corners": ops.hashgrid_backward(x, [0, 1, 2], spec, g)}
    variants.set(hashgrid_bwd="atomic")
    got["atomic"] = ops.hashgrid_backward(x, [0, 1, 2], spec, g)
    variants.clear("hashgrid_bwd")
    for plan in ((2, 4), (2, 3)):
        assert _hip.hashgrid_bwd_ws_bytes(M_SMALL, spec, *plan) > 0  # the binned entry is what runs
        got[f"binned{plan} rows"] = ops.hashgrid_backward(x, [0, 1, 2], spec, g, fine_from=plan)
        got[f"binned{plan} level-major"] = ops.hashgrid_backward(x, [0, 1, 2], spec, g_lm, fine_from=plan)
    torch.cuda.synchronize()
    for name, t in got.items():
        assert torch.equal(t.cpu(), ref), name


# ---- the space-time grids (three time-sliced 2-D grids, 8 levels x 4 features) ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid4d_case():
    """Pairs (x,y), (x,z), (y,z): 2-D grids 4 -> 512 of 2^15 / 2^13 / 2^13 rows (the level sizes of the reference's dynamic hash: two
    workgroups per slice of the LDS form for pair 0, one for the others).  The scalar sums G[pair][row] of M = 1003 rows."""
    from nvsf import field_ops as ops
    specs = [ops.GridSpec(2, 8, 4, log2, 4, 2.0) for log2 in (15, 13, 13)]
    rng = np.random.default_rng(7)
    x = _lattice8(rng, M_SMALL)
    g = rng.integers(0, 4, size=(M_SMALL, 24)).astype(np.float64)
    sums = []
    for p, (spec, (a, b)) in enumerate(zip(specs, ((0, 1), (0, 2), (1, 2)))):
        ref = ExactSum(spec.n_rows, 6)
        for l in range(8):
            for rows_c, w in _level_corners(x[:, [a, b]], spec, l):
                ref.add(rows_c, w * g[:, p * 8 + l])
        sums.append(ref.result())
    pad = _lattice8(rng, M_LARGE - M_SMALL)  # rows without a gradient
    return specs, x.astype(np.float32), g.astype(np.float32), sums, pad.astype(np.float32)


def _grid4d_host(specs):
    from nvsf import _hip
    return (_hip.host_f32([v for s in specs for v in s.scales]), _hip.host_u32([v for s in specs for v in s.res]),
            _hip.host_u32([v for s in specs for v in s.offsets]))


def _grid4d_sums(dev, entry, x, g, specs):
    from nvsf import _hip
    sums = [torch.zeros(s.n_rows, dtype=torch.float32, device=dev) for s in specs]
    _hip.call(entry, _hip.ptr(x), 3, x.shape[0], *_grid4d_host(specs), _hip.ptr(g), (ctypes.c_void_p * 3)(*[t.data_ptr() for t in sums]))
    torch.cuda.synchronize()
    return [t.cpu() for t in sums]


def test_hash4d_scalar_sums_run_merging_is_the_exact_sum(dev, variants):
    specs, x_np, g_np, ref, _ = _grid4d_case()
    variants.set(hash4d_bwd="runs")
    got = _grid4d_sums(dev, "nvsf_hashgrid4d_dynamic_bwd_scalar", torch.from_numpy(x_np).to(dev), torch.from_numpy(g_np).to(dev), specs)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("col_major", [False, True], ids=["rows", "columns"])
def test_hash4d_scalar_sums_through_lds_are_the_exact_sum(dev, col_major):
    """The LDS form (2^16 + 77 rows: the same rows followed by rows without a gradient), fed by rows [M, 24] and by columns [24][M]."""
    specs, x_np, g_np, ref, pad = _grid4d_case()
    x = torch.from_numpy(np.concatenate([x_np, pad])).to(dev)
    g = torch.zeros(M_LARGE, 24, device=dev)
    g[:M_SMALL] = torch.from_numpy(g_np).to(dev)
    if col_major:
        got = _grid4d_sums(dev, "nvsf_hashgrid4d_dynamic_bwd_scalar_t", x, g.t().contiguous(), specs)
    else:
        got = _grid4d_sums(dev, "nvsf_hashgrid4d_dynamic_bwd_scalar", x, g, specs)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


TIME_BLEND, TIME_LAG = (0.25, 0.75), (1.0, 2.0, 0.5, 1.0)  # dyadic: addends w g lag blend are multiples of 2^-6 * 2^-1 * 2^-2 = 2^-9


@functools.lru_cache(maxsize=None)
def _grid4d_slice_reference(same_slice):
    """Per pair the gradients of the (lo, hi) slice tables [rows, 4]: the addends w_c g lag_i blend themselves through ExactSum(2^-9), and
    on the CPU already equal to the expansion lag_i * blend * G[row] of the scalar sums."""
    specs, x_np, g_np, sums, _ = _grid4d_case()
    x, g = x_np.astype(np.float64), g_np.astype(np.float64)
    lag, out = np.array(TIME_LAG), []
    for p, (spec, (a, b)) in enumerate(zip(specs, ((0, 1), (0, 2), (1, 2)))):
        pair = []
        for blend in ((1.0,) if same_slice else TIME_BLEND):
            ref = ExactSum(spec.n_rows * 4, 9)
            for l in range(8):
                for rows_c, w in _level_corners(x[:, [a, b]], spec, l):
                    ref.add(rows_c[:, None] * 4 + np.arange(4), (w * g[:, p * 8 + l])[:, None] * (lag * blend))
            pair.append(ref.result().view(-1, 4))
            assert torch.equal(pair[-1], sums[p][:, None] * torch.tensor(TIME_LAG) * blend)
        out.append(pair if len(pair) == 2 else [pair[0], torch.zeros_like(pair[0])])  # same slice: the hi tables are not touched
    return out


@pytest.mark.parametrize("same_slice", [0, 1])
def test_hash4d_slice_gradients_are_the_expanded_exact_sum(dev, same_slice):
    """nvsf_hashgrid4d_dynamic_bwd (the per-feature form: 16 lanes per item) against lag_i * blend * G[row], dyadic time weights."""
    from nvsf import _hip
    specs, x_np, g_np, _, _ = _grid4d_case()
    ref = _grid4d_slice_reference(same_slice)
    x, g = torch.from_numpy(x_np).to(dev), torch.from_numpy(g_np).to(dev)
    tables = [torch.zeros(s.n_rows, 4, dtype=torch.float32, device=dev) for s in specs for _ in range(2)]
    lo, hi = tables[0::2], tables[1::2]
    _hip.call("nvsf_hashgrid4d_dynamic_bwd", _hip.ptr(x), 3, M_SMALL, *_grid4d_host(specs), _hip.host_f32(TIME_BLEND + TIME_LAG), same_slice,
              _hip.ptr(g), (ctypes.c_void_p * 6)(*[t.data_ptr() for t in lo + hi]))
    torch.cuda.synchronize()
    for p in range(3):
        assert torch.equal(lo[p].cpu(), ref[p][0]) and torch.equal(hi[p].cpu(), ref[p][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# K-planes
# ---------------------------------------------------------------------------------------------------------------------------------
PLANE_RES = (3, 3, 3, 3, 5, 5, 5, 3, 9, 17, 9, 5, 17, 33, 17, 9)  # per scale: x, y, z, t -- all 2^a + 1
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
GROUP_PAIRS = ((0, 1, 3), (2, 4, 5))  # static | time planes


def _plane_offsets():
    off, at = [], 0
    for s in range(4):
        off.append([])
        for a, b in PAIRS:
            off[s].append(at)
            at += PLANE_RES[4 * s + a] * PLANE_RES[4 * s + b] * 8
    return off, at


def _axis(p, R):
    """One axis of make_tap (csrc/planes.hip): cell, clamped neighbour, the two weights."""
    u = np.clip(p * (R - 1), 0.0, R - 1.0)
    f0 = np.floor(u)
    c0 = f0.astype(np.int64)
    return c0, np.minimum(c0 + 1, R - 1), (f0 + 1.0) - u, u - f0


def _planes_add(acc, planes, p, g, grp):
    """The texel-gradient addends of one evaluation: positions p [N, 4], feature gradients g [N, 32] (already scaled), group grp."""
    off, _ = _plane_offsets()
    ch = np.arange(8)
    for s in range(4):
        taps, vals = [], []
        for q in GROUP_PAIRS[grp]:
            a, b = PAIRS[q]
            W = PLANE_RES[4 * s + a]
            ac0, ac1, aw0, aw1 = _axis(p[:, a], W)
            bc0, bc1, bw0, bw1 = _axis(p[:, b], PLANE_RES[4 * s + b])
            idx = [bc0 * W + ac0, bc0 * W + ac1, bc1 * W + ac0, bc1 * W + ac1]
            w = [aw0 * bw0, aw1 * bw0, aw0 * bw1, aw1 * bw1]
            taps.append((off[s][q], idx, w))
            vals.append(sum(planes[off[s][q] + i[:, None] * 8 + ch] * wk[:, None] for i, wk in zip(idx, w)))
        for j in range(3):
            gv = g[:, s * 8:(s + 1) * 8] * (vals[(j + 1) % 3] * vals[(j + 2) % 3])
            base, idx, w = taps[j]
            for i, wk in zip(idx, w):
                acc.add(base + i[:, None] * 8 + ch, gv * wk[:, None])


def _burst_rows(rng, M):
    """Positions [M, 3] on the 1/16 lattice and the rows that carry a gradient: bursts of 3-5 consecutive rows inside one cell of
    the res-5 scale, across rows 32 k / 128 k / 8192 k (staging round, item, slice of the time kernel) and at both ends."""
    x = rng.integers(0, 17, size=(M, 3)).astype(np.float64) / 16.0
    starts = [0, 30, 62, 126, 254, 510, 766, M - 4] + [int(v) for v in rng.integers(140, 1000, size=16)]
    if M > (1 << 16):
        starts += [8190, 16382, 32766, 40959, (1 << 16) - 2, M - 9] + [int(v) for v in rng.integers(1100, 1 << 16, size=4)]
    live = np.zeros(M, bool)
    for r0 in starts:
        n = int(rng.integers(3, 6))
        rows = np.arange(r0, min(r0 + n, M))
        corner = rng.integers(0, 4, size=3) / 4.0
        x[rows] = corner + rng.integers(0, 5, size=(len(rows), 3)) / 16.0  # inside [corner, corner + 1/4], 1.0 included
        live[rows] = True
    return x, live


@functools.lru_cache(maxsize=None)
def _planes_case(M):
    rng = np.random.default_rng(M)
    _, n = _plane_offsets()
    planes = rng.integers(0, 2, size=n).astype(np.float64)
    x, live = _burst_rows(rng, M)
    flow = rng.integers(-1, 2, size=(M, 6)).astype(np.float64) / 16.0
    for c in (0, 3):  # x + flow stays on the lattice inside [0, 1]
        flow[:, c:c + 3] = np.clip(x + flow[:, c:c + 3], 0.0, 1.0) - x
    g = np.zeros((M, 64))
    g[live] = rng.random((int(live.sum()), 64)) < 0.3  # 0 or 1; sparse enough for the 2^4 budget behind the blend's 1/4
    assert 60 <= int(live.sum()) <= 200
    return planes, x, flow, g, live


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


@functools.lru_cache(maxsize=None)
def _planes_bwd_reference(want):
    planes, x, _, g, live = _planes_case(M_SMALL)
    xt = np.concatenate([x, np.full((M_SMALL, 1), 0.4375)], axis=1)
    xt[live, 3] = (np.arange(int(live.sum())) % 17) / 16.0
    ref = ExactSum(len(planes), 18)
    for grp in range(2):
        if want & (1 << grp):
            _planes_add(ref, planes, xt[live], g[live, 32 * grp:32 * grp + 32], grp)
    return xt, ref.result()


@pytest.mark.parametrize("want", [1, 2, 3])
def test_planes_bwd_runs_and_atomic_are_the_exact_sum(dev, variants, want):
    from nvsf import _hip
    planes, _, _, g, _ = _planes_case(M_SMALL)
    xt_np, ref = _planes_bwd_reference(want)
    xt, cl = _dev(xt_np, dev), _dev(planes, dev)
    g_s, g_d = _dev(g[:, :32], dev), _dev(g[:, 32:], dev)
    for variant in ("runs", "atomic"):
        variants.set(planes_bwd=variant)
        gp = torch.zeros_like(cl)
        _hip.call("nvsf_planes_bwd", _hip.ptr(xt), M_SMALL, _hip.ptr(cl), 4, 8, _hip.host_u32(PLANE_RES), want, _hip.ptr(g_s) if want & 1 else None,
                  _hip.ptr(g_d) if want & 2 else None, _hip.ptr(gp), None)
        torch.cuda.synchronize()
        assert torch.equal(gp.cpu(), ref), variant


TIMES = (0.4375, 0.4375, 0.5625, 0.3125)  # static (unused), t, t + 1 frame, t - 1 frame: on the 1/16 lattice


@functools.lru_cache(maxsize=None)
def _planes_multi_reference(M):
    """Static + three time-plane evaluations (x, x + flow[:, :3], x + flow[:, 3:]) sharing the gradient, scaled 1, 1/2, 1/4, 1/4."""
    planes, x, flow, g, live = _planes_case(M)
    ref = ExactSum(len(planes), 20)
    xl, fl, gl = x[live], flow[live], g[live]
    for grp, off, t_e, scale in ((0, 0.0, TIMES[0], 1.0), (1, 0.0, TIMES[1], 0.5), (1, fl[:, 0:3], TIMES[2], 0.25), (1, fl[:, 3:6], TIMES[3], 0.25)):
        p = np.concatenate([xl + off, np.full((len(xl), 1), t_e)], axis=1)
        _planes_add(ref, planes, p, gl[:, 32 * grp:32 * grp + 32] * scale, grp)
    return ref.result()


def _planes_multi(dev, M):
    planes, x, flow, g, _ = _planes_case(M)
    enc = types.SimpleNamespace(planes_cl=_dev(planes, dev), _res_host=list(PLANE_RES))
    flow_wide = torch.zeros(M, 8, device=dev)  # rows wider than the six flow components, as the flow MLP pads them
    flow_wide[:, :6] = _dev(flow, dev)
    g_wide = torch.zeros(M, 72, device=dev)    # the gradient is a column slice of a wider matrix
    g_wide[:, :64] = _dev(g, dev)
    return multi_bwd_call(enc, _dev(x, dev), flow_wide, g_wide, list(TIMES), dev).cpu()


@pytest.mark.parametrize("variant", ["global", "atomic"])
def test_planes_multi_bwd_run_sums_are_the_exact_sum(dev, variants, variant):
    variants.set(planes_bwd=variant)
    assert torch.equal(_planes_multi(dev, M_SMALL), _planes_multi_reference(M_SMALL))


def test_planes_multi_bwd_production_form_is_the_exact_sum(dev):
    """2^16 + 77 rows: the time planes through the LDS images (fp64), the static planes as run sums."""
    assert torch.equal(_planes_multi(dev, M_LARGE), _planes_multi_reference(M_LARGE))
