"""TEST INFRASTRUCTURE -- differentiable float64 restatements of the three space-time encoders, operator by operator.

The K-planes (csrc/planes.hip: PlanesFn, PlanesMultiFn), the time-sliced 2-D hash grids (csrc/hashgrid4d.hip: HashGrid4D's dynamic half,
HashDynFn / HashDyn3Fn) and the flow field's 3-D grid with Lagrange reduction (k_hash3d_lagrange, FlowGridFn) written as plain torch
algebra.  Every function runs on the device of its inputs (the CPU included) and is linear in its table, so autograd's gradient is an
independent high-precision statement of what the HIP backward kernels compute.  The rules are those of tests/torch_f64_static.py:

  * whatever decides a cell index, a fraction, an interpolation weight or a border clamp is computed in fp32, operation by operation
    as the kernel computes it, and then promoted: the K-planes' `u` of make_axis (planes.hip), its clamp, its floor and the two cells
    per axis; the hash grids' pos = fmaf(scale, x, 0.5), cell, frac and corner weights (hashgrid_device.h) and the uint32 index
    arithmetic of grid_row (the stride walk decides dense / hashed); a flow-warped position x + flow is an fp32 sum;
  * the K-planes' two linear weights per axis are u - floor(u) and 1 - (u - floor(u)) of the PROMOTED u; the derivative with respect
    to a coordinate is attached to that u as a straight-through term: R - 1 inside the image, 0 where u <= 0 or u >= R - 1 (torch's
    border rule, the kernel's Axis::grad) -- exactly the piecewise-linear function the kernel differentiates, on the kernel's cell;
  * the fp16 roundings of the forward are applied (tables, slice features, grid features; regime 1 rounds every product and sum),
    their gradient passes straight through; the DIRECTION of a grid feature's rounding is taken from the kernels' fp32 corner chain
    (grid_features, rounding="chain32"; "sum" rounds the float64 sum itself, as tests/torch_f64_static.py does);
  * everything that is summed or multiplied afterwards is `dtype` = float64.  With dtype = float32 the same functions are the
    BASELINE of tests/test_dynamic_f64_gpu.py: torch's own elementwise kernels, gathers by index_select (whose backward is index_add_);
  * the only values taken from the product are host constants it passes to its kernels: hash_field.lagrange_weights_host and the two
    blend factors formed in np.float32 (time_constants).  Nothing a kernel produced is read.

`abs_sum=True` evaluates the same expression with the absolute value of every addend (|table|, |time weight|, and the K-planes'
lower linear weight differentiated with the sign of the upper one): fed with |incoming gradient| its autograd gradient is, per entry,
the sum of the |addend| that make the entry up -- the unit the error bars are stated in.

`handover=True` (hash grids) restates the operator CHAIN forms (testing.variant(hash4d_train="slices"), FlowField.grid_train_mode =
"chain"): there the feature gradient reaches the encoder's backward as an fp16 tensor (the encoders return fp16, autograd casts the
gradient of `.float()` / of a mixed-type product back), formed as half(fp32 product of the incoming fp32 gradient and the fp32 time
factors in the chain's order).  That rounding is part of what those forms compute; it is applied here as they apply it.
"""
import math

import numpy as np
import torch

from torch_f64_static import _F16, f16  # noqa: F401  (re-exported: the fp16 rounding with a straight-through gradient)

_PRIMES = (1, 2654435761, 805459861)
_U32 = 0xFFFFFFFF
PLANE_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
_GROUPS = ((0, 1, 3), (2, 4, 5))  # static planes xy xz yz | time planes xt yt zt
HASH_PAIRS = ((0, 1), (0, 2), (1, 2))
C = 8


class _Through(torch.autograd.Function):
    """Forward: any map of the values (abs); backward: straight through -- the gradient is taken with respect to the mapped values."""

    @staticmethod
    def forward(ctx, x):
        return x.abs()

    @staticmethod
    def backward(ctx, g):
        return g


class _HandOver(torch.autograd.Function):
    """value * prod(factors); backward: half(((g * f_0)_fp32 * f_1)_fp32 ...) -- the fp16 gradient hand-over of the operator chains."""

    @staticmethod
    def forward(ctx, x, factors):
        ctx.factors = factors
        return x * math.prod(factors)

    @staticmethod
    def backward(ctx, g):
        h = g.float()
        for f in ctx.factors:
            h = h * float(f)
        return h.half().to(g.dtype), None


# ------------------------------------------------------------------------------------------------------------------------------------
# K-planes
# ------------------------------------------------------------------------------------------------------------------------------------
def plane_layout(res_host):
    """[(scale, pair, float offset, H, W)] of the channel-last parameter: per scale the six pairs (a, b), each [res_b][res_a][8]."""
    out, off = [], 0
    for s in range(len(res_host) // 4):
        r = res_host[4 * s:4 * s + 4]
        for q, (a, b) in enumerate(PLANE_PAIRS):
            out.append((s, q, off, int(r[b]), int(r[a])))
            off += int(r[a]) * int(r[b]) * C
    return out


def _axis(p32, R):
    """make_axis in fp32: the clamped u, its two cells (int64) and `inside` (the coordinate gradient is R - 1 there, 0 elsewhere)."""
    u = ((p32 * 2.0 - 1.0 + 1.0) / 2.0) * float(R - 1)
    inside = ~((u <= 0.0) | (u >= float(R - 1)))
    u = torch.clamp(u, min=0.0, max=float(R - 1))  # fminf(R - 1, fmaxf(u, 0))
    f0 = torch.floor(u)
    c0 = f0.to(torch.int64)
    c1 = torch.clamp(c0 + 1, max=R - 1)
    return u, f0, c0, c1, inside


def _axis_weights(p32, carrier, R, dtype, abs_sum):
    """(c0, c1, w0, w1) of one axis: the cells in fp32, the weights in `dtype` from the promoted u, d u / d p attached through `carrier`
    (a `dtype` tensor equal to the position whose gradient is wanted, or None)."""
    u, f0, c0, c1, inside = _axis(p32, R)
    up = u.to(dtype)
    if carrier is not None:
        up = up + float(R - 1) * inside.to(dtype) * (carrier - carrier.detach())
    w1 = up - f0.to(dtype)
    w0 = 1.0 - w1
    if abs_sum:  # |d w0 / d u| = +1
        w0 = w0.detach() + (w1 - w1.detach())
    return c0, c1, w0, w1


def _plane_group(pos32, carriers, planes, res_host, grp, dtype, abs_sum):
    """Features [M, S 8] of one group of three planes at pos32 [M, 4] fp32: per scale (p0 * p1) * p2 of the bilinear values."""
    layout = plane_layout(res_host)
    out = []
    for s in range(len(res_host) // 4):
        r = res_host[4 * s:4 * s + 4]
        ax = [_axis_weights(pos32[:, d], None if carriers is None else carriers[d], int(r[d]), dtype, abs_sum) for d in range(4)]
        f = None
        for q in _GROUPS[grp]:
            a, b = PLANE_PAIRS[q]
            _, _, off, H, W = layout[6 * s + q]
            tex = planes[off:off + H * W * C].view(H * W, C)
            v = None
            for cb, wb in ((ax[b][0], ax[b][2]), (ax[b][1], ax[b][3])):
                for ca, wa in ((ax[a][0], ax[a][2]), (ax[a][1], ax[a][3])):
                    term = (wa * wb)[:, None] * tex.index_select(0, cb * W + ca)
                    v = term if v is None else v + term
            f = v if f is None else f * v
        out.append(f)
    return torch.cat(out, -1)


def planes_features(xt, planes, res_host, want, dtype=torch.float64, abs_sum=False, xt_leaf=None):
    """PlanesFn: xt [M, 4] fp32, planes: the channel-last parameter as a `dtype` leaf -> (static, dynamic) [M, S 8] (None for a group
    `want` leaves out: bit 0 static, bit 1 dynamic).  xt_leaf: a `dtype` leaf of xt's shape that receives the coordinate gradient (only
    its gradient is used: the cells and weights come from xt)."""
    P = _Through.apply(planes) if abs_sum else planes
    pos = xt.detach().float()
    car = None if xt_leaf is None else [xt_leaf[:, d] for d in range(4)]
    return tuple(_plane_group(pos, car, P, res_host, g, dtype, abs_sum) if want & (1 << g) else None for g in (0, 1))


def multi_positions(x, flow, t0, t1, t2, blend):
    """The evaluations of PlanesMultiFn as [(group, pos32 [M, 4], flow column or None)]: static and dynamic at (x, t0), dynamic at
    (x + flow[:, :3], t1) and (x + flow[:, 3:6], t2), the sums in fp32.  An absent neighbour (time None) is left out, or -- blend --
    is the base evaluation (the multi node's rule)."""
    x = x.detach().float()

    def at(p, t):
        return torch.cat([p[:, :3], torch.full_like(p[:, :1], float(np.float32(t)))], -1)
    evals = [(0, at(x, t0), None), (1, at(x, t0), None)]
    for tn, col in ((t1, 0), (t2, 3)):
        if tn is not None:
            evals.append((1, at(x[:, :3] + flow.detach().float()[:, col:col + 3], tn), col))
        elif blend:
            evals.append((1, at(x, t0), None))
        else:
            evals.append(None)
    return evals


def planes_multi_features(x, flow, planes, res_host, t0, t1, t2, blend=False, dtype=torch.float64, abs_sum=False,
                          flow_leaf=None):
    """PlanesMultiFn: x [M, >= 3] fp32, flow [M, >= 6] fp32 or None -> (static, d, d1, d2) with None for an absent neighbour, or --
    blend -- (static, 0.5 d + 0.25 (d1 + d2)).  flow_leaf: a `dtype` leaf [M, 6] that receives the flow gradient (as xt_leaf above)."""
    P = _Through.apply(planes) if abs_sum else planes
    outs = []
    for ev in multi_positions(x, flow, t0, t1, t2, blend):
        if ev is None:
            outs.append(None)
            continue
        grp, pos, col = ev
        car = None
        if col is not None and flow_leaf is not None:
            car = [flow_leaf[:, col + d] for d in range(3)] + [None]
        outs.append(_plane_group(pos, car, P, res_host, grp, dtype, abs_sum))
    if not blend:
        return tuple(outs)
    return outs[0], 0.5 * outs[1] + 0.25 * (outs[2] + outs[3])


def touched_texels(evals, res_host):
    """bool over the channel-last parameter: the texel entries some tap of some evaluation [(group, pos32 [M, 4])] reads, whatever its
    weight -- all others must receive no gradient."""
    layout = plane_layout(res_host)
    total = layout[-1][2] + layout[-1][3] * layout[-1][4] * C
    dev = evals[0][1].device
    hit = torch.zeros(total // C, dtype=torch.bool, device=dev)
    for grp, pos in evals:
        for s in range(len(res_host) // 4):
            r = res_host[4 * s:4 * s + 4]
            cells = [_axis(pos[:, d], int(r[d]))[2:4] for d in range(4)]
            for q in _GROUPS[grp]:
                a, b = PLANE_PAIRS[q]
                _, _, off, H, W = layout[6 * s + q]
                for cb in cells[b]:
                    for ca in cells[a]:
                        hit[off // C + cb * W + ca] = True
    return hit.repeat_interleave(C)


def clamped_axes(pos32, res_host):
    """bool [M, 3]: the spatial axes whose coordinate is clamped (u <= 0 or u >= R - 1) at EVERY scale: no gradient passes there."""
    out = torch.ones(pos32.shape[0], 3, dtype=torch.bool, device=pos32.device)
    for s in range(len(res_host) // 4):
        for d in range(3):
            out[:, d] &= ~_axis(pos32[:, d], int(res_host[4 * s + d]))[4]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# hash grids (D = 2 with a column pair, D = 3)
# ------------------------------------------------------------------------------------------------------------------------------------
def _grid_row(cc, res, hsize):
    """grid_row of hashgrid_device.h on uint32 values held in int64: the stride walk decides dense / hashed."""
    stride, index, dense = 1, torch.zeros_like(cc[0]), True
    for c in cc:
        if stride <= hsize:
            index = (index + ((c * (stride & _U32)) & _U32)) & _U32
            stride *= res
        else:
            dense = False
    if not dense or hsize < stride:
        index = torch.zeros_like(cc[0])
        for c, p in zip(cc, _PRIMES):
            index = index ^ ((c * p) & _U32)
    return index % hsize


def _corners(x32, spec, cols):
    """(level, table row offset, rows [M] int64, weight [M] fp32) of every corner of every level of the columns `cols` of x32 (fp32), as
    grid_cell / encode_level form them: pos = fmaf(scale, x, 0.5), corner c takes frac where bit d of c is set, weights multiplied in
    axis order starting from 1."""
    D = len(cols)
    xs = x32[:, list(cols)]
    for l in range(spec.L):
        scale = float(np.float32(spec.scales[l]))
        res, off = int(spec.res[l]), int(spec.offsets[l])
        hsize = int(spec.offsets[l + 1]) - off
        pos = (xs.double() * scale + 0.5).float()  # the fp64 product of two fp32 values is exact, + 0.5 too: one rounding, as fmaf
        cell = torch.floor(pos)
        frac = pos - cell
        c = cell.to(torch.int32).to(torch.int64) & _U32  # (uint32_t)(int32_t)floor
        for k in range(1 << D):
            b = [(k >> d) & 1 for d in range(D)]
            cc = [(c[:, d] + b[d]) & _U32 for d in range(D)]
            w = torch.ones_like(frac[:, 0])
            for d in range(D):
                w = w * (frac[:, d] if b[d] else 1.0 - frac[:, d])
            yield l, off, _grid_row(cc, res, hsize), w


def grid_features(x32, table, spec, cols, dtype=torch.float64, abs_sum=False, rounding="chain32"):
    """One grid lookup: x32 fp32 -> [M, L, F] `dtype`, the fp16-rounded sum over corners of weight * fp16(table); table: `dtype` leaf.
    The sum that carries the gradient is a `dtype` sum.  rounding: what the fp16 rounding of the value is applied to --
      "sum":     that `dtype` sum (the rule of tests/torch_f64_static.py);
      "chain32": the fp32 chain acc = fmaf(w_c, v_c, acc) over the corners in encode_level's order, which is what the kernels round.
                 A float64 sum that lies within the chain's fp32 error of an fp16 rounding boundary rounds the other way (measured on
                 the CPU fixtures: 7 of 72 000 regime-0 features, 16 of 172 800 slice features against the CPU oracle), a whole fp16
                 ulp = up to 2^13 units of 2^-24 where the sums are compared; the direction of an fp16 rounding is a decision of the
                 kernel like a cell index, so it is taken in fp32 as the kernel takes it, and no row has to be set aside."""
    tab = f16(table).view(-1, spec.F)
    if abs_sum:
        tab = _Through.apply(tab)
    acc = [None] * spec.L
    chain = [None] * spec.L
    for l, off, idx, w in _corners(x32, spec, cols):
        v = tab.index_select(0, off + idx)
        term = w.to(dtype)[:, None] * v
        acc[l] = term if acc[l] is None else acc[l] + term
        if rounding == "chain32":
            with torch.no_grad():  # the product of an fp32 and an fp16 value is exact in fp64, and so is the sum short of 2^-29 cases
                prev = 0.0 if chain[l] is None else chain[l].double()
                chain[l] = (w.double()[:, None] * v.double() + prev).float()
    out = torch.stack(acc, 1)
    if rounding == "chain32":
        rounded = torch.stack(chain, 1).half().to(dtype)
        return out + (rounded - out).detach()  # the chain's value, the sum's (straight-through) gradient
    return f16(out)


def touched_entries(x32, spec, cols):
    """bool [n_rows F]: the table entries some corner of x32 reads (whatever its weight)."""
    hit = torch.zeros(spec.n_rows, dtype=torch.bool, device=x32.device)
    for _, off, idx, _ in _corners(x32, spec, cols):
        hit[off + idx] = True
    return hit.repeat_interleave(spec.F)


def time_constants(t_host, time_resolution, reciprocal_division):
    """The host constants HashGrid4D hands to its kernels: (k1, k2, blend_lo, blend_hi, lag[4])."""
    from nvsf.nerf.models.hash_field import lagrange_weights_host
    idx = np.float32(t_host) * np.float32(time_resolution - 1)
    k1, k2 = int(math.floor(idx)), int(math.ceil(idx))
    return k1, k2, float(np.float32(k2) - idx), float(idx - np.float32(k1)), lagrange_weights_host(t_host, 4, reciprocal_division)


def _slice_features(x32, tables, specs, k, dtype, abs_sum, rounding="chain32"):
    return [grid_features(x32, tables[pl][k], specs[pl], HASH_PAIRS[pl], dtype, abs_sum, rounding) for pl in range(3)]  # 3 x [M, 8, 4]


def hash_time_features(x32, tables, specs, time_resolution, t_host, reciprocal_division=True, dtype=torch.float64, abs_sum=False,
                       handover=False, rounding="chain32"):
    """Regime 0 of HashGrid4D's dynamic half: x32 [M, 3] fp32, tables[pair][slice]: `dtype` leaves -> [M, 24] = per pair and level
    sum_i lag_i (blend_lo f_lo[i] + blend_hi f_hi[i]); no blend when floor == ceil."""
    k1, k2, b_lo, b_hi, lag = time_constants(t_host, time_resolution, reciprocal_division)
    if abs_sum:
        b_lo, b_hi, lag = abs(b_lo), abs(b_hi), [abs(v) for v in lag]
    lo = _slice_features(x32, tables, specs, k1, dtype, abs_sum, rounding)
    hi = _slice_features(x32, tables, specs, k2, dtype, abs_sum, rounding) if k1 != k2 else None
    out = []
    for pl in range(3):
        acc = None
        for i in range(4):
            if handover and not abs_sum:
                feat = _HandOver.apply(lo[pl][:, :, i], (lag[i],) if hi is None else (lag[i], b_lo))
                if hi is not None:
                    feat = feat + _HandOver.apply(hi[pl][:, :, i], (lag[i], b_hi))
            else:
                feat = lo[pl][:, :, i] if hi is None else b_lo * lo[pl][:, :, i] + b_hi * hi[pl][:, :, i]
                feat = lag[i] * feat
            acc = feat if acc is None else acc + feat
        out.append(acc)
    return torch.cat(out, -1)


def hash_time_features_f16(x32, tables, specs, time_resolution, t_host, reciprocal_division=False, dtype=torch.float64, abs_sum=False,
                           rounding="chain32"):
    """Regime 1 (a 0-dim t: the flow-warped neighbour frames), forward only: the blend and the reduction round every product and every
    sum to fp16, (a.float() * b.float()).half() and so on -> [M, 24] fp16.  abs_sum: the same sums of absolute values, unrounded.
    Behind the slice features every operation here is fp32 -> fp16 whatever `dtype` is: a float32 evaluation is the same computation."""
    k1, k2, b_lo, b_hi, lag = time_constants(t_host, time_resolution, reciprocal_division)
    with torch.no_grad():
        lo = _slice_features(x32, tables, specs, k1, dtype, abs_sum, rounding)
        hi = _slice_features(x32, tables, specs, k2, dtype, abs_sum, rounding) if k1 != k2 else None
        out = []
        for pl in range(3):
            acc = None
            for i in range(4):
                if abs_sum:
                    feat = lo[pl][:, :, i] if hi is None else abs(b_lo) * lo[pl][:, :, i] + abs(b_hi) * hi[pl][:, :, i]
                    term = abs(lag[i]) * feat
                    acc = term if acc is None else acc + term
                    continue
                f_lo = lo[pl][:, :, i].float()  # fp16 values
                if hi is None:
                    feat = f_lo
                else:
                    feat = ((f_lo * b_lo).half().float() + (hi[pl][:, :, i].float() * b_hi).half().float()).half().float()
                term = (feat * lag[i]).half().float()
                acc = term if acc is None else (acc + term).half().float()
            out.append(acc)
        res = torch.cat(out, -1)
        return res if abs_sum else res.half()


def flow_grid_features(x32, table, spec, t_host, reciprocal_division=True, dtype=torch.float64, abs_sum=False, handover=False,
                       rounding="chain32"):
    """The flow field's front end: 3-D grid (F = 8), features rounded to fp16, reduced[:, 2 l + e] = sum_i w_i f[l, 2 i + e] -> [M, 2 L]."""
    from nvsf.nerf.models.hash_field import lagrange_weights_host
    w = lagrange_weights_host(t_host, 4, reciprocal_division)
    if abs_sum:
        w = [abs(v) for v in w]
    f = grid_features(x32[:, :3], table, spec, (0, 1, 2), dtype, abs_sum, rounding).view(x32.shape[0], spec.L, 4, 2)
    acc = None
    for i in range(4):
        term = _HandOver.apply(f[:, :, i, :], (w[i],)) if handover and not abs_sum else w[i] * f[:, :, i, :]
        acc = term if acc is None else acc + term
    return acc.reshape(x32.shape[0], 2 * spec.L)
