"""TEST INFRASTRUCTURE -- numpy float64 statement of the coordinate gradient of the time-sliced 2-D hash grids
(nvsf_hashgrid4d_dynamic_grad_x, HashGrid4D.dynamic_grad_x).

Per coordinate pair q with axes (a, b) in ((x, y), (x, z), (y, z)) the blended, Lagrange-reduced feature of level l is linear in the
table entries, so the three pair grids are restated as three D = 2, F = 1 grids over an EFFECTIVE table
    T_eff[row] = sum_i w_i (b_lo lo[row][i] + b_hi hi[row][i])        (sum_i w_i lo[row][i] on a slice time),
formed in float64 from the values the kernel reads (pass the fp16 tables) and the host constants of hash_field.time_slot, and handed to
tests/hashgrid_gradx_oracle.py (`grad_x`, `cells`, `rows`: the kernel's fp32 cells and fracs, its uint32 index arithmetic).
`grad_x` also returns A[m, d], the sum of the absolute values of the 2 pairs x 8 levels x 4 corners x 4 features x 2 slices addends of
each output (one slice on a slice time): the same call on T_abs[row] = sum_i |w_i| (|b_lo| |lo| + |b_hi| |hi|).
`features` is the float64 function itself, for finite differences.
"""
import types

import numpy as np

import hashgrid_gradx_oracle as GX

PAIRS = ((0, 1), (0, 2), (1, 2))
L, F = 8, 4


def pair_spec(spec):
    """The D = 2, F = 1 grid with the levels of a pair grid's GridSpec (scales, res, offsets in rows)."""
    assert spec.D == 2 and spec.L == L and spec.F == F
    return types.SimpleNamespace(D=2, L=L, F=1, scales=spec.scales, res=spec.res, offsets=spec.offsets)


def effective_table(lo, hi, slot, absolute=False):
    """T_eff [rows] float64 of one pair: lo / hi = the two slices' tables [rows * 4] (hi is not read on a slice time)."""
    f = (lambda v: np.abs(v)) if absolute else (lambda v: v)
    lo = f(np.asarray(lo).astype(np.float64).reshape(-1, F))
    w = f(np.array([float(np.float32(v)) for v in slot.lag], np.float64))
    if slot.same:
        return lo @ w
    hi = f(np.asarray(hi).astype(np.float64).reshape(-1, F))
    return (f(float(np.float32(slot.b_lo))) * lo + f(float(np.float32(slot.b_hi))) * hi) @ w


def grad_x(p, tables, specs, slot, g, grad_scale=1.0, pos_dtype=np.float32):
    """p [M, 3] fp32 positions (x, or x + offset summed in fp32), tables = [lo slice of pair 0, 1, 2, hi slice of pair 0, 1, 2] (what
    HashGrid4D._slice_tables returns), specs: the three pair GridSpecs, slot: hash_field.TimeSlot, g [M, 24] (column 8 q + l)
    -> (dL/dp [M, 3] float64, A [M, 3] float64).  pos_dtype as in hashgrid_gradx_oracle.cells (float32: the kernel's cells and fracs)."""
    p = np.asarray(p, pos_dtype)
    M = p.shape[0]
    g = float(grad_scale) * np.asarray(g, np.float64).reshape(M, 3, L)
    out, A = np.zeros((M, 3)), np.zeros((M, 3))
    for q, axes in enumerate(PAIRS):
        s2 = pair_spec(specs[q])
        xy = p[:, list(axes)]
        gq = g[:, q, :, None]
        d, _ = GX.grad_x(xy, effective_table(tables[q], tables[3 + q], slot), s2, gq, pos_dtype)
        _, a = GX.grad_x(xy, effective_table(tables[q], tables[3 + q], slot, absolute=True), s2, gq, pos_dtype)
        for k, axis in enumerate(axes):
            out[:, axis] += d[:, k]
            A[:, axis] += a[:, k]
    return out, A


def features(p, tables, specs, slot, pos_dtype=np.float64):
    """The 24 features [M, 24] in float64 at the float64 positions p [M, 3] (no fp16 rounding of any intermediate)."""
    p = np.asarray(p, np.float64)
    out = []
    for q, axes in enumerate(PAIRS):
        out.append(GX.features(p[:, list(axes)], effective_table(tables[q], tables[3 + q], slot), pair_spec(specs[q]), pos_dtype)[:, :, 0])
    return np.concatenate(out, -1)


def face_margin(p, specs):
    """min over pairs, levels and axes of the distance of pos from the nearest cell face, in units of p.  [M]."""
    p = np.asarray(p, np.float64)
    m = np.full(p.shape[0], np.inf)
    for q, axes in enumerate(PAIRS):
        m = np.minimum(m, GX.face_margin(p[:, list(axes)], pair_spec(specs[q])))
    return m
