"""The distortion loss of mip-NeRF 360 (Barron et al. 2022, eq. 15) as DEFINED, in float64 on the CPU: the O(T^2) double sum, its
analytic gradient, and the input cases the CPU and GPU tests share.  No prefix sums here -- that is what is under test.

Per ray, from the fp32 inputs held as float64, with R = far - near:
    delta_i = z_{i+1} - z_i (i < T - 1), delta_{T-1} = R / T;  m_i = (z_i + delta_i / 2 - near) / R;  d_i = delta_i / R
    ray = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i
    d ray / d w_k = 2 sum_j w_j |m_k - m_j| + 2/3 w_k d_k
    loss = alpha sum_n ray_n / N;  a ray whose R is not finite or not > 0 gives 0 and a zero gradient row, and counts in N.
`alpha` is an fp32 input as well: ALPHA is 0.01 rounded to fp32, held as a Python float."""
import functools

import numpy as np
import torch

ALPHA = float(np.float32(0.01))
KINDS = ("spread", "peaked", "ties", "zeros", "degenerate")


def midpoints_and_widths(z, nears, fars):
    """z [N, T], nears, fars [N] float64 -> (m, d, ok): ok [N] marks the rays with a finite R > 0 (the others get m = d = 0)."""
    N, T = z.shape
    R = (fars - nears).reshape(N, 1)
    ok = torch.isfinite(R) & (R > 0)
    Rs = torch.where(ok, R, torch.ones_like(R))
    delta = torch.cat([z[:, 1:] - z[:, :-1], Rs / T], dim=1)
    m = (z + delta / 2 - nears.reshape(N, 1)) / Rs
    d = delta / Rs
    return torch.where(ok, m, torch.zeros_like(m)), torch.where(ok, d, torch.zeros_like(d)), ok.reshape(N)


def distortion(w, z, nears, fars, alpha, grad_loss=1.0):
    """-> (ray [N], loss, grad [N, T]) in float64: the double sum as written, rays in chunks of at most 2^22 pair terms."""
    w, z, nears, fars = (t.detach().cpu().double() for t in (w, z, nears, fars))
    N, T = w.shape
    m, d, ok = midpoints_and_widths(z, nears.reshape(-1), fars.reshape(-1))
    wk = torch.where(ok[:, None], w, torch.zeros_like(w))
    ray, grad = torch.zeros(N, dtype=torch.float64), torch.zeros(N, T, dtype=torch.float64)
    chunk = max(1, (1 << 22) // (T * T))
    for a in range(0, N, chunk):
        ws, ms, ds = wk[a:a + chunk], m[a:a + chunk], d[a:a + chunk]
        dist = (ms[:, :, None] - ms[:, None, :]).abs()                                   # |m_i - m_j|
        ray[a:a + chunk] = (ws[:, :, None] * ws[:, None, :] * dist).sum(dim=(1, 2)) + (ws * ws * ds).sum(dim=1) / 3
        grad[a:a + chunk] = 2 * (ws[:, None, :] * dist).sum(dim=2) + 2 * ws * ds / 3
    ray = torch.where(ok, ray, torch.zeros_like(ray))
    grad = torch.where(ok[:, None], grad, torch.zeros_like(grad))
    return ray, alpha * ray.sum() / N, grad_loss * alpha / N * grad


def bar(ref):
    """The issue's bound per element: one fp32 rounding of an fp64 result with a factor two of slack, plus ten times what the order of
    an fp64 sum of 768 terms <= 1 can move it."""
    return 2.0 ** -23 * ref.abs() + 1e-12


@functools.lru_cache(maxsize=None)
def case(N, T, kind):
    """-> dict of fp32 CPU inputs w, z [N, T], nears, fars [N] (computed once per case, never modified).  Every row of weights sums to at
    most 1, as a compositor's do: the absolute part of `bar` is worked out for sums of terms <= 1."""
    gen = torch.Generator().manual_seed(100003 * N + 101 * T + KINDS.index(kind))
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    nears = 0.05 + 0.2 * rnd(N)
    fars = nears + 0.5 + rnd(N)
    z = nears[:, None] + (fars - nears)[:, None] * torch.sort(0.001 + 0.99 * rnd(N, T), dim=1).values
    w = rnd(N, T)
    w = w / w.sum(dim=1, keepdim=True) * (0.2 + 0.8 * rnd(N, 1))
    if kind == "peaked":  # a Gaussian bump two samples wide among the last third of the row + 1e-6 noise: m W - M cancels
        centre = T - 1 - (rnd(N, 1) * (T / 3.0)).floor()
        i = torch.arange(T, dtype=torch.float64)[None, :]
        w = 0.15 * torch.exp(-0.5 * ((i - centre) / 2.0) ** 2) + 1e-6 * rnd(N, T)
    elif kind == "ties":  # pairs of equal depths, as merged rows have
        z[:, 1::2] = z[:, 0:T - 1:2]
    elif kind == "zeros":
        w[::3] = 0.0
    elif kind == "degenerate":
        fars[0] = nears[0]                     # far == near
        if N > 2:
            fars[2] = nears[2] - 0.25          # far < near
        if N > 4:
            fars[4] = float("inf")             # R not finite
    out = {"w": w.float(), "z": z.float(), "nears": nears.float(), "fars": fars.float()}
    if kind == "degenerate":                   # fp32 rounding must not undo far == near
        out["fars"][0] = out["nears"][0]
    assert bool((out["z"][:, 1:] >= out["z"][:, :-1]).all())
    return out


@functools.lru_cache(maxsize=None)
def reference(N, T, kind):
    """(ray, loss, grad) of `case(N, T, kind)` under ALPHA, float64; computed once and shared."""
    c = case(N, T, kind)
    return distortion(c["w"], c["z"], c["nears"], c["fars"], ALPHA)
