"""The depth statistics of DESIGN.md section 9n as DEFINED, in float64 on the CPU: a sequential cumsum, the first crossing, the
formulas, and the gradient by float64 autograd through them; plus the error bars and the input cases the CPU and GPU tests share.

Per ray, from the fp32 inputs held as float64 (w_i >= 0, z_i non-decreasing):
    delta_i = z_{i+1} - z_i (i < T - 1), delta_{T-1} = (far - near) / T;  C_i = w_0 + ... + w_i, C_{-1} = 0, W = C_{T-1}
    tau = q W (normalize) or q;  i* = the first i with C_i >= tau;  t_q = z_{i*} + delta_{i*} (tau - C_{i*-1}) / w_{i*}
    t_q = 0 where W = 0 or (absolute form) W < q
    mode = z_i of the first i with w_i = max w (0 where W = 0);  std = sqrt(sum_i w_i (z_i - mu)^2 / W), mu = sum_i w_i z_i / W (0 where W = 0)
"""
import functools

import torch

EPS64 = 2.0 ** -52


def intervals(z, nears, fars):
    N, T = z.shape
    return torch.cat([z[:, 1:] - z[:, :-1], ((fars - nears) / T).reshape(N, 1)], dim=1)


def quantile_parts(w, z, nears, fars, q, normalize=True):
    """One level on float64 rows -> dict: t [N] (differentiable in w), ok [N], idx [N], and the quantities the bars are made of
    (W, tau, a = tau - C_{i-1}, wi, delta_i, zi, margin = min_i |C_i - tau|)."""
    N, T = w.shape
    delta = intervals(z, nears, fars)
    C = torch.cumsum(w, dim=1)
    W = C[:, -1]
    tau = q * W if normalize else torch.full_like(W, q)
    ok = (W > 0) & (W >= tau)
    hit = C >= tau[:, None]
    idx = torch.where(ok, hit.to(torch.int64).argmax(dim=1), torch.zeros(N, dtype=torch.int64, device=w.device))  # argmax of 0 / 1: the first 1
    pick = lambda m: m.gather(1, idx[:, None])[:, 0]
    c_prev = pick(torch.cat([torch.zeros(N, 1, dtype=w.dtype, device=w.device), C[:, :-1]], dim=1))
    wi = torch.where(ok, pick(w), torch.ones_like(W))
    a = tau - c_prev
    t = torch.where(ok, pick(z) + pick(delta) * a / wi, torch.zeros_like(W))
    margin = torch.where(ok, (C - tau[:, None]).abs().min(dim=1).values, torch.full_like(W, float("inf")))
    return {"t": t, "ok": ok, "idx": idx, "W": W, "tau": tau, "a": a, "wi": wi, "delta": pick(delta), "zi": pick(z), "margin": margin}


def stats(w, z, nears, fars, q=(0.5,), normalize=True):
    """-> dict of float64: quantiles [N, Q], mode [N], std [N], and `parts`, the per-level quantile_parts."""
    w, z, nears, fars = (t.detach().cpu().double() for t in (w, z, nears.reshape(-1), fars.reshape(-1)))
    N, T = w.shape
    parts = [quantile_parts(w, z, nears, fars, float(ql), normalize) for ql in q]
    W = w.sum(dim=1)
    live = W > 0
    Ws = torch.where(live, W, torch.ones_like(W))
    mu = (w * z).sum(dim=1) / Ws
    std = torch.where(live, torch.sqrt((w * (z - mu[:, None]) ** 2).sum(dim=1) / Ws), torch.zeros_like(W))
    first_max = (w == w.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)
    mode = torch.where(live, z.gather(1, first_max[:, None])[:, 0], torch.zeros_like(W))
    return {"quantiles": torch.stack([p["t"] for p in parts], dim=1), "mode": mode, "std": std, "parts": parts, "mu": mu,
            "zmax": z.abs().max(dim=1).values}


def quantile_grad(w, z, nears, fars, q, normalize, grad_q):
    """d (sum grad_q * quantiles) / d w by float64 autograd through the restatement: [N, T]."""
    w, z, nears, fars = (t.detach().cpu().double() for t in (w, z, nears.reshape(-1), fars.reshape(-1)))
    w = w.clone().requires_grad_()
    t = torch.stack([quantile_parts(w, z, nears, fars, float(ql), normalize)["t"] for ql in q], dim=1)
    (g,) = torch.autograd.grad((t * grad_q.double()).sum(), w)
    return g


# ---- bars -------------------------------------------------------------------------------------------------------------------------
# The kernel forms every sum in fp64 and rounds once to fp32.  What separates it from this file is (a) that one rounding, a relative
# 2^-24, and (b) the order of its scan: a parallel and a sequential fp64 sum of T terms that add up to W differ by at most about
# T 2^-53 W each, so tau - C_{i-1} (two such sums) moves by scan_error = T 2^-52 W.
def scan_error(T, W):
    return T * EPS64 * W


def quantile_bar(p, T):
    """|kernel - t| per ray for one level: one fp32 rounding of t, the scan error carried through delta_i / w_i, and 2^-50 (|z_i| +
    delta_i) for the three fp64 operations of the last expression."""
    return 2.0 ** -24 * p["t"].abs() + scan_error(T, p["W"]) * p["delta"].abs() / p["wi"] + 2.0 ** -50 * (p["zi"].abs() + p["delta"].abs())


def settled(p, T):
    """Rays whose crossing a scan error cannot move to a neighbouring sample: margin >= scan_error (and every ray without a crossing)."""
    return p["margin"] >= scan_error(T, p["W"])


def std_bar(s, T):
    """std is the w-weighted L2 norm of z - mu: an error e in mu moves it by at most e (triangle inequality), and mu = M / W carries
    the two sums' order, e <= T 2^-52 max|z|; the norm's own sum adds a relative T 2^-52; then one fp32 rounding."""
    return 2.0 ** -24 * s["std"] + T * EPS64 * (s["std"] + s["zmax"])


def grad_bar(w, z, nears, fars, q, normalize, grad_q, ref):
    """Per entry: one fp32 rounding of the entry; the scan error in a = tau - C_{i-1}, which only the crossing sample's own entry
    holds (delta a / w^2); and 2^-49 of the magnitudes the levels' terms are added up from."""
    w, z, nears, fars = (t.detach().cpu().double() for t in (w, z, nears.reshape(-1), fars.reshape(-1)))
    N, T = w.shape
    bar = 2.0 ** -24 * ref.abs()
    for l, ql in enumerate(q):
        p = quantile_parts(w, z, nears, fars, float(ql), normalize)
        g = grad_q[:, l].double().abs() * p["ok"]
        r = p["delta"].abs() / p["wi"]
        own = torch.zeros(N, T, dtype=torch.float64).scatter_(1, p["idx"][:, None], (g * r / p["wi"])[:, None])
        bar = bar + own * (scan_error(T, p["W"]) + 2.0 ** -49 * p["a"].abs())[:, None] + 2.0 ** -49 * (g * r)[:, None]
    return bar


# ---- cases ------------------------------------------------------------------------------------------------------------------------
KINDS = ("random", "zeros", "plateaus", "hier")
LEVELS = {1: (0.5,), 4: (0.05, 0.25, 0.5, 0.95)}
# partial workgroups of four rays x below / at / across the 64-sample chunk, a carry over several chunks
SHAPES = [(1, 1), (1, 3), (5, 3), (5, 63), (5, 64), (67, 65), (5, 200), (67, 200)]
BIG = (4096, 768)


@functools.lru_cache(maxsize=None)
def case(N, T, kind):
    """-> dict of fp32 CPU inputs w, z [N, T], nears, fars [N]; computed once per case, never modified."""
    gen = torch.Generator().manual_seed(7919 * N + 104729 * T + KINDS.index(kind))
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    nears = 0.01 + 0.05 * rnd(N)
    fars = nears + 0.5 + 0.5 * rnd(N)
    R = (fars - nears)[:, None]
    if kind == "hier":  # non-uniform depths with ties, as a merged coarse + fine row has: a uniform row and draws crowded round one depth
        n_fine = T // 4
        coarse = nears[:, None] + R * (torch.arange(T - n_fine, dtype=torch.float64)[None, :] + 0.5) / max(T - n_fine, 1)
        fine = nears[:, None] + R * (0.3 + 0.4 * rnd(N, 1) + 0.01 * (rnd(N, n_fine) - 0.5))
        z = torch.sort(torch.cat([coarse, fine], dim=1), dim=1).values
        if T > 1:
            z[:, 1] = z[:, 0]
    else:
        z = nears[:, None] + R * torch.sort(0.001 + 0.99 * rnd(N, T), dim=1).values
    w = rnd(N, T) ** 4  # a few strong samples among many weak ones
    w = w / w.sum(dim=1, keepdim=True) * (0.2 + 0.8 * rnd(N, 1))
    if kind == "zeros":  # exact zeros: whole rows, and leading / trailing / scattered samples of the others
        w = w * (rnd(N, T) > 0.5)
        w[:, -1:] = 0.0
        w[::3] = 0.0
    elif kind == "plateaus":  # runs of equal weights of random heights: the arg-max has ties, the CDF equal steps
        w = w[:, torch.arange(T) // 4 * 4]
        w[:, T // 2:] = w.max(dim=1, keepdim=True).values
        w = w / w.sum(dim=1, keepdim=True) * (0.2 + 0.8 * rnd(N, 1))
    out = {"w": w.float(), "z": z.float(), "nears": nears.float(), "fars": fars.float()}
    assert bool((out["z"][:, 1:] >= out["z"][:, :-1]).all()) and bool((out["w"] >= 0).all())
    return out


@functools.lru_cache(maxsize=None)
def reference(N, T, kind, Q, normalize=True):
    c = case(N, T, kind)
    return stats(c["w"], c["z"], c["nears"], c["fars"], LEVELS[Q], normalize)


def grad_seed(N, Q):
    """the upstream gradient the backward cases use: fixed, both signs"""
    gen = torch.Generator().manual_seed(31 * N + Q)
    return (torch.rand(N, Q, generator=gen) - 0.5).float()


def two_surface_ray(T=50):
    """A beam that grazes an edge: 0.45 of the weight at z = 0.2, 0.45 at z = 0.6, dust (0.1 in all) elsewhere; T uniform samples on
    [0, 1).  -> (w, z, nears, fars) fp32 rows of one ray."""
    z = torch.arange(T, dtype=torch.float64) / T
    w = torch.full((T,), 0.1 / (T - 2), dtype=torch.float64)
    w[int(round(0.2 * T))] = 0.45
    w[int(round(0.6 * T))] = 0.45
    z[int(round(0.2 * T))], z[int(round(0.6 * T))] = 0.2, 0.6
    return w.float()[None], z.float()[None], torch.zeros(1), torch.ones(1)


def dyadic_case(N=9, T=130):
    """Weights k / 1024 and depths j / 256 with a last interval of exactly 1 / 256: every sum, tau = q W for q in {1/4, 1/2, 3/4, 1} and
    delta a are exact in fp64, so only the final division and addition round -- identically on either side."""
    gen = torch.Generator().manual_seed(5)
    k = torch.randint(0, 8, (N, T), generator=gen)
    k[0] = 0
    k[1, :-1] = 0
    k[1, -1] = 3                      # all the weight in the last sample
    k[2, 1:] = 0
    k[2, 0] = 5                       # ... in the first
    k[3, T // 2:] = 0                 # zeros behind the last positive sample: q = 1 ends there
    w = k.double() / 1024
    z = torch.cumsum(torch.randint(0, 3, (N, T), generator=gen), dim=1).double() / 256
    nears = torch.zeros(N)
    fars = torch.full((N,), T / 256.0)
    return w.float(), z.float(), nears, fars, (0.25, 0.5, 0.75, 1.0)
