"""TEST INFRASTRUCTURE -- differentiable restatements of the operators between the space-time encoders and (sigma, geo_feat, flow).

The density tail (csrc/density_dynamic.hip forward, DensityTailFn + nvsf_density_tail_grad_split backward) and the flow MLP (FlowMlpFn
on nvsf_mlp_fwd / nvsf_mlp_bwd) written as plain torch algebra with a selectable `dtype`, under the rules of tests/torch_f64_static.py
(whose `f16`, `_ReluF16`, `_TruncExp` and `mlp` are imported, not copied):

  * the neighbour blend 0.5 d + 0.25 (d1 + d2) of network_dynamic.py:273-287 is formed as PyTorch forms it from the tensors the
    encoders return: fp32 operations, each rounded once, in the order (d1 + d2), 0.25 *, 0.5 *, +.  When BOTH hash neighbours are fp16
    (`half` = (True, True)) their sum and the 0.25 * product are each rounded to fp16 before the fp32 sum (fp16 + fp16 stays fp16 in
    PyTorch, and so does a Python scalar times fp16); one fp16 neighbour is promoted and nothing is rounded.  The VALUE of the blend is
    this fp32 chain whatever `dtype` is (it decides which fp16 number the network reads, like a cell index); its GRADIENT is the
    linear map (0.5, 0.25, 0.25) in `dtype`.  One tensor handed in as plane_d, plane_1 and plane_2 is the blend its producer formed
    (0.5 v + 0.25 (v + v) = v): it passes unchanged and receives the whole slice of the gradient;
  * the assembled row [plane_s | plane blend | hash_s | hash blend] is rounded to fp16 with a straight-through gradient and followed
    by eight ones (columns 120..127: FullyFusedMLP pads its input with ones);
  * hash_s may come level-major, [8, M, 4]: level l is columns 4 l .. 4 l + 3 of the row;
  * MLP products, trunc_exp and everything behind them are `dtype`; with dtype = float32 the input assembly is bit for bit what
    torch's own fp32 / fp16 kernels compute, which tests/test_dynamic_tail_cpu.py checks against the literal expression.

Nothing a kernel produced is read.  tools/mutate_f64_tail.py applies deliberate errors to a copy of this file; every text it searches
for occurs here exactly once.
"""
import types

import torch

from torch_f64_static import _ReluF16, _TruncExp, f16, mlp  # noqa: F401  (_ReluF16 re-exported: the gate rule of the hidden layers)

W_BASE, W_NEIGHBOUR = 0.5, 0.25  # network_dynamic.py:273-274
N_FEATURES, IN_COLS = 120, 128
FRAGILE = 2.0 ** -20  # a ReLU is "decided" when its pre-activation is at least this fraction of the sum of its |addends| from zero


class _Blend(torch.autograd.Function):
    """0.5 d + 0.25 (d1 + d2): the value in fp32 (fp16 where PyTorch's promotion keeps fp16), the gradient linear in ctx's dtype."""

    @staticmethod
    def forward(ctx, d, d1, d2, half_sum, dtype):
        a, b, c = d.detach().float(), d1.detach().float(), d2.detach().float()
        s = b + c
        if half_sum:
            s = s.half().float()
        q = W_NEIGHBOUR * s
        if half_sum:
            q = q.half().float()
        return (W_BASE * a + q).to(dtype)

    @staticmethod
    def backward(ctx, g):
        return W_BASE * g, W_NEIGHBOUR * g, W_NEIGHBOUR * g, None, None


class _ScaleGrad(torch.autograd.Function):
    """Identity whose gradient is multiplied by a constant."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.k, None


def hash_s_rows(hash_s):
    """[M, 32] rows of the static hash features: as they are, or from the level-major [8, M, 4] form."""
    if hash_s.dim() == 2:
        return hash_s
    order = list(range(hash_s.shape[0]))
    return torch.cat([hash_s[l] for l in order], -1)


def tail_input(plane_s, plane_d, plane_1, plane_2, hash_s, hash_d, hash_1, hash_2, dtype=torch.float64, half=None):
    """The density network's input [M, 128] in `dtype` (fp16 values).  The eight tensors hold fp32 / fp16 values in any float dtype
    (a float64 leaf of an fp16 tensor's values included); half = (hash_1 is fp16, hash_2 is fp16), by default read off their dtypes."""
    if half is None:
        half = (hash_1.dtype == torch.float16, hash_2.dtype == torch.float16)
    if plane_1 is plane_d and plane_2 is plane_d:
        plane_b = _ScaleGrad.apply(plane_d.to(dtype), 1.0)
    else:
        plane_b = _Blend.apply(plane_d, plane_1, plane_2, False, dtype)
    hash_b = _Blend.apply(hash_d, hash_1, hash_2, bool(half[0] and half[1]), dtype)
    row = torch.cat([plane_s.to(dtype), plane_b, hash_s_rows(hash_s).to(dtype), hash_b], -1)
    pad = torch.ones(row.shape[0], IN_COLS - N_FEATURES, dtype=dtype, device=row.device)
    return torch.cat([f16(row), pad], -1)


def _full_width(spec):
    """The spec of an MLP whose input arrives already padded: torch_f64_static.mlp then appends nothing."""
    return types.SimpleNamespace(n_in=spec.in_cols, in_cols=spec.in_cols, split=spec.split)


def density_tail(plane_s, plane_d, plane_1, plane_2, hash_s, hash_d, hash_1, hash_2, w64, spec, dtype=torch.float64, half=None):
    """-> sigma [M] = trunc_exp(h0), geo [M, n_out - 1], the logits h [M, out_cols] and the network input x [M, 128], all `dtype`;
    w64: the flat fp32 parameters of sigma_net as a `dtype` leaf, spec: its MlpSpec (120 -> 64 -> 16)."""
    x = tail_input(plane_s, plane_d, plane_1, plane_2, hash_s, hash_d, hash_1, hash_2, dtype, half)
    h = mlp(x, w64, _full_width(spec))
    return _TruncExp.apply(h[:, 0]), h[:, 1:spec.n_out], h, x


def flow_mlp(x, w0, w1, w2):
    """flow [M, n_out] = W2 relu(W1 relu(W0 x)) on the Linear layers' own [out, in] leaves (dtype of x): fp16-rounded input, weights
    and hidden activations, no padding column (the 32 inputs fill two MFMA steps) and no padded output row."""
    shapes = [tuple(w.shape) for w in (w0, w1, w2)]

    def split(flat):
        mats, o = [], 0
        for a, b in shapes:
            mats.append(flat[o:o + a * b].view(a, b))
            o += a * b
        return mats
    flat = torch.cat([w0.reshape(-1), w1.reshape(-1), w2.reshape(-1)])
    return mlp(x, flat, types.SimpleNamespace(n_in=x.shape[1], in_cols=x.shape[1], split=split))


def fragile_rows(x, mats):
    """bool [M]: rows of the (fp16-valued, padded) network input x whose gradient depends on a coin flip -- some hidden pre-activation
    p = sum_j a_j w_j lies within FRAGILE sum_j |a_j w_j| of zero without being an exact zero, so that the fp32 accumulation of the
    matrix cores may put it on the other side of the ReLU than the float64 sum (precedent: golden_dynamic.fragile_rows).  mats: the
    hidden layers' weight matrices [out, in] (fp16 values, any float dtype); evaluated in float64."""
    a = x.detach().double()
    flag = torch.zeros(a.shape[0], dtype=torch.bool, device=a.device)
    for W in mats:
        W = W.detach().double().half().double()
        p = a @ W.t()
        mag = a.abs() @ W.abs().t()
        flag |= ((p.abs() < FRAGILE * mag) & (p != 0)).any(1)
        a = torch.relu(p).half().double()
    return flag
