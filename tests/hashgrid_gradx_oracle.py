"""TEST INFRASTRUCTURE -- numpy float64 statement of the hash grid's coordinate gradient (nvsf_hashgrid_grad_x).

For sample m the function differentiated is the piecewise-multilinear function the forward evaluates, on the kernel's own cell:
    pos_d = fmaf(scale_l, x_d, 0.5f), cell_d = floorf(pos_d), frac_d = pos_d - cell_d, w_d(0) = 1 - frac_d, w_d(1) = frac_d
    dL/dx_d[m] = sum_l scale_l sum_f g[m, l, f] sum_{c in {0,1}^D} s_d(c) prod_{e != d} w_e(c_e) table[row(l, cell + c)][f],  s_d(c) = +-1
Cells and fracs are formed in fp32 as tests/torch_f64_static.py::_corners forms them (the float64 product plus 0.5, rounded once --
the value of the fused multiply-add); rows are the kernel's 32-bit index arithmetic; everything after that is float64.
`grad_x` also returns A[m, d], the sum of the absolute values of the addends of each output: what a bound on an fp32 sum in any
order is proportional to.  `features` is the float64 function itself (positions float64 throughout), for finite differences.
"""
import numpy as np

_PRIMES = (1, 2654435761, 805459861)
_U32 = 0xFFFFFFFF


def cells(x, scale, pos_dtype=np.float32):
    """(cell [M, D] int64, frac [M, D] float64) of x [M, D] at one level.  pos_dtype = float32: pos rounded once to fp32, as the kernel
    forms it (x must then hold fp32 values); float64: no rounding (the float64 feature function)."""
    pos = (np.asarray(x, np.float64) * float(np.float32(scale)) + 0.5).astype(pos_dtype)
    cell = np.floor(pos)
    frac = pos - cell  # exact in either format
    return cell.astype(np.int64), frac.astype(np.float64)


def rows(cc, res, n_rows):
    """Table row inside the level of the grid vertices cc [M, D] int64 (any integers): grid_row of csrc/hashgrid_device.h in its own
    uint32 arithmetic -- dense index while res^D fits the level's table, spatial hash otherwise, modulo the level's rows."""
    D = cc.shape[1]
    u = cc & _U32  # (uint32_t)(int32_t)floor
    if res ** D <= n_rows:
        idx = np.zeros(cc.shape[0], np.int64)
        for d in range(D):
            idx = (idx + u[:, d] * (res ** d)) & _U32
    else:
        idx = np.zeros(cc.shape[0], np.int64)
        for d in range(D):
            idx = idx ^ ((u[:, d] * _PRIMES[d]) & _U32)
    return idx % n_rows


def _level(spec, l):
    off = int(spec.offsets[l])
    return float(np.float32(spec.scales[l])), int(spec.res[l]), off, int(spec.offsets[l + 1]) - off


def grad_x(x, table, spec, g, pos_dtype=np.float32):
    """x [M, D] (fp32 values), table [n_rows F] (the values the kernel reads: pass the fp16 copy), g [M, L, F]
    -> (dL/dx [M, D] float64, A [M, D] float64)."""
    D, L, F = spec.D, spec.L, spec.F
    x = np.asarray(x)
    M = x.shape[0]
    tab = np.asarray(table).astype(np.float64).reshape(-1, F)
    g = np.asarray(g, np.float64).reshape(M, L, F)
    out, A = np.zeros((M, D)), np.zeros((M, D))
    for l in range(L):
        scale, res, off, n_rows = _level(spec, l)
        cell, frac = cells(x, scale, pos_dtype)
        for c in range(1 << D):
            bits = [(c >> d) & 1 for d in range(D)]
            v = tab[off + rows(cell + np.array(bits, np.int64)[None, :], res, n_rows)]  # [M, F]
            for d in range(D):
                w = np.ones(M)
                for e in range(D):
                    if e != d:
                        w = w * (frac[:, e] if bits[e] else 1.0 - frac[:, e])
                addends = (scale * (1.0 if bits[d] else -1.0)) * g[:, l, :] * w[:, None] * v
                out[:, d] += addends.sum(-1)
                A[:, d] += np.abs(addends).sum(-1)
    return out, A


def features(x, table, spec, pos_dtype=np.float64):
    """The encoded features [M, L, F] in float64 (no fp16 rounding of the result); positions float64 unless pos_dtype says otherwise."""
    D, L, F = spec.D, spec.L, spec.F
    x = np.asarray(x, np.float64)
    M = x.shape[0]
    tab = np.asarray(table).astype(np.float64).reshape(-1, F)
    out = np.zeros((M, L, F))
    for l in range(L):
        scale, res, off, n_rows = _level(spec, l)
        cell, frac = cells(x, scale, pos_dtype)
        for c in range(1 << D):
            bits = [(c >> d) & 1 for d in range(D)]
            w = np.ones(M)
            for d in range(D):
                w = w * (frac[:, d] if bits[d] else 1.0 - frac[:, d])
            out[:, l, :] += w[:, None] * tab[off + rows(cell + np.array(bits, np.int64)[None, :], res, n_rows)]
    return out


def face_margin(x, spec):
    """min over levels and axes of the distance of pos from the nearest cell face, in units of x (distance / scale_l): a step
    smaller than this keeps x +- step inside the cell on every level.  [M]."""
    x = np.asarray(x, np.float64)
    m = np.full(x.shape[0], np.inf)
    for l in range(spec.L):
        scale = _level(spec, l)[0]
        _, frac = cells(x, scale, np.float64)
        m = np.minimum(m, (np.minimum(frac, 1.0 - frac) / scale).min(-1))
    return m


def field_gradient_f64(model, x_world, lidar, rounded=True):
    """Float64 gradient of the restated static density field sigma(x) = exp(mlp(hash_features(x01))[0]) at the world-space points
    x_world [M, 3] (a CPU fp32 tensor): -> (sigma [M], grad [M, 3]) numpy float64, grad = clamp(sigma) d h0 / d x01 / (2 bound).
    rounded = True: tests/torch_f64_static.py's hash_features -> mlp with the forward's fp16 rounding points (table, encoded features,
    MLP input, hidden activations, weights; gradients pass straight through them); False: the same chain with none of them (fp32
    master parameters, no rounding of features or activations).  Cells and fracs are the kernel's fp32 ones in both.  d h0 / d features
    is autograd's float64 gradient of the MLP, d features / d x01 is `grad_x` above."""
    import torch
    import torch_f64_static as S
    enc = model.hash_encoder_lidar if lidar else model.hash_encoder_camera
    net = model.sigma_net
    x01 = (x_world.detach().cpu().float() + model.bound) / (2 * model.bound)  # as NeRFNetworkStatic.density normalises, fp32
    table64, w64 = enc.params.detach().cpu().double(), net.params.detach().cpu().double()
    spec = enc.spec
    if rounded:
        table = table64.half().numpy()
        feat = S.hash_features(x01, table64, spec).detach().requires_grad_()
        h = S.mlp(feat, w64, net.spec)
    else:
        table = table64.numpy()
        feat = torch.from_numpy(features(x01.numpy(), table, spec, pos_dtype=np.float32).reshape(x01.shape[0], -1)).requires_grad_()
        a = torch.cat([feat, torch.ones(feat.shape[0], net.spec.in_cols - net.spec.n_in, dtype=torch.float64)], -1)
        mats = net.spec.split(w64)
        for W in mats[:-1]:
            a = torch.relu(a @ W.t())
        h = a @ mats[-1].t()
    h[:, 0].sum().backward()
    dh, _ = grad_x(x01.numpy(), table, spec, feat.grad.numpy().reshape(-1, spec.L, spec.F))
    sigma = torch.exp(h[:, 0].detach())
    grad = sigma.clamp(S._LO, S._HI).numpy()[:, None] * dh / (2.0 * float(model.bound))
    return sigma.numpy(), grad
