"""TEST INFRASTRUCTURE -- the space-time model's density gradient in float64 (nvsf.nerf.normals.density_gradient for NeRFNetwork,
DESIGN.md section 9m), assembled from the existing restatements:

  * K-planes: tests/torch_f64_dynamic.py's plane groups with position carriers (the kernel's piecewise-linear function on its own cell),
    differentiated by autograd;
  * hash grids: tests/hashgrid_gradx_oracle.py (the static 3-D grid, the flow field's 3-D grid with the Lagrange-expanded gradient) and
    tests/hash4d_gradx_oracle.py (the time-sliced 2-D grids);
  * the density MLP and the flow MLP: float64 autograd (tests/torch_f64_static.py's `mlp`, tests/torch_f64_tail.py's `tail_input`).

With u = (x + bound) / (2 bound), f = flow(u, t), p_k = u + f_k at the neighbour times t_k and the blend weights c = (0.5, 0.25, 0.25) (an
absent neighbour is the base evaluation):
    d h0 / d u = a0 + a1 + a2 + J_f(u)^T [a1; a2],
    a0 = d/du [g_ps . plane_s(u) + c0 g_pd . plane_d(u, t) + g_hs . hash_s(u) + c0 g_hd . hash_d(u, t)],
    a_k = d/dp c_k [g_pd . plane_d(p, t_k) + g_hd . hash_d(p, t_k)] at p = p_k,            g = d h0 / d (network input).

rounded = True: the forward's fp16 rounding points (tables, slice features, the neighbours' fp16 regime, the network input, weights
and hidden activations of the density MLP and -- with fp16 -- of the flow MLP); gradients pass straight through them.  rounded = False:
none of them (fp32 master parameters).  In both, with pos_dtype = float32, cells, fracs and the warped positions are the kernels' fp32
ones: u and u + f_k are fp32, f is `flow32` where the caller hands in the flow the model itself evaluated (a warped position decides
cells like an index; the caller on the device passes NeRFNetwork.flow's output) and otherwise the rounded restatement's own flow
rounded to fp32.  pos_dtype = float64 makes every position, cell and frac float64: then the result is the exact derivative of `h0`
below, which is what central differences of it approach.
"""
import numpy as np
import torch

import hash4d_gradx_oracle as H4
import hashgrid_gradx_oracle as GX
import torch_f64_dynamic as D
import torch_f64_static as S
import torch_f64_tail as T

W = (T.W_BASE, T.W_NEIGHBOUR, T.W_NEIGHBOUR)


def _f64(p):
    return p.detach().cpu().double()


def _slot(t_host, R, reciprocal):
    from nvsf.nerf.models.hash_field import TimeSlot
    k1, k2, b_lo, b_hi, lag = D.time_constants(t_host, R, reciprocal)
    return TimeSlot(k1, k2, None, b_lo, b_hi, k1 == k2, lag)


def _plane_group(pos, carrier3, P, res_host, grp):
    car = None if carrier3 is None else [carrier3[:, d] for d in range(3)] + [None]
    return D._plane_group(pos, car, P, res_host, grp, torch.float64, False)


def _plain_mlp(a, mats):
    """relu MLP in float64 on the master weights -> (output, [hidden gates])."""
    gates = []
    for Wm in mats[:-1]:
        z = a @ Wm.t()
        gates.append(z > 0)
        a = torch.relu(z)
    return a @ mats[-1].t(), gates


def plane_face_margin(p, res_host):
    """min over scales and spatial axes of the distance of p [M, 3] from the nearest texel boundary of the K-planes, in units of p."""
    p = np.asarray(p, np.float64)
    m = np.full(p.shape[0], np.inf)
    for s in range(len(res_host) // 4):
        for d in range(3):
            R = int(res_host[4 * s + d])
            u = p[:, d] * (R - 1)
            fr = u - np.floor(u)
            m = np.minimum(m, np.minimum(fr, 1.0 - fr) / (R - 1))
    return m


def evaluate(model, u, t_host, lidar, rounded=True, fp16=True, flow_jacobian=True, flow32=None, pos_dtype=np.float32, want_grad=True):
    """u [M, 3]: positions in the unit cube, a CPU tensor of dtype float32 (pos_dtype = float32) or float64 (pos_dtype = float64);
    model: a NeRFNetwork on the CPU (its parameters are read, nothing is launched).  -> dict of numpy float64 arrays:
    "h0" [M], "sigma" [M], "dh" [M, 3] = d h0 / d u, "a" [M, 6] = [a1 | a2], "flow" [M, 6], "margin" [M] (the distance of the three
    positions from the nearest cell face of any grid, in units of u) and "gates" [M, n] bool (the hidden ReLU gates of both MLPs)."""
    from nvsf.nerf.models.hash_field import lagrange_weights_host, neighbour_frames
    exact = pos_dtype == np.float64
    assert not (exact and rounded), "the rounded restatement takes its decisions in fp32"
    tdt = torch.float64 if exact else torch.float32
    u = u.detach().cpu().to(tdt)
    M = u.shape[0]
    t_host = float(np.float32(t_host))
    frame_idx = int(np.float32(t_host) * np.float32(model.num_frames - 1))
    nb = neighbour_frames(frame_idx, model.num_frames)
    hash_enc = model.hash_encoder_lidar if lidar else model.hash_encoder_camera
    planes_enc = model.planes_encoder_lidar if lidar else model.planes_encoder_camera
    res_host = [int(r) for r in planes_enc._res_host]
    P = _f64(planes_enc.planes_cl)
    R = hash_enc.hash_dynamic[0].time_resolution
    specs = [pl.hash_t[0].spec for pl in hash_enc.hash_dynamic]
    spec_s, spec_f = hash_enc.hash_static.spec, model.flow_net.grid_enc.spec
    tab = (lambda p: _f64(p).half().numpy()) if rounded else (lambda p: _f64(p).numpy())  # what the derivative oracles read
    tab_s, tab_f = tab(hash_enc.hash_static.params), tab(model.flow_net.grid_enc.params)

    def slice_tabs(slot):
        return [tab(pl.hash_t[k].params) for k in (slot.k1, slot.k2) for pl in hash_enc.hash_dynamic]
    slot0 = _slot(t_host, R, True)
    slots = [None if n is None else _slot(n[1], R, False) for n in nb]
    un = u.numpy()

    # ---- the flow field
    w_lag = lagrange_weights_host(t_host, 4, True)
    if rounded:
        red = D.flow_grid_features(u, _f64(model.flow_net.grid_enc.params), spec_f, t_host, True).detach()
    else:
        f = torch.from_numpy(GX.features(un, tab_f, spec_f, pos_dtype)).view(M, spec_f.L, 4, 2)
        red = sum(float(np.float32(w_lag[i])) * f[:, :, i, :] for i in range(4)).reshape(M, 2 * spec_f.L)
    red = red.clone().requires_grad_(want_grad)
    lin = [_f64(m.weight) for m in model.flow_net.mlp if isinstance(m, torch.nn.Linear)]
    if rounded and fp16:
        flow, flow_gates = T.flow_mlp(red, *lin), []
    else:
        flow, flow_gates = _plain_mlp(red, lin)
    fl = flow.detach()
    if exact:
        warp = fl
    else:
        warp = fl.float() if flow32 is None else flow32.detach().cpu().float()
    pos = [u] + [None if n is None else u + warp[:, n[2]:n[2] + 3] for n in nb]  # fp32 sums (float64 when exact)
    t_col = lambda p, t: torch.cat([p, torch.full_like(p[:, :1], float(np.float32(t)))], -1)
    times = [t_host] + [None if n is None else float(n[0]) for n in nb]

    # ---- features: the planes with position carriers, the hash grids as values
    car = [torch.zeros(M, 3, dtype=torch.float64, requires_grad=True) if (p is not None and want_grad) else None for p in pos]
    plane_s = _plane_group(t_col(pos[0], times[0]), car[0], P, res_host, 0)
    plane_d = [None if p is None else _plane_group(t_col(p, times[k]), car[k], P, res_host, 1) for k, p in enumerate(pos)]
    if rounded:
        tabs64 = [[_f64(pl.hash_t[k].params) for k in range(R)] for pl in hash_enc.hash_dynamic]
        hash_s = D.grid_features(u, _f64(hash_enc.hash_static.params), spec_s, (0, 1, 2)).reshape(M, -1).detach()
        hash_d = [D.hash_time_features(u, tabs64, specs, R, t_host, True).detach()]
        hash_d += [None if n is None else D.hash_time_features_f16(pos[k + 1], tabs64, specs, R, n[1], False).double() for k, n in enumerate(nb)]
    else:
        hash_s = torch.from_numpy(GX.features(un, tab_s, spec_s, pos_dtype).reshape(M, -1))
        hash_d = [torch.from_numpy(H4.features(un, slice_tabs(slot0), specs, slot0, pos_dtype))]
        hash_d += [None if n is None else torch.from_numpy(H4.features(pos[k + 1].numpy(), slice_tabs(slots[k]), specs, slots[k], pos_dtype))
                   for k, n in enumerate(nb)]

    # ---- the density tail on leaves of the feature values: their gradients are g times the blend weights
    leaf = lambda v: v.detach().clone().requires_grad_(want_grad)
    ps, hs = leaf(plane_s), leaf(hash_s)
    pd = [None if v is None else leaf(v) for v in plane_d]
    hd = [None if v is None else leaf(v) for v in hash_d]
    pick = lambda seq, k: seq[0] if seq[k] is None else seq[k]  # an absent neighbour is the base evaluation
    net = model.sigma_net
    w64 = _f64(net.params)
    if rounded:
        x = T.tail_input(ps, pd[0], pick(pd, 1), pick(pd, 2), hs, hd[0], pick(hd, 1), pick(hd, 2), torch.float64,
                         half=(nb[0] is not None, nb[1] is not None))
        h, gates = S.mlp(x, w64, T._full_width(net.spec)), []
    else:
        row = torch.cat([ps, W[0] * pd[0] + W[1] * (pick(pd, 1) + pick(pd, 2)), hs, W[0] * hd[0] + W[1] * (pick(hd, 1) + pick(hd, 2)),
                         torch.ones(M, net.spec.in_cols - net.spec.n_in, dtype=torch.float64)], -1)
        mats = net.spec.split(w64)
        h, gates = _plain_mlp(row, mats)
        habs = row.detach().abs()  # the sum of |addend| behind h0: what the rounding error of a float64 evaluation is proportional to
        for Wm in mats[:-1]:
            habs = habs @ Wm.abs().t()
        habs = (habs @ mats[-1].abs().t())[:, 0].numpy()
    h0 = h[:, 0].detach().numpy()
    margin = np.minimum(GX.face_margin(un, spec_s), GX.face_margin(un, spec_f))
    for p in pos:
        if p is not None:
            margin = np.minimum(margin, np.minimum(H4.face_margin(p.numpy(), specs), plane_face_margin(p.numpy(), res_host)))
    out = {"h0": h0, "sigma": np.exp(h0), "flow": fl.numpy(), "margin": margin,
           "gates": torch.cat([g.reshape(M, -1) for g in gates + flow_gates], -1).numpy() if (gates or flow_gates) else np.zeros((M, 0), bool)}
    if not rounded:
        out["habs"] = habs
    if not want_grad:
        return out

    # ---- the chain rule
    h[:, 0].sum().backward()
    total = (ps.grad * plane_s).sum()
    for k in range(3):
        if plane_d[k] is not None:
            total = total + (pd[k].grad * plane_d[k]).sum()
    total.backward()
    a = [c.grad.numpy().copy() if c is not None else np.zeros((M, 3)) for c in car]
    a[0] += GX.grad_x(un, tab_s, spec_s, hs.grad.numpy().reshape(M, spec_s.L, spec_s.F), pos_dtype)[0]
    a[0] += H4.grad_x(un, slice_tabs(slot0), specs, slot0, hd[0].grad.numpy(), 1.0, pos_dtype)[0]
    for k, n in enumerate(nb):
        if n is not None:
            a[k + 1] += H4.grad_x(pos[k + 1].numpy(), slice_tabs(slots[k]), specs, slots[k], hd[k + 1].grad.numpy(), 1.0, pos_dtype)[0]
    dh = a[0] + a[1] + a[2]
    a6 = np.concatenate([a[1], a[2]], -1)
    if flow_jacobian and (nb[0] is not None or nb[1] is not None):
        (g_red,) = torch.autograd.grad(flow, red, torch.from_numpy(a6))
        g8 = g_red.numpy().reshape(M, spec_f.L, 1, 2) * np.array([float(np.float32(v)) for v in w_lag]).reshape(1, 1, 4, 1)
        dh = dh + GX.grad_x(un, tab_f, spec_f, g8.reshape(M, spec_f.L, 8), pos_dtype)[0]
    out.update(dh=dh, a=a6)
    return out


def field_gradient_f64(model, x_world, time, lidar, rounded=True, fp16=True, flow_jacobian=True, flow32=None):
    """(sigma [M], grad [M, 3]) numpy float64 at the world-space points x_world [M, 3] (a CPU fp32 tensor) and the frame time `time`:
    grad = clamp(sigma, e^-15, e^15) d h0 / d u / (2 bound), u normalised in fp32 as NeRFNetwork.density normalises."""
    u = (x_world.detach().cpu().float() + model.bound) / (2 * model.bound)
    r = evaluate(model, u, time, lidar, rounded, fp16, flow_jacobian, flow32)
    return r["sigma"], np.clip(r["sigma"], S._LO, S._HI)[:, None] * r["dh"] / (2.0 * float(model.bound))
