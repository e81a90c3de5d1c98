"""Ray-drop refinement: the reference's U-Net post-process (Trainer.refine, nvsf/nerf/trainer.py:905-1017, and its use in
eval_step, :721-733) around the HIP forward of csrc/unet.hip.

RaydropRefiner is a stand-alone object, NOT a sub-module of the field: the model's parameters(), state_dict(), optimiser groups and
EMA positions stay what they are.  It holds the torch module (nvsf/nerf/models/unet.py), the device copy of its weights packed for
the kernels (BatchNorm folded to scale and shift from the running statistics) and the kernels' workspace.

    r = RaydropRefiner(device)
    r.fit(model, frames, num_steps, ema=step.ema)        # or r.load_from_checkpoint(path)
    p = r(raydrop, intensity, depth)                     # HIP, evaluation mode
    p, gi, gd = r(raydrop, intensity, depth, thres=0.5)  # + intensity * (p > thres), depth * (p > thres) from the same last kernel

The fit is the reference's loop in plain torch (convolution and BatchNorm backward are PyTorch's own).  Deviation from the
reference, as DESIGN.md section 9c does for RANSAC: the random boxes and the frame subset come from a seeded torch.Generator instead
of numpy's global state, and dropout draws from a generator state forked from it, so a fit is reproducible and leaves the global
generators untouched.
"""
import numpy as np
import torch

from nvsf import _hip
from nvsf.nerf.models.unet import UNet

# order of the packed records: include/nvsf_hip.h section 13.  (conv, batch norm in front of it or None)
_RECORDS = (
    [("inc.conv", None)]
    + [(f"down{i}.conv.double_conv.{c}", f"down{i}.conv.double_conv.{c - 3}") for i in (1, 2, 3, 4) for c in (3, 7)]
    + [("attn.proj_qkv", "attn.norm"), ("attn.proj", None)]
    + [(f"up{i}.conv.double_conv.{c}", f"up{i}.conv.double_conv.{c - 3}") for i in (1, 2, 3, 4) for c in (3, 7)]
    + [("outc.conv.2", "outc.conv.0")]
)
_CHUNK = 16  # input channels are padded to the kernels' staging chunk


def fold_batchnorm(bn):
    """Evaluation-mode BatchNorm2d as y = x * scale + shift, from its running statistics and eps (fp32, the module's device)."""
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    return scale, bn.bias.detach().float() - bn.running_mean.detach().float() * scale


def pack_weights(unet):
    """The fp32 vector nvsf_unet_forward reads (layout: include/nvsf_hip.h section 13), on the module's device."""
    mods = dict(unet.named_modules())
    parts = []
    for conv_name, bn_name in _RECORDS:
        conv = mods[conv_name]
        w = conv.weight.detach().float()
        cout, cin, kh, kw = w.shape
        cp = (cin + _CHUNK - 1) // _CHUNK * _CHUNK
        scale, shift = torch.ones(cp, device=w.device), torch.zeros(cp, device=w.device)
        if bn_name is not None:
            scale[:cin], shift[:cin] = fold_batchnorm(mods[bn_name])
        bias = conv.bias.detach().float() if conv.bias is not None else torch.zeros(cout, device=w.device)
        rows = torch.zeros(cp, kh * kw, cout, device=w.device)
        rows[:cin] = w.permute(1, 2, 3, 0).reshape(cin, kh * kw, cout)
        parts += [scale, shift, bias, rows.reshape(-1)]
    return torch.cat(parts).contiguous()


def draw_boxes(H, W, max_boxes, generator):
    """The reference's augmentation boxes (trainer.py:981-989): n in [0, max_boxes) boxes of 1 <= size < int(0.1 * side) per axis (at
    least 1 where a side is shorter than 20), placed so that they end inside the image.  Returns [(y, x, h, w)]."""
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=generator))
    ymax, xmax = max(int(0.1 * H), 2), max(int(0.1 * W), 2)
    boxes = []
    for _ in range(ri(0, max_boxes)):
        bh, bw = ri(1, ymax), ri(1, xmax)
        boxes.append((ri(0, H - bh), ri(0, W - bw), bh, bw))
    return boxes


class RaydropRefiner:
    def __init__(self, device=None, channels=32):
        self.unet = UNet(3, channels, 1).to(device if device is not None else "cpu").eval()
        self._packed = None
        self._ws = {}  # (H, W) -> workspace tensor
        self.fit_lrs = []

    @property
    def device(self):
        return self.unet.inc.conv.weight.device

    # ---- HIP forward ------------------------------------------------------------------------------------------------------
    def repack(self):
        """Packs the module's current weights for the kernels: call after changing them by hand (fit_tensors and
        load_from_checkpoint do)."""
        if self.unet.channels != 32 or self.unet.in_channels != 3 or self.unet.out_channels != 1:
            raise _hip.NvsfHipError("the HIP forward is built for UNet(in_channels=3, channels=32, out_channels=1) only")
        if not self.device.type == "cuda":
            raise _hip.NvsfHipError("the HIP forward needs the module on a HIP device; there is no CPU fallback (torch_forward runs the module)")
        self._packed = pack_weights(self.unet)
        return self._packed

    @staticmethod
    def _planes(raydrop, intensity, depth):
        planes = []
        for t in (raydrop, intensity, depth):
            if not torch.is_tensor(t) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != 1):
                raise ValueError("expected [H, W] or [1, H, W] tensors")
            planes.append(t.reshape(t.shape[-2], t.shape[-1]))
        if not (planes[0].shape == planes[1].shape == planes[2].shape):
            raise ValueError(f"plane shapes differ: {[tuple(p.shape) for p in planes]}")
        return planes

    def __call__(self, raydrop, intensity, depth, thres=None):
        """Refined ray-drop probability of one frame through csrc/unet.hip, in the shape of `raydrop`; with `thres` also
        intensity * (p > thres) and depth * (p > thres)."""
        planes = self._planes(raydrop, intensity, depth)
        H, W = planes[0].shape
        for t in planes:
            if not t.is_cuda:
                raise _hip.NvsfHipError("NVSF HIP kernels need tensors on a HIP device (got a CPU tensor); there is no CPU fallback")
            if t.dtype != torch.float32:
                raise ValueError(f"expected float32 planes, got {t.dtype}")
        if H < 16 or W < 16 or H * W > 1 << 21:
            raise ValueError(f"the U-Net forward needs 16 <= H, W and H * W <= 2^21 (got {H} x {W})")
        if self._packed is None:
            self.repack()
        planes = [t.contiguous() for t in planes]
        ws = self._workspace(H, W)
        prob = torch.empty(H, W, dtype=torch.float32, device=self.device)
        gi = gd = None
        if thres is not None:
            gi, gd = torch.empty_like(prob), torch.empty_like(prob)
        _hip.call("nvsf_unet_forward", _hip.ptr(planes[0]), _hip.ptr(planes[1]), _hip.ptr(planes[2]), H, W, _hip.ptr(self._packed),
                  self._packed.numel(), _hip.ptr(ws), ws.numel() * 4, float(thres if thres is not None else 0.0), _hip.ptr(prob),
                  _hip.ptr(gi), _hip.ptr(gd))
        if thres is None:
            return prob.reshape(raydrop.shape)
        return prob.reshape(raydrop.shape), gi.reshape(intensity.shape), gd.reshape(depth.shape)

    def _workspace(self, H, W):
        ws = self._ws.get((H, W))
        if ws is None:
            if self._packed is None:
                self.repack()
            sizes = np.zeros(2, dtype=np.uint64)
            _hip.call("nvsf_unet_sizes", H, W, sizes.ctypes.data)
            assert int(sizes[1]) == self._packed.numel(), "packed layout disagrees with the library"
            ws = self._ws[(H, W)] = torch.empty(int(sizes[0]) // 4, dtype=torch.float32, device=self.device)
        return ws

    STAGES = ("x0", "x1", "x2", "x3", "x4", "mid", "qkv", "att", "x4a", "u0", "u1", "u2", "u3")

    def stage_views(self, H, W):
        """{name: [C, H_l, W_l] view} of the 13 tensors the HIP forward leaves in its H x W workspace (nvsf_unet_layout: x0 .. x4 =
        inc, down1 .. down4; mid = up4's first convolution; qkv, att, x4a = the attention block; u0 .. u3 = up1 .. up4).  The views
        alias the workspace: valid after a forward at this shape and overwritten by the next one."""
        ws = self._workspace(H, W)
        layout = np.zeros((len(self.STAGES), 4), dtype=np.uint64)
        _hip.call("nvsf_unet_layout", H, W, layout.ctypes.data)
        return {name: ws[int(o):int(o) + int(c) * int(h) * int(w)].view(int(c), int(h), int(w)) for name, (o, c, h, w) in zip(self.STAGES, layout)}

    def torch_forward(self, raydrop, intensity, depth, thres=None):
        """The same through the torch module in evaluation mode, on whatever device the module lives."""
        planes = self._planes(raydrop, intensity, depth)
        was_training = self.unet.training
        self.unet.eval()
        try:
            with torch.no_grad():
                prob = self.unet(torch.stack(planes)[None].float())[0, 0]
        finally:
            self.unet.train(was_training)
        if thres is None:
            return prob.reshape(raydrop.shape)
        mask = (prob > thres).to(prob.dtype)
        return prob.reshape(raydrop.shape), (planes[1] * mask).reshape(intensity.shape), (planes[2] * mask).reshape(depth.shape)

    # ---- fit --------------------------------------------------------------------------------------------------------------
    def fit_tensors(self, unet_input, raydrop_gt, iterations=1000, batch_size=None, lr=1e-3, max_boxes=32, generator=None):
        """The reference's optimisation (trainer.py:956-1008): module in training mode, Adam(lr, no weight decay) under
        OneCycleLR(max_lr=lr, total_steps=iterations), per iteration one mask of fewer than `max_boxes` zeroed boxes over all frames
        and channels, BCELoss against raydrop_gt.  unet_input [F, 3, H, W], raydrop_gt [F, 1, H, W] on the module's device.  Returns
        the losses; `fit_lrs` holds the learning rate of every iteration.  Leaves the module in evaluation mode and, on a HIP device
        at channels = 32, the kernels' weights repacked."""
        if generator is None:
            generator = torch.Generator().manual_seed(0)
        unet_input, raydrop_gt = unet_input.to(self.device).float(), raydrop_gt.to(self.device).float()
        F_, _, H, W = unet_input.shape
        opt = torch.optim.Adam(self.unet.parameters(), lr=lr, weight_decay=0)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=lr, total_steps=iterations)
        bce = torch.nn.BCELoss()
        losses, self.fit_lrs = [], []
        devices = [self.device] if self.device.type == "cuda" else []
        self.unet.train()
        try:
            with torch.random.fork_rng(devices=devices):  # dropout: reproducible, and the global generators are left as they were
                torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=generator)))
                for _ in range(iterations):
                    opt.zero_grad()
                    x, gt = unet_input, raydrop_gt
                    if batch_size is not None:
                        idx = torch.randperm(F_, generator=generator)[:batch_size].to(self.device)
                        x, gt = x[idx], gt[idx]
                    mask = torch.ones(1, 1, H, W, device=self.device)
                    for y0, x0, bh, bw in draw_boxes(H, W, max_boxes, generator):
                        mask[:, :, y0:y0 + bh, x0:x0 + bw] = 0.0
                    loss = bce(self.unet(x * mask), gt)
                    loss.backward()
                    losses.append(float(loss.detach()))
                    self.fit_lrs.append(opt.param_groups[0]["lr"])
                    opt.step()
                    sched.step()
        finally:
            self.unet.eval()
        self._packed = None
        if self.device.type == "cuda" and self.unet.channels == 32:
            self.repack()
        return losses

    def fit(self, model, frames, num_steps, ema=None, **fit_kwargs):
        """Trainer.refine: staged LiDAR render of every frame of `frames` (a FrameSet opened with training=False), under the EMA weights
        when `ema` is given (restored afterwards; the reference drops its average here), the tensors assembled as trainer.py:941-954,
        then fit_tensors."""
        was_training = model.training
        model.eval()
        if ema is not None:
            ema.store()
            ema.copy_to()
        inputs, gts = [], []
        try:
            with torch.no_grad():
                for i in range(len(frames)):
                    data = frames.collate([i])
                    gl = data["images_lidar"]
                    B, H, W, _ = gl.shape
                    o = model.render(data["rays_o_lidar"], data["rays_d_lidar"], data["time"], staged=True, cal_lidar_color=True,
                                     num_steps=num_steps)
                    img = o["image_lidar"].reshape(B, H, W, 2)
                    inputs.append(torch.stack([img[..., 0], img[..., 1], o["depth_lidar"].reshape(B, H, W)], dim=1).float())
                    gts.append(gl[..., 0].reshape(B, 1, H, W).float())
        finally:
            if ema is not None:
                ema.restore()
            model.train(was_training)
        return self.fit_tensors(torch.cat(inputs).contiguous(), torch.cat(gts).contiguous(), **fit_kwargs)

    # ---- checkpoints ------------------------------------------------------------------------------------------------------
    def state_entries(self):
        """The `unet.*` entries of a reference checkpoint's `model` dict (trainer.py:1011-1012 saves them with the field's)."""
        return {"unet." + k: v for k, v in self.unet.state_dict().items()}

    def load_from_checkpoint(self, checkpoint):
        """checkpoint: a path, a checkpoint dict (its `model` entry is read) or a state dict; the `unet.*` keys are loaded strictly."""
        if not isinstance(checkpoint, dict):
            checkpoint = torch.load(checkpoint, map_location=self.device)
        state = checkpoint.get("model", checkpoint)
        own = {k[len("unet."):]: v for k, v in state.items() if k.startswith("unet.")}
        if not own:
            raise KeyError("the checkpoint holds no `unet.*` entries")
        self.unet.load_state_dict(own, strict=True)
        self._packed = None
        if self.device.type == "cuda" and self.unet.channels == 32:
            self.repack()
